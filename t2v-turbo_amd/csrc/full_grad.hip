// Parameter gradients of the base weights for FULL fine-tuning of the student UNet (train_latent_t2v_turbo_v2.py:798-816 param
// groups, :1262 accelerator.backward: every UNet parameter is trainable there, not only LoRA tensors).  Two pieces that the
// token-contracted weight-gradient kernel (wgrad_tn.hip: dW = dy^T x) does not cover by itself:
//
//  * t2v_im2col_bf16 — the shifted-row matrix of a conv leaf, xcol[m][tap * C + c] = x[src(m, tap)][c] (zero outside the grid), in the
//    K order of the forward's tap-major weight pack, for every gather mode of t2v_gemm (3x3 stride 1 / stride 2 / stride 2 padded
//    right-bottom / over the nearest-x2 upsampled input, (3,1,1) temporal).  dW[n][tap][c] = sum_m dy[m][n] xcol[m][tap * C + c] is then
//    ONE t2v_wgrad_tn product (openaimodel3d.py:155-159,179-184 ResBlock convs, :63-79 Down/Upsample, :257-309 TemporalConvBlock under
//    autograd).  HBM-bound copy: 2 C bytes in, 2 taps C bytes out per output row.
//  * t2v_norm_affine_grad — the per-channel reductions over token rows that the normalisation layers' affine parameters, every bias
//    and the time-embedding row vector need:
//        dgamma[u][c] = sum_{rows of u} dz[m][c] xhat[m][c],   dbeta[u][c] = sum_{rows of u} dz[m][c]
//    with xhat from GroupNorm statistics ((mean, rstd) per (unit, group): lvdm/basics.py:78-89 GroupNormSpecific) or recomputed per row
//    (LayerNorm: attention.py:300-311), dz = dy, or dy * silu'(xhat gamma + beta) where the forward applied SiLU after the norm
//    (openaimodel3d.py:223-254 in_layers / out_layers), or plain column sums of dy (kind 2: biases; per-clip sums = d(loss)/d(emb)).
//    `sum_rows` consecutive rows make one output row u.  Two launches: per-block partial sums in a fixed order, then their sum in block
//    order — deterministic, no float atomics.  HBM-bound: reads x and dy once.
//  * t2v_repack_conv_f32 — the weights move every optimizer step, so the bf16 packs the recorded launch lists point at are re-made per step
//    (engine.Packer.refresh): a conv leaf's fp32 parameter [N][C][taps] into its tap-major forward pack [N][taps][C] or its data-gradient
//    pack [C][taps flipped][N], cast included, through an LDS tile so that both sides are coalesced (torch's strided cast-and-copy did
//    37 us per pack, ~ 300 GB/s: profiles/r06_full_finetune_kernel_stats.csv).
//  * t2v_rowlin_fwd / t2v_rowlin_bwd_data / t2v_rowlin_wgrad — the B-row conditioning branch of the training routes (time / fps / guidance
//    MLPs and every ResBlock's SiLU -> Linear emb_layers: openaimodel3d.py:683-706,172-178; their LoRA branches: utils/lora.py:45-50), B <= 8
//    rows, on the fp32 master parameters IN PLACE: no packs, no refresh, fp32 arithmetic end to end.  Every kernel reads or writes each
//    weight-sized array once with 16-byte accesses (HBM-bound: the 22 emb_layers weights are ~ 103 MB at full width); a table of problems
//    per launch (all emb_layers in one), fixed summation order, no float atomics.  The row counts per workgroup below are first choices,
//    not tuned ones: nothing here has been timed against an alternative.
#include "common.h"
#include <math.h>

namespace {

constexpr int IM_KIND_S1 = T2V_GEMM_CONV3X3, IM_KIND_S2 = T2V_GEMM_CONV3X3_S2, IM_KIND_UP2 = T2V_GEMM_CONV3X3_UP2, IM_KIND_T = T2V_GEMM_TCONV3,
              IM_KIND_S2P = T2V_GEMM_CONV3X3_S2_PAD01;

// one thread per 16-byte chunk (8 channels) of one (output row, tap)
__global__ __launch_bounds__(256) void im2col_kernel(const bf16_t* __restrict__ x0, int c0, int ld0, const bf16_t* __restrict__ x1, int c1, int ld1,
                                                     int mode, int n_img, int h, int w, int ho, int wo, int frames, int taps,
                                                     bf16_t* __restrict__ out, int ldo, long long total) {
    const int C = c0 + c1, cpr = C >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ci = (int)(i % cpr);
        const long long mt = i / cpr;
        const int tap = (int)(mt % taps);
        const long long m = mt / taps;
        long long src = -1;
        if (mode == IM_KIND_T) {
            const int hw = h * w;
            const long long img = m / hw;            // (clip, frame)
            const int f = (int)(img % frames), sf = f + tap - 1;
            if (sf >= 0 && sf < frames) src = m + (long long)(tap - 1) * hw;
        } else {
            const int xo = (int)(m % wo), yo = (int)((m / wo) % ho);
            const long long img = m / ((long long)wo * ho);
            const int ty = tap / 3, tx = tap - 3 * ty;
            int sy, sx;
            bool ok;
            if (mode == IM_KIND_S1) { sy = yo + ty - 1; sx = xo + tx - 1; ok = sy >= 0 && sy < h && sx >= 0 && sx < w; }
            else if (mode == IM_KIND_S2) { sy = 2 * yo + ty - 1; sx = 2 * xo + tx - 1; ok = sy >= 0 && sy < h && sx >= 0 && sx < w; }
            else if (mode == IM_KIND_S2P) { sy = 2 * yo + ty; sx = 2 * xo + tx; ok = sy < h && sx < w; }
            else { const int uy = yo + ty - 1, ux = xo + tx - 1; ok = uy >= 0 && uy < 2 * h && ux >= 0 && ux < 2 * w; sy = uy >> 1; sx = ux >> 1; }
            if (ok) src = (img * h + sy) * (long long)w + sx;
        }
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (src >= 0) {
            const int c = ci * 8;
            v = c < c0 ? *(const uint4*)(x0 + src * ld0 + c) : *(const uint4*)(x1 + src * ld1 + (c - c0));
        }
        *(uint4*)(out + m * ldo + (long long)tap * C + ci * 8) = v;
    }
}

// ---- per-channel row reductions ------------------------------------------------------------------------------------------------------
// Block = 4 waves; a wave owns whole rows (lane l holds the 16-byte chunks l, l + 64, ... of the row: NJ of them), so a LayerNorm's row
// statistics are two butterflies.  Block (bx, u) walks rows [bx * rows_per_blk, ...) of output row u; its four waves' register sums meet
// in LDS in wave order; partial[(u * nblk + bx)][2][C].
constexpr int AG_MAXJ = 5;   // C <= 64 * 8 * 5 = 2560 per launch (the widest GroupNorm: a 1280 + 1280 concat); plain column sums go out in column chunks
// NJ = chunks per lane (1, 2, 3, 5 by width), UR = rows a wave has in flight per trip (4 / 2 / 1): the first form (NJ = 5 for every width, one
// row per trip, the GroupNorm group of every element by an integer division per row) kept ~ 200 registers and 1.3 KB per wave in flight and
// ran at ~ 1 TB/s (profiles/r06_full_finetune_kernel_stats.csv: 55 us per GroupNorm launch).  Rows are still taken in the order
// r, r + 4, r + 8, ... per wave: the sums are bit-identical to the first form's.
template <int KIND, int NJ, int UR>   // KIND 0: GroupNorm statistics given, 1: LayerNorm (row statistics recomputed), 2: column sums of dy only
__global__ __launch_bounds__(256) void affine_grad_partial_kernel(const bf16_t* __restrict__ x0, int c0, int ld0, const bf16_t* __restrict__ x1,
                                                                  int c1, int ld1, long long sum_rows, int rows_per_blk, int rows_per_unit,
                                                                  int groups, const float* __restrict__ stats, float ln_eps,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta, int silu,
                                                                  const bf16_t* __restrict__ dy, int ldy, float* __restrict__ partial) {
    const int C = c0 + c1, cpr = C >> 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.y, bx = blockIdx.x, nblk = gridDim.x;
    const long long r_begin = (long long)u * sum_rows + (long long)bx * rows_per_blk;
    const long long r_end = min((long long)(u + 1) * sum_rows, r_begin + rows_per_blk);
    float ag[NJ][8], ab[NJ][8];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) { ag[j][e] = 0.f; ab[j][e] = 0.f; }
    const int cpg = KIND == 0 ? C / groups : 1;
    const float inv_c = 1.0f / (float)C;
    // GroupNorm: with >= 8 channels per group a chunk lies in at most two groups — the first one and where the second begins, once per lane
    const bool two_groups = KIND == 0 && cpg >= 8;
    int glo[NJ], eb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = (lane + 64 * j) * 8;
        glo[j] = KIND == 0 ? c / cpg : 0;
        eb[j] = KIND == 0 ? (glo[j] + 1) * cpg - c : 8;   // elements e >= eb are in group glo + 1
    }
    for (long long r0 = r_begin + wave; r0 < r_end; r0 += 4 * UR) {
        uint4 xr[UR][NJ], dr[UR][NJ];
#pragma unroll
        for (int k = 0; k < UR; ++k) {
            const long long r = r0 + 4 * k;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ci = lane + 64 * j;
                xr[k][j] = make_uint4(0u, 0u, 0u, 0u); dr[k][j] = make_uint4(0u, 0u, 0u, 0u);
                if (r < r_end && ci < cpr) {
                    dr[k][j] = *(const uint4*)(dy + r * ldy + ci * 8);
                    if (KIND != 2) {
                        const int c = ci * 8;
                        xr[k][j] = c < c0 ? *(const uint4*)(x0 + r * ld0 + c) : *(const uint4*)(x1 + r * ld1 + (c - c0));
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < UR; ++k) {
            const long long r = r0 + 4 * k;
            if (r >= r_end) break;
            float xv[NJ][8], dv[NJ][8];
#pragma unroll
            for (int j = 0; j < NJ; ++j) { unpack8(dr[k][j], dv[j]); unpack8(xr[k][j], xv[j]); }
            float mean = 0.f, rstd = 1.f;
            if (KIND == 1) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) s += xv[j][e];
                mean = wave_sum(s) * inv_c;
                float q = 0.f;
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    if (lane + 64 * j < cpr) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const float dlt = xv[j][e] - mean; q += dlt * dlt; }
                    }
                rstd = rsqrtf(wave_sum(q) * inv_c + ln_eps);
            }
            const long long unit = KIND == 0 ? r / rows_per_unit : 0;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ci = lane + 64 * j;
                if (ci < cpr) {
                    float gm[8], bt[8];   // (re-read per row from L1: kept in registers beside the sums they would not fit at 2560 channels)
                    if (KIND != 2 && silu) {
                        const float4 g0 = *(const float4*)(gamma + ci * 8), g1 = *(const float4*)(gamma + ci * 8 + 4);
                        const float4 b0 = *(const float4*)(beta + ci * 8), b1 = *(const float4*)(beta + ci * 8 + 4);
                        gm[0] = g0.x; gm[1] = g0.y; gm[2] = g0.z; gm[3] = g0.w; gm[4] = g1.x; gm[5] = g1.y; gm[6] = g1.z; gm[7] = g1.w;
                        bt[0] = b0.x; bt[1] = b0.y; bt[2] = b0.z; bt[3] = b0.w; bt[4] = b1.x; bt[5] = b1.y; bt[6] = b1.z; bt[7] = b1.w;
                    }
                    float2 s_lo = make_float2(0.f, 1.f), s_hi = s_lo;
                    if (two_groups) {
                        const float* st = stats + (unit * groups + glo[j]) * 2;
                        s_lo = *(const float2*)st;
                        if (eb[j] < 8) s_hi = *(const float2*)(st + 2);
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float xh = 0.f, dz = dv[j][e];
                        if (KIND == 0) {
                            float2 st2;
                            if (two_groups) st2 = e < eb[j] ? s_lo : s_hi;
                            else st2 = *(const float2*)(stats + (unit * groups + (ci * 8 + e) / cpg) * 2);
                            xh = (xv[j][e] - st2.x) * st2.y;
                        } else if (KIND == 1) {
                            xh = (xv[j][e] - mean) * rstd;
                        }
                        if (KIND != 2 && silu) {   // y = silu(z), z = xhat gamma + beta: dz = dy * sigma(z) (1 + z (1 - sigma(z)))
                            const float z = xh * gm[e] + bt[e];
                            const float sg = 1.0f / (1.0f + __expf(-z));
                            dz *= sg * (1.0f + z * (1.0f - sg));
                        }
                        ag[j][e] += dz * xh;
                        ab[j][e] += dz;
                    }
                }
            }
        }
    }
    // the four waves' sums, added in wave order
    extern __shared__ float red[];   // [4][2][C]
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int ci = lane + 64 * j;
        if (ci < cpr) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                red[(wave * 2 + 0) * C + ci * 8 + e] = ag[j][e];
                red[(wave * 2 + 1) * C + ci * 8 + e] = ab[j][e];
            }
        }
    }
    __syncthreads();
    float* dst = partial + ((long long)u * nblk + bx) * 2 * C;
    for (int i = threadIdx.x; i < 2 * C; i += 256) dst[i] = ((red[i] + red[2 * C + i]) + red[4 * C + i]) + red[6 * C + i];
}

// out[u][i] = sum over the unit's blocks.  Block (x, u) owns 64 consecutive values i (coalesced rows of the partial array); its 16
// waves take the blocks b = wave, wave + 16, ... (four loads in flight per trip), meet in LDS and are added in wave order: a fixed
// summation tree, deterministic.  (The first form walked all blocks with ONE thread per value: 116 us per call on ~1 000 blocks — a
// third of the full fine-tuning step, profiles/r06_full_finetune_kernel_stats.csv.)
constexpr int AGF_WAVES = 16;
__global__ __launch_bounds__(AGF_WAVES * 64) void affine_grad_final_kernel(const float* __restrict__ partial, int nblk, int C, float* __restrict__ dgamma,
                                                                           int ld_g, float* __restrict__ dbeta, int ld_b) {
    __shared__ float red[AGF_WAVES][64];
    const int u = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const bool ok = i < 2 * C;
    const float* src = partial + (long long)u * nblk * 2 * C + (ok ? i : 0);
    const long long stride = 2LL * C;
    float s = 0.f;
    int b = wave;
    for (; b + 3 * AGF_WAVES < nblk; b += 4 * AGF_WAVES) {
        const float v0 = src[(long long)b * stride], v1 = src[(long long)(b + AGF_WAVES) * stride];
        const float v2 = src[(long long)(b + 2 * AGF_WAVES) * stride], v3 = src[(long long)(b + 3 * AGF_WAVES) * stride];
        s += v0; s += v1; s += v2; s += v3;
    }
    for (; b < nblk; b += AGF_WAVES) s += src[(long long)b * stride];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && ok) {
        float t = red[0][lane];
#pragma unroll
        for (int w = 1; w < AGF_WAVES; ++w) t += red[w][lane];
        if (i < C) { if (dgamma) dgamma[(long long)u * ld_g + i] = t; }
        else if (dbeta) dbeta[(long long)u * ld_b + (i - C)] = t;
    }
}

// ---- conv weight packs from the fp32 parameter ------------------------------------------------------------------------------------------
// kind 0: out[n][t][c] = w[n][c][t].  Block (c chunk of RP_C channels, n): reads RP_C * taps consecutive floats, writes taps runs of RP_C bf16.
// kind 1: out[c][taps - 1 - t][n] = w[n][c][t] (the conv over dy that gives dx: channels and filters swapped, taps mirrored).  Block
//         (c chunk of RP_DC channels, n chunk of RP_DN filters): per filter RP_DC * taps consecutive floats in, per (c, t) a run of RP_DN bf16 out.
constexpr int RP_C = 256, RP_DC = 16, RP_DN = 64, RP_MAXT = 9;
__global__ __launch_bounds__(256) void repack_conv_fwd_kernel(const float* __restrict__ w, int C, int taps, bf16_t* __restrict__ out, int ldo) {
    __shared__ float tile[RP_C * RP_MAXT];
    const int n = blockIdx.y, c0 = blockIdx.x * RP_C, nc = min(RP_C, C - c0);
    const float* src = w + ((long long)n * C + c0) * taps;
    for (int i = threadIdx.x; i < nc * taps; i += 256) tile[i] = src[i];
    __syncthreads();
    bf16_t* dst = out + (long long)n * ldo + c0;
    for (int i = threadIdx.x; i < nc * taps; i += 256) {
        const int t = i / nc, c = i - t * nc;
        dst[(long long)t * C + c] = f2bf(tile[c * taps + t]);
    }
}
__global__ __launch_bounds__(256) void repack_conv_dgrad_kernel(const float* __restrict__ w, int N, int C, int taps, bf16_t* __restrict__ out, int ldo) {
    __shared__ float tile[RP_DN][RP_DC * RP_MAXT + 1];
    const int c0 = blockIdx.x * RP_DC, n0 = blockIdx.y * RP_DN, nc = min(RP_DC, C - c0), nn = min(RP_DN, N - n0);
    const int run = nc * taps;
    for (int i = threadIdx.x; i < nn * run; i += 256) {
        const int j = i / run, k = i - j * run;
        tile[j][k] = w[((long long)(n0 + j) * C + c0) * taps + k];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < run * nn; i += 256) {
        const int k = i / nn, j = i - k * nn;          // k = c * taps + t of the source
        const int c = k / taps, t = k - c * taps;
        out[(long long)(c0 + c) * ldo + (long long)(taps - 1 - t) * N + n0 + j] = f2bf(tile[j][k]);
    }
}

// ---- B-row linear family -----------------------------------------------------------------------------------------------------------------
constexpr int RL_MAXP = 24;         // problems per launch: the table is a kernel argument (24 x 112 bytes + the offsets below < 4 KB)
constexpr int RL_FWD_ROWS = 32;     // weight rows per forward workgroup (4 waves x 2 passes x 4 rows)
constexpr int RL_SPLIT_ROWS = 64;   // weight rows per workgroup of bwd_data (one N split) and wgrad
constexpr int RL_LDS_FLOATS = 16384;   // f(x) of one forward problem in LDS: B * K floats, 64 KB

struct RowlinTable {
    t2v_rowlin_problem p[RL_MAXP];
    long long ws_off[RL_MAXP];      // bwd_data: first float of the problem's partial sums [nsplit][B][K]
    int first[RL_MAXP + 1];         // block prefix sums
    int nsplit[RL_MAXP];            // bwd_data: N splits of RL_SPLIT_ROWS rows
    int lead[RL_MAXP];              // bwd_data: per distinct dx, the first problem that names it
    int n, B, ngroups;
};

// SiLU and its derivative in double, rounded once: the fp32 error budget of these entries is a few roundings per output (B = 1, N = 1)
__device__ __forceinline__ float rl_silu(float v) { return (float)((double)v / (1.0 + exp(-(double)v))); }
__device__ __forceinline__ float rl_dsilu(float v) {
    const double sg = 1.0 / (1.0 + exp(-(double)v));
    return (float)(sg * (1.0 + (double)v * (1.0 - sg)));
}

// elements [k0, k0 + VEC) of one weight row as floats (VEC = 4 fp32 / 8 bf16: 16 bytes); at or past K: 0, never read
template <int WB>
__device__ __forceinline__ void rl_load_w(const void* w, long long row_off, int k0, int K, bool vec, float* f) {
    if (WB) {
        const bf16_t* r = (const bf16_t*)w + row_off;
        if (vec && k0 + 8 <= K) { const uint4 v = *(const uint4*)(r + k0); unpack8(v, f); }
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = k0 + e < K ? bf2f(r[k0 + e]) : 0.f;
        }
    } else {
        const float* r = (const float*)w + row_off;
        if (vec && k0 + 4 <= K) { const float4 v = *(const float4*)(r + k0); f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = k0 + e < K ? r[k0 + e] : 0.f;
        }
    }
}

// y[b][n] = bias[n] + sum_k xs[b][k] W[n][k] (+ res[b][n]).  A wave owns four weight rows at a time: lane l holds the 16-byte chunks l, l + 64, ...
// of each (one pass over W), B accumulators per row, then one butterfly per (row, b).
template <int WB>
__device__ __forceinline__ void rl_fwd_body(const t2v_rowlin_problem& p, int B, int n_blk0, const float* xs) {
    constexpr int VEC = WB ? 8 : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = p.K, N = p.N, nch = (K + VEC - 1) / VEC;
    const bool wvec = (uintptr_t)p.w % 16 == 0 && p.ldw % VEC == 0;
    for (int pass = 0; pass < RL_FWD_ROWS / 16; ++pass) {
        const int n0 = n_blk0 + pass * 16 + wave * 4;
        if (n0 >= N) break;   // (wave-uniform)
        float acc[4][T2V_ROWLIN_MAX_ROWS];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b) acc[r][b] = 0.f;
        for (int c = lane; c < nch; c += 64) {
            const int k0 = c * VEC;
            float wv[4][VEC];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (n0 + r < N) rl_load_w<WB>(p.w, (long long)(n0 + r) * p.ldw, k0, K, wvec, wv[r]);
                else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) wv[r][e] = 0.f;
                }
            }
#pragma unroll
            for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b) {
                if (b < B) {
                    float xv[VEC];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) xv[e] = k0 + e < K ? xs[b * K + k0 + e] : 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) acc[r][b] += xv[e] * wv[r][e];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b) {
                if (b < B) {
                    float v = wave_sum(acc[r][b]) * p.alpha;
                    const int n = n0 + r;
                    if (lane == r * T2V_ROWLIN_MAX_ROWS + b && n < N) {
                        if (p.bias) v += p.bias[n];
                        if (p.res) v += p.res[(long long)b * p.ldr + n];
                        p.y[(long long)b * p.ldy + n] = v;
                    }
                }
            }
    }
}

__global__ __launch_bounds__(256) void rowlin_fwd_kernel(const RowlinTable t) {
    extern __shared__ float rl_xs[];   // f(x) [B][K] of this block's problem
    int i = 0;
    while (i + 1 < t.n && (int)blockIdx.x >= t.first[i + 1]) ++i;   // block-uniform
    const t2v_rowlin_problem& p = t.p[i];
    const int B = t.B, K = p.K;
    for (int j = threadIdx.x; j < B * K; j += 256) {
        const int b = j / K, k = j - b * K;
        const float v = p.x[(long long)b * p.ldx + k];
        rl_xs[j] = p.silu ? rl_silu(v) : v;
    }
    __syncthreads();
    const int n_blk0 = ((int)blockIdx.x - t.first[i]) * RL_FWD_ROWS;
    if (p.w_bf16) rl_fwd_body<1>(p, B, n_blk0, rl_xs);
    else rl_fwd_body<0>(p, B, n_blk0, rl_xs);
}

// Stage 1 of bwd_data: block (problem, N split, tile of 64 column chunks), one wave.  Lane l owns the 16-byte column chunk 64 tile + l of every
// weight row of the split (rows in order: a fixed sum), dy of the split's rows waits in LDS; partial[b][k] goes to the workspace.
template <int WB>
__device__ __forceinline__ void rl_bwd_body(const t2v_rowlin_problem& p, int B, int n0, int rows, int kt, float* part, const float (*sdy)[RL_SPLIT_ROWS]) {
    constexpr int VEC = WB ? 8 : 4;
    const int K = p.K, k0 = (kt * 64 + (int)threadIdx.x) * VEC;
    if (k0 >= K) return;
    const bool wvec = (uintptr_t)p.w % 16 == 0 && p.ldw % VEC == 0;
    float acc[T2V_ROWLIN_MAX_ROWS][VEC];
#pragma unroll
    for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[b][e] = 0.f;
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
        float wv[VEC];
        rl_load_w<WB>(p.w, (long long)(n0 + r) * p.ldw, k0, K, wvec, wv);
#pragma unroll
        for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b) {
            if (b < B) {
                const float d = sdy[b][r];
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[b][e] += d * wv[e];
            }
        }
    }
#pragma unroll
    for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b) {
        if (b < B) {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (k0 + e < K) part[(long long)b * K + k0 + e] = acc[b][e] * p.alpha;
        }
    }
}

__global__ __launch_bounds__(64) void rowlin_bwd_partial_kernel(const RowlinTable t, float* __restrict__ ws) {
    __shared__ float sdy[T2V_ROWLIN_MAX_ROWS][RL_SPLIT_ROWS];
    int i = 0;
    while (i + 1 < t.n && (int)blockIdx.x >= t.first[i + 1]) ++i;
    const t2v_rowlin_problem& p = t.p[i];
    const int B = t.B, VEC = p.w_bf16 ? 8 : 4;
    const int ktiles = ((p.K + VEC - 1) / VEC + 63) / 64;
    const int local = (int)blockIdx.x - t.first[i], split = local / ktiles, kt = local - split * ktiles;
    const int n0 = split * RL_SPLIT_ROWS, rows = min(RL_SPLIT_ROWS, p.N - n0);
    const int lane = threadIdx.x;
#pragma unroll
    for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b)
        if (b < B) sdy[b][lane] = lane < rows ? p.y[(long long)b * p.ldy + n0 + lane] : 0.f;
    __syncthreads();
    float* part = ws + t.ws_off[i] + (long long)split * B * p.K;
    if (p.w_bf16) rl_bwd_body<1>(p, B, n0, rows, kt, part, sdy);
    else rl_bwd_body<0>(p, B, n0, rows, kt, part, sdy);
}

// Stage 2: dx[b][k] (+)= g(pre[b][k]) * (sum of the partial sums of every problem that names this dx: problems in table order, their splits in
// order).  Block (256 values of [B][K], distinct dx).
__global__ __launch_bounds__(256) void rowlin_bwd_finish_kernel(const RowlinTable t, const float* __restrict__ ws) {
    const t2v_rowlin_problem& q = t.p[t.lead[blockIdx.y]];
    const int B = t.B, K = q.K;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * K) return;
    const int b = idx / K, k = idx - b * K;
    const long long slab = (long long)B * K;
    float s = 0.f;
    for (int i = 0; i < t.n; ++i) {
        if (t.p[i].dx != q.dx) continue;
        const float* src = ws + t.ws_off[i] + idx;
        const int ns = t.nsplit[i];
#pragma unroll 4
        for (int sp = 0; sp < ns; ++sp) s += src[sp * slab];
    }
    if (q.silu) s *= rl_dsilu(q.x[(long long)b * q.ldx + k]);
    float* d = q.dx + (long long)b * q.ldo + k;
    *d = q.accumulate ? *d + s : s;
}

// dW[n][k] (+)= alpha sum_b dy[b][n] f(x[b][k]), db[n] (+)= sum_b dy[b][n]: block (problem, RL_SPLIT_ROWS weight rows, tile of 64 four-column
// chunks), one wave.  Lane l keeps f(x[:, chunk]) in registers and streams its 16 bytes of every row out; the first column tile also writes db.
__global__ __launch_bounds__(64) void rowlin_wgrad_kernel(const RowlinTable t) {
    __shared__ float sdy[T2V_ROWLIN_MAX_ROWS][RL_SPLIT_ROWS];
    int i = 0;
    while (i + 1 < t.n && (int)blockIdx.x >= t.first[i + 1]) ++i;
    const t2v_rowlin_problem& p = t.p[i];
    const int B = t.B, K = p.K;
    const int ktiles = ((K + 3) / 4 + 63) / 64;
    const int local = (int)blockIdx.x - t.first[i], rblk = local / ktiles, kt = local - rblk * ktiles;
    const int n0 = rblk * RL_SPLIT_ROWS, rows = min(RL_SPLIT_ROWS, p.N - n0);
    const int lane = threadIdx.x;
#pragma unroll
    for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b)
        if (b < B) sdy[b][lane] = lane < rows ? p.y[(long long)b * p.ldy + n0 + lane] : 0.f;
    __syncthreads();
    if (kt == 0 && p.db && lane < rows) {
        float s = 0.f;
#pragma unroll
        for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b)
            if (b < B) s += sdy[b][lane];
        p.db[n0 + lane] = p.accumulate ? p.db[n0 + lane] + s : s;
    }
    const int k0 = (kt * 64 + lane) * 4;
    if (k0 >= K) return;
    const bool full = k0 + 4 <= K;
    const bool xvec = full && (uintptr_t)p.x % 16 == 0 && p.ldx % 4 == 0, ovec = full && (uintptr_t)p.dw % 16 == 0 && p.ldo % 4 == 0;
    float xv[T2V_ROWLIN_MAX_ROWS][4];
#pragma unroll
    for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b) {
        if (b < B) {
            const float* xr = p.x + (long long)b * p.ldx + k0;
            if (xvec) { const float4 v = *(const float4*)xr; xv[b][0] = v.x; xv[b][1] = v.y; xv[b][2] = v.z; xv[b][3] = v.w; }
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[b][e] = k0 + e < K ? xr[e] : 0.f;
            }
            if (p.silu) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k0 + e < K) xv[b][e] = rl_silu(xv[b][e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[b][e] = 0.f;
        }
    }
    const float alpha = p.alpha;
    const int acc = p.accumulate;
    for (int r = 0; r < rows; ++r) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < T2V_ROWLIN_MAX_ROWS; ++b) {
            if (b < B) {
                const float d = sdy[b][r];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += d * xv[b][e];
            }
        }
        float* dst = p.dw + (long long)(n0 + r) * p.ldo + k0;
        if (ovec) {
            float4 v = make_float4(o[0] * alpha, o[1] * alpha, o[2] * alpha, o[3] * alpha);
            if (acc) { const float4 old = *(const float4*)dst; v.x += old.x; v.y += old.y; v.z += old.z; v.w += old.w; }
            *(float4*)dst = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k0 + e < K) dst[e] = acc ? dst[e] + o[e] * alpha : o[e] * alpha;
        }
    }
}

// out[r][c] = keep(r, c) ? x[r][c] * inv_keep : 0 (+ resid[r][c]) on fp32 rows: the mask of t2v_dropout_bf16 (common.h: one splitmix64 word per quad
// of the row-major [rows][ncols] matrix, 16 bits per element), for the B-row LoRA branches of the conditioning leaves
__global__ __launch_bounds__(256) void dropout_f32_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ resid, int ldr, float* __restrict__ out,
                                                          int ldo, long long total, int ncols, uint32_t thr, float inv_keep, const uint64_t* __restrict__ seed_p,
                                                          uint32_t site) {
    const uint64_t key = dropout_key(*seed_p, site);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / ncols;
        const int c = (int)(i - r * ncols);
        const uint64_t w = dropout_quad(key, (uint64_t)(i >> 2));
        float v = dropout_keep16(w, (int)(i & 3), thr) ? x[r * ldx + c] * inv_keep : 0.f;
        if (resid) v += resid[r * ldr + c];
        out[r * ldo + c] = v;
    }
}

// cos || sin of t * exp(-ln(1e4) i / half) (guidance_style: sin || cos of 1000 t with the (half - 1) divisor), fp32 out: the arithmetic of
// elementwise.hip's bf16 entry without its last rounding
__global__ void timestep_embedding_f32_kernel(const void* t, int t_is_f32, int n, int dim, int guidance_style, float* out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int half = dim / 2;
    if (idx >= n * half) return;
    const int row = idx / half, i = idx % half;
    const float tv = t_is_f32 ? ((const float*)t)[row] : (float)((const long long*)t)[row];
    float c, s;
    if (guidance_style) {
        const float freq = expf((float)i * -(logf(10000.0f) / (float)(half - 1)));
        sincosf(tv * 1000.0f * freq, &s, &c);
        out[row * dim + i] = s;
        out[row * dim + half + i] = c;
    } else {
        const float freq = expf(-logf(10000.0f) * (float)i / (float)half);
        sincosf(tv * freq, &s, &c);
        out[row * dim + i] = c;
        out[row * dim + half + i] = s;
    }
    if ((dim & 1) && i == 0) out[row * dim + dim - 1] = 0.f;
}

}  // namespace

extern "C" long long t2v_im2col_rows(int mode, int n_img, int h, int w) {
    if (mode == T2V_GEMM_CONV3X3 || mode == T2V_GEMM_TCONV3) return (long long)n_img * h * w;
    if (mode == T2V_GEMM_CONV3X3_S2) return (long long)n_img * ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1);
    if (mode == T2V_GEMM_CONV3X3_S2_PAD01) return (long long)n_img * ((h - 2) / 2 + 1) * ((w - 2) / 2 + 1);
    if (mode == T2V_GEMM_CONV3X3_UP2) return (long long)n_img * 4 * h * w;
    return -1;
}

extern "C" int t2v_im2col_bf16(const void* x0, int c0, int ld0, const void* x1, int c1, int ld1, int mode, int n_img, int h, int w, int frames,
                               void* out, int ldo, void* stream) {
    T2V_REQUIRE(x0 && out && n_img > 0 && h > 0 && w > 0 && c0 > 0 && c1 >= 0 && (c1 == 0 || x1), T2V_EINVAL, "t2v_im2col_bf16: bad argument");
    const long long rows = t2v_im2col_rows(mode, n_img, h, w);
    T2V_REQUIRE(rows > 0, T2V_EINVAL, "t2v_im2col_bf16: mode must be one of the conv gather modes of t2v_gemm");
    const int taps = mode == T2V_GEMM_TCONV3 ? 3 : 9, C = c0 + c1;
    T2V_REQUIRE(c0 % 8 == 0 && c1 % 8 == 0 && ld0 % 8 == 0 && (c1 == 0 || ld1 % 8 == 0) && ldo % 8 == 0 && ldo >= taps * C &&
                    (uintptr_t)x0 % 16 == 0 && (uintptr_t)x1 % 16 == 0 && (uintptr_t)out % 16 == 0,
                T2V_ESHAPE, "t2v_im2col_bf16: channels / row strides in multiples of 8, 16-byte aligned rows, ldo >= taps * C");
    T2V_REQUIRE(ld0 >= c0 && (c1 == 0 || ld1 >= c1), T2V_ESHAPE, "t2v_im2col_bf16: row stride smaller than the part's channel count");
    T2V_REQUIRE(mode != T2V_GEMM_TCONV3 || (frames > 0 && n_img % frames == 0), T2V_ESHAPE, "t2v_im2col_bf16: n_img must be clips x frames");
    int ho = h, wo = w;
    if (mode == T2V_GEMM_CONV3X3_S2) { ho = (h - 1) / 2 + 1; wo = (w - 1) / 2 + 1; }
    else if (mode == T2V_GEMM_CONV3X3_S2_PAD01) { ho = (h - 2) / 2 + 1; wo = (w - 2) / 2 + 1; }
    else if (mode == T2V_GEMM_CONV3X3_UP2) { ho = 2 * h; wo = 2 * w; }
    const long long total = rows * taps * (C / 8);
    long long blocks = (total + 255) / 256;
    if (blocks > 256LL * 16) blocks = 256LL * 16;
    hipLaunchKernelGGL(im2col_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x0, c0, ld0, (const bf16_t*)x1, c1,
                       ld1, mode, n_img, h, w, ho, wo, frames, taps, (bf16_t*)out, ldo, total);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

static int affine_grad_blocks(long long sum_rows, long long n_out) {
    // about 1024 blocks over the whole launch, at least 16 rows (four per wave) each
    long long nblk = (1024 + n_out - 1) / n_out;
    const long long max_blk = (sum_rows + 15) / 16;
    if (nblk > max_blk) nblk = max_blk;
    if (nblk < 1) nblk = 1;
    return (int)nblk;
}

extern "C" long long t2v_norm_affine_grad_ws_floats(long long rows, long long sum_rows, int channels) {
    if (rows <= 0 || sum_rows <= 0 || rows % sum_rows || channels <= 0) return -1;
    const long long n_out = rows / sum_rows;
    return n_out * affine_grad_blocks(sum_rows, n_out) * 2 * channels;
}

extern "C" int t2v_norm_affine_grad(const void* x0, int c0, int ld0, const void* x1, int c1, int ld1, long long rows, long long sum_rows, int kind,
                                    int rows_per_unit, int groups, const float* stats, float ln_eps, const float* gamma, const float* beta,
                                    int silu, const void* dy, int ldy, float* dgamma, int ld_dgamma, float* dbeta, int ld_dbeta, float* ws,
                                    void* stream) {
    T2V_REQUIRE(dy && ws && rows > 0 && sum_rows > 0 && rows % sum_rows == 0 && kind >= 0 && kind <= 2 && (dgamma || dbeta), T2V_EINVAL,
                "t2v_norm_affine_grad: bad argument");
    if (kind == 2) {
        c1 = 0; x1 = nullptr; silu = 0;
        constexpr int CHUNK = 2048;
        if (c0 > CHUNK) {   // plain column sums are independent per column: wider matrices (the 8 C-wide GEGLU pre-activation) go out in chunks
            for (int c = 0; c < c0; c += CHUNK) {
                const int n = c0 - c < CHUNK ? c0 - c : CHUNK;
                const int rc = t2v_norm_affine_grad(nullptr, n, 0, nullptr, 0, 0, rows, sum_rows, 2, 0, 0, nullptr, 0.f, nullptr, nullptr, 0,
                                                    (const bf16_t*)dy + c, ldy, dgamma ? dgamma + c : nullptr, ld_dgamma, dbeta ? dbeta + c : nullptr,
                                                    ld_dbeta, ws, stream);
                if (rc != T2V_OK) return rc;
            }
            return T2V_OK;
        }
    }
    const int C = c0 + c1;
    T2V_REQUIRE(C > 0 && C % 8 == 0 && C <= 64 * 8 * AG_MAXJ && c0 % 8 == 0 && ldy % 8 == 0 && (uintptr_t)dy % 16 == 0, T2V_ESHAPE,
                "t2v_norm_affine_grad: channels a multiple of 8 (<= 2560 behind a norm), 16-byte aligned rows");
    if (kind != 2 && silu)
        T2V_REQUIRE(((uintptr_t)gamma | (uintptr_t)beta) % 16 == 0, T2V_ESHAPE, "t2v_norm_affine_grad: gamma / beta 16-byte aligned");
    if (kind != 2) {
        T2V_REQUIRE(x0 && ld0 % 8 == 0 && (uintptr_t)x0 % 16 == 0 && (c1 == 0 || (x1 && ld1 % 8 == 0 && (uintptr_t)x1 % 16 == 0)), T2V_ESHAPE,
                    "t2v_norm_affine_grad: the normalised tensor's rows must be 16-byte aligned");
        T2V_REQUIRE(!silu || (gamma && beta), T2V_EINVAL, "t2v_norm_affine_grad: SiLU behind the norm needs gamma and beta");
        T2V_REQUIRE(dgamma, T2V_EINVAL, "t2v_norm_affine_grad: dgamma");
    }
    if (kind == 0)
        T2V_REQUIRE(stats && groups > 0 && C % groups == 0 && rows_per_unit > 0 && rows % rows_per_unit == 0, T2V_ESHAPE,
                    "t2v_norm_affine_grad: GroupNorm statistics [rows / rows_per_unit][groups][2]");
    T2V_REQUIRE(ldy >= C && (kind == 2 || (ld0 >= c0 && (c1 == 0 || ld1 >= c1))) && (!dgamma || ld_dgamma >= C) && (!dbeta || ld_dbeta >= C),
                T2V_ESHAPE, "t2v_norm_affine_grad: row stride smaller than the channel count");
    const long long n_out = rows / sum_rows;
    T2V_REQUIRE(n_out <= 65535, T2V_ESHAPE, "t2v_norm_affine_grad: grid");
    const int nblk = affine_grad_blocks(sum_rows, n_out);
    const int rows_per_blk = (int)((sum_rows + nblk - 1) / nblk);
    hipStream_t s = (hipStream_t)stream;
    const size_t smem = (size_t)8 * C * sizeof(float);
    dim3 grid(nblk, (unsigned)n_out);
#define T2V_AG_LAUNCH(K, NJ, UR)                                                                                                              \
    do {                                                                                                                                      \
        static bool attr_set = false;   /* (8 C floats of LDS: 80 KB at 2560 channels, above the 64 KB a launch gets unasked) */             \
        if (!attr_set) { hipFuncSetAttribute((const void*)affine_grad_partial_kernel<K, NJ, UR>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); attr_set = true; } \
        hipLaunchKernelGGL((affine_grad_partial_kernel<K, NJ, UR>), grid, dim3(256), smem, s, (const bf16_t*)x0, c0, ld0, (const bf16_t*)x1, c1, ld1, sum_rows, \
                           rows_per_blk, rows_per_unit, groups, stats, ln_eps, gamma, beta, silu, (const bf16_t*)dy, ldy, ws);               \
    } while (0)
#define T2V_AG_BY_WIDTH(K)                                                                                                                    \
    do {                                                                                                                                      \
        if (C <= 512) T2V_AG_LAUNCH(K, 1, 4);                                                                                                 \
        else if (C <= 1024) T2V_AG_LAUNCH(K, 2, 2);                                                                                           \
        else if (C <= 1536) T2V_AG_LAUNCH(K, 3, 1);                                                                                           \
        else T2V_AG_LAUNCH(K, 5, 1);                                                                                                          \
    } while (0)
    if (kind == 0) T2V_AG_BY_WIDTH(0);
    else if (kind == 1) T2V_AG_BY_WIDTH(1);
    else T2V_AG_BY_WIDTH(2);
#undef T2V_AG_BY_WIDTH
#undef T2V_AG_LAUNCH
    T2V_CHECK_LAUNCH();
    hipLaunchKernelGGL(affine_grad_final_kernel, dim3((2 * C + 63) / 64, (unsigned)n_out), dim3(AGF_WAVES * 64), 0, s, (const float*)ws, nblk, C,
                       dgamma, ld_dgamma, dbeta, ld_dbeta);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

extern "C" int t2v_repack_conv_f32(const float* w, int N, int C, int taps, int kind, void* out, int ldo, void* stream) {
    T2V_REQUIRE(w && out && N > 0 && C > 0 && taps >= 1 && taps <= RP_MAXT && (kind == 0 || kind == 1), T2V_EINVAL,
                "t2v_repack_conv_f32: bad argument (taps <= 9, kind 0 = forward pack, 1 = data-gradient pack)");
    T2V_REQUIRE(ldo >= taps * (kind == 0 ? C : N), T2V_ESHAPE, "t2v_repack_conv_f32: ldo smaller than a pack row");
    hipStream_t s = (hipStream_t)stream;
    if (kind == 0) {
        T2V_REQUIRE(N <= 65535, T2V_ESHAPE, "t2v_repack_conv_f32: grid");
        hipLaunchKernelGGL(repack_conv_fwd_kernel, dim3((C + RP_C - 1) / RP_C, N), dim3(256), 0, s, w, C, taps, (bf16_t*)out, ldo);
    } else {
        T2V_REQUIRE((N + RP_DN - 1) / RP_DN <= 65535, T2V_ESHAPE, "t2v_repack_conv_f32: grid");
        hipLaunchKernelGGL(repack_conv_dgrad_kernel, dim3((C + RP_DC - 1) / RP_DC, (N + RP_DN - 1) / RP_DN), dim3(256), 0, s, w, N, C, taps,
                           (bf16_t*)out, ldo);
    }
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

// ---- B-row linear family: host side ------------------------------------------------------------------------------------------------------
enum { RL_FWD = 0, RL_BWD = 1, RL_WGRAD = 2 };

// every check of one entry over the WHOLE table, before anything is launched
static int rowlin_check(const t2v_rowlin_problem* p, int n, int B, int which) {
    T2V_REQUIRE(p && n >= 1, T2V_EINVAL, "t2v_rowlin: null or empty problem table");
    T2V_REQUIRE(B >= 1 && B <= T2V_ROWLIN_MAX_ROWS, T2V_EINVAL, "t2v_rowlin: 1 <= B <= T2V_ROWLIN_MAX_ROWS (8) rows");
    for (int i = 0; i < n; ++i) {
        const t2v_rowlin_problem& q = p[i];
        T2V_REQUIRE(q.K > 0 && q.N > 0 && q.y, T2V_EINVAL, "t2v_rowlin: bad problem (K, N > 0; y / dy must be given)");
        T2V_REQUIRE(q.ldy >= q.N, T2V_ESHAPE, "t2v_rowlin: ldy smaller than N");
        if (which == RL_FWD) {
            T2V_REQUIRE(q.x && q.w, T2V_EINVAL, "t2v_rowlin_fwd: null x or w");
            T2V_REQUIRE(q.ldx >= q.K && q.ldw >= q.K && (!q.res || q.ldr >= q.N), T2V_ESHAPE, "t2v_rowlin_fwd: row stride smaller than the row");
            T2V_REQUIRE((long long)B * q.K <= RL_LDS_FLOATS, T2V_ESHAPE, "t2v_rowlin_fwd: B * K <= 16384 (the input rows wait in LDS)");
        } else if (which == RL_BWD) {
            T2V_REQUIRE(q.w && q.dx && (!q.silu || q.x), T2V_EINVAL, "t2v_rowlin_bwd_data: null w or dx, or silu without the saved pre-activation");
            T2V_REQUIRE(q.ldw >= q.K && q.ldo >= q.K && (!q.silu || q.ldx >= q.K), T2V_ESHAPE, "t2v_rowlin_bwd_data: row stride smaller than the row");
            for (int j = 0; j < i; ++j)
                if (p[j].dx == q.dx)
                    T2V_REQUIRE(p[j].K == q.K && p[j].ldo == q.ldo && p[j].silu == q.silu && p[j].accumulate == q.accumulate &&
                                    (!q.silu || (p[j].x == q.x && p[j].ldx == q.ldx)),
                                T2V_EINVAL, "t2v_rowlin_bwd_data: problems that share dx must agree on K, ldo, g and accumulate");
        } else {
            T2V_REQUIRE(q.x && q.dw, T2V_EINVAL, "t2v_rowlin_wgrad: null x or dw");
            T2V_REQUIRE(q.ldx >= q.K && q.ldo >= q.K, T2V_ESHAPE, "t2v_rowlin_wgrad: row stride smaller than the row");
        }
    }
    return T2V_OK;
}

static int rowlin_splits(const t2v_rowlin_problem& q) { return (q.N + RL_SPLIT_ROWS - 1) / RL_SPLIT_ROWS; }

extern "C" long long t2v_rowlin_ws_floats(const t2v_rowlin_problem* problems, int n, int B) {
    if (!problems || n < 1 || B < 1 || B > T2V_ROWLIN_MAX_ROWS) return -1;
    long long most = 0;
    for (int c0 = 0; c0 < n; c0 += RL_MAXP) {   // (one launch pair per RL_MAXP problems: the workspace is reused from its start)
        long long need = 0;
        for (int i = c0; i < n && i < c0 + RL_MAXP; ++i) {
            if (problems[i].K <= 0 || problems[i].N <= 0) return -1;
            need += (long long)rowlin_splits(problems[i]) * B * problems[i].K;
        }
        if (need > most) most = need;
    }
    return most;
}

extern "C" int t2v_rowlin_fwd(const t2v_rowlin_problem* problems, int n, int B, void* stream) {
    const int rc = rowlin_check(problems, n, B, RL_FWD);
    if (rc != T2V_OK) return rc;
    for (int c0 = 0; c0 < n; c0 += RL_MAXP) {
        RowlinTable t = RowlinTable();
        t.n = n - c0 < RL_MAXP ? n - c0 : RL_MAXP; t.B = B; t.ngroups = 0;
        int blocks = 0, kmax = 0;
        for (int i = 0; i < t.n; ++i) {
            t.p[i] = problems[c0 + i];
            t.first[i] = blocks;
            blocks += (t.p[i].N + RL_FWD_ROWS - 1) / RL_FWD_ROWS;
            if (t.p[i].K > kmax) kmax = t.p[i].K;
        }
        t.first[t.n] = blocks;
        hipLaunchKernelGGL(rowlin_fwd_kernel, dim3((unsigned)blocks), dim3(256), (size_t)B * kmax * sizeof(float), (hipStream_t)stream, t);
        T2V_CHECK_LAUNCH();
    }
    return T2V_OK;
}

extern "C" int t2v_rowlin_bwd_data(const t2v_rowlin_problem* problems, int n, int B, float* ws, long long ws_floats, void* stream) {
    const int rc = rowlin_check(problems, n, B, RL_BWD);
    if (rc != T2V_OK) return rc;
    T2V_REQUIRE(ws && (uintptr_t)ws % 4 == 0, T2V_EINVAL, "t2v_rowlin_bwd_data: null workspace");
    T2V_REQUIRE(ws_floats >= t2v_rowlin_ws_floats(problems, n, B), T2V_ESHAPE, "t2v_rowlin_bwd_data: workspace smaller than t2v_rowlin_ws_floats");
    for (int c0 = 0; c0 < n; c0 += RL_MAXP) {
        RowlinTable t = RowlinTable();
        t.n = n - c0 < RL_MAXP ? n - c0 : RL_MAXP; t.B = B; t.ngroups = 0;
        int blocks = 0, kmax = 0;
        long long off = 0;
        for (int i = 0; i < t.n; ++i) {
            t2v_rowlin_problem& q = t.p[i];
            q = problems[c0 + i];
            for (int j = 0; j < c0; ++j)   // a dx an earlier launch pair of this call already wrote: its sums are added to, g(pre) distributes
                if (problems[j].dx == q.dx) q.accumulate = 1;
            const int vec = q.w_bf16 ? 8 : 4, ktiles = ((q.K + vec - 1) / vec + 63) / 64;
            t.nsplit[i] = rowlin_splits(q);
            t.ws_off[i] = off;
            t.first[i] = blocks;
            blocks += t.nsplit[i] * ktiles;
            off += (long long)t.nsplit[i] * B * q.K;
            bool seen = false;
            for (int j = 0; j < i; ++j) seen = seen || t.p[j].dx == q.dx;
            if (!seen) { t.lead[t.ngroups++] = i; if (q.K > kmax) kmax = q.K; }
        }
        t.first[t.n] = blocks;
        hipLaunchKernelGGL(rowlin_bwd_partial_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, t, ws);
        T2V_CHECK_LAUNCH();
        hipLaunchKernelGGL(rowlin_bwd_finish_kernel, dim3((unsigned)((B * kmax + 255) / 256), (unsigned)t.ngroups), dim3(256), 0, (hipStream_t)stream, t,
                           (const float*)ws);
        T2V_CHECK_LAUNCH();
    }
    return T2V_OK;
}

extern "C" int t2v_rowlin_wgrad(const t2v_rowlin_problem* problems, int n, int B, void* stream) {
    const int rc = rowlin_check(problems, n, B, RL_WGRAD);
    if (rc != T2V_OK) return rc;
    for (int c0 = 0; c0 < n; c0 += RL_MAXP) {
        RowlinTable t = RowlinTable();
        t.n = n - c0 < RL_MAXP ? n - c0 : RL_MAXP; t.B = B; t.ngroups = 0;
        int blocks = 0;
        for (int i = 0; i < t.n; ++i) {
            t.p[i] = problems[c0 + i];
            t.first[i] = blocks;
            blocks += rowlin_splits(t.p[i]) * (((t.p[i].K + 3) / 4 + 63) / 64);
        }
        t.first[t.n] = blocks;
        hipLaunchKernelGGL(rowlin_wgrad_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, t);
        T2V_CHECK_LAUNCH();
    }
    return T2V_OK;
}

extern "C" int t2v_timestep_embedding_f32(const void* t, int t_is_f32, int n, int dim, int guidance_style, float* out, void* stream) {
    T2V_REQUIRE(t && out && n > 0 && dim >= 4, T2V_EINVAL, "t2v_timestep_embedding_f32");
    const long long total = (long long)n * (dim / 2);
    hipLaunchKernelGGL(timestep_embedding_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, t_is_f32, n, dim,
                       guidance_style, out);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

extern "C" int t2v_dropout_f32(const float* x, int ldx, const float* resid, int ldr, float* out, int ldo, long long rows, int ncols, float p,
                               const void* seed, unsigned site, void* stream) {
    T2V_REQUIRE(x && out && seed && rows > 0 && ncols > 0, T2V_EINVAL, "t2v_dropout_f32: null pointer / empty");
    T2V_REQUIRE(p >= 0.f && p < 1.f - 1.f / 65536.f, T2V_EINVAL, "t2v_dropout_f32: p must be in [0, 1 - 2^-16)");
    T2V_REQUIRE(ncols % 2 == 0 && ldx >= ncols && ldo >= ncols && (!resid || ldr >= ncols), T2V_ESHAPE,
                "t2v_dropout_f32: even column count, row strides >= ncols");
    const double t = (double)p * 4294967296.0;
    const uint32_t thr = (t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t) >> 16;
    const float inv_keep = 65536.0f / (65536.0f - (float)thr);
    const long long total = rows * ncols;
    long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(dropout_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, resid, ldr, out, ldo, total, ncols, thr, inv_keep,
                       (const uint64_t*)seed, (uint32_t)site);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
