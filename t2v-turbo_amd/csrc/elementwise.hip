// Layout conversion, embeddings, small direct conv and the scheduler / consistency-distillation
// elementwise family for gfx950.  All bandwidth/latency bound; vectorised where the layout allows.
#include <math.h>
#include "common.h"

namespace {

__device__ __forceinline__ float load_as_f32(const void* p, int dt, long long i) {
    if (dt == T2V_F32) return ((const float*)p)[i];
    if (dt == T2V_BF16) return bf2f(((const bf16_t*)p)[i]);
    return (float)(((const _Float16*)p)[i]);
}
__device__ __forceinline__ void store_from_f32(void* p, int dt, long long i, float v) {
    if (dt == T2V_F32) ((float*)p)[i] = v;
    else if (dt == T2V_BF16) ((bf16_t*)p)[i] = f2bf(v);
    else ((_Float16*)p)[i] = (_Float16)v;
}

// (b,c,f,hw) -> rows ((b*f + fi)*hw + p), c columns.  One thread per (row): reads c strided
// planes (each coalesced across threads), writes c contiguous values.
__global__ void ncfhw_to_tokens_kernel(const void* x, int dt, int B, int C, int F, int HW, bf16_t* out, int ldo) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long M = (long long)B * F * HW;
    if (m >= M) return;
    const int p = (int)(m % HW);
    const long long bf = m / HW;
    const int f = (int)(bf % F);
    const long long b = bf / F;
    for (int c = 0; c < C; ++c)
        out[m * ldo + c] = f2bf(load_as_f32(x, dt, ((b * C + c) * F + f) * HW + p));
}
__global__ void tokens_to_ncfhw_kernel(const void* tok, int tok_f32, int ld, int B, int C, int F, int HW, void* out, int dt) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long M = (long long)B * F * HW;
    if (m >= M) return;
    const int p = (int)(m % HW);
    const long long bf = m / HW;
    const int f = (int)(bf % F);
    const long long b = bf / F;
    for (int c = 0; c < C; ++c) {
        const float v = tok_f32 ? ((const float*)tok)[m * ld + c] : bf2f(((const bf16_t*)tok)[m * ld + c]);
        store_from_f32(out, dt, ((b * C + c) * F + f) * HW + p, v);
    }
}

__global__ void timestep_embedding_kernel(const void* t, int t_is_f32, int n, int dim, int guidance_style, bf16_t* out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int half = dim / 2;
    if (idx >= n * half) return;
    const int row = idx / half, i = idx % half;
    float tv = t_is_f32 ? ((const float*)t)[row] : (float)((const long long*)t)[row];
    float c, s;
    if (guidance_style) {  // sin||cos of (w*1000) * exp(-i*ln(1e4)/(half-1))
        const float freq = expf((float)i * -(logf(10000.0f) / (float)(half - 1)));
        const float a = tv * 1000.0f * freq;
        sincosf(a, &s, &c);
        out[row * dim + i] = f2bf(s);
        out[row * dim + half + i] = f2bf(c);
    } else {  // cos||sin of t * exp(-ln(1e4) * i / half)
        const float freq = expf(-logf(10000.0f) * (float)i / (float)half);
        const float a = tv * freq;
        sincosf(a, &s, &c);
        out[row * dim + i] = f2bf(c);
        out[row * dim + half + i] = f2bf(s);
    }
    if ((dim & 1) && i == 0) out[row * dim + dim - 1] = 0;
}

__global__ void silu_kernel(const bf16_t* x, bf16_t* out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = f2bf(silu_f(bf2f(x[i])));
}
__global__ void cast_kernel(const void* x, int dt_in, void* out, int dt_out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) store_from_f32(out, dt_out, i, load_as_f32(x, dt_in, i));
}

struct Coef3 { float a[64], b[64], c[64]; };
__global__ void lincomb3_kernel(const float* x, const float* y, const float* z, Coef3 k, long long inner, long long total, float* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / inner);
    float v = k.a[b] * x[i];
    if (y) v += k.b[b] * y[i];
    if (z) v += k.c[b] * z[i];
    out[i] = v;
}
__global__ void lcm_step_kernel(const float* x, const void* eps, int eps_dt, const float* noise, float sa_t, float sb_t,
                                float c_skip, float c_out, float sa_p, float sb_p, long long n, float* prev, float* den) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float xv = x[i];
    const float e = load_as_f32(eps, eps_dt, i);
    const float x0 = (xv - sb_t * e) / sa_t;
    const float dn = c_out * x0 + c_skip * xv;
    den[i] = dn;
    prev[i] = noise ? sa_p * dn + sb_p * noise[i] : dn;
}

// direct 3x3 s1 p1 conv for cin <= 8: thread = (token, 8 output channels); weights fp32 in LDS, staged ONCE per block
// (a block walks its share of the tokens grid-stride: staging the 46 KiB of a 4 -> 320 conv for every 6 tokens was
// 9/10 of this kernel's time)
template <int CIN>
__global__ __launch_bounds__(256) void conv_small_kernel(const bf16_t* x, int n_img, int H, int W, const float* wgt,
                                                         const float* bias, int cout, bf16_t* out) {
    extern __shared__ float sw[];  // [9*CIN][cout + 4]: a thread reads its 8 output channels as two float4
    const int ldw = cout + 4;      // +4: the transposing writes below (consecutive k, same oc) spread over 16 banks, not 1
    for (int i = threadIdx.x; i < cout * 9 * CIN; i += 256) {
        const int oc = i / (9 * CIN), k = i - oc * 9 * CIN;
        sw[k * ldw + oc] = wgt[i];
    }
    __syncthreads();
    const int nch = cout / 8;
    const long long M = (long long)n_img * H * W;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < M * nch; e += (long long)gridDim.x * 256) {
    const long long m = e / nch;
    const int oc0 = (int)(e % nch) * 8;
    const int px = (int)(m % W), py = (int)((m / W) % H);
    const long long nbase = (m / ((long long)W * H)) * H * W;
    float acc[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = bias ? bias[oc0 + o] : 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = py + ky - 1, ix = px + kx - 1;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const bf16_t* xp = x + (nbase + (long long)iy * W + ix) * CIN;
            float xv[CIN];
            if constexpr (CIN == 4) {
                const uint2 u = *(const uint2*)xp;
                xv[0] = __uint_as_float(u.x << 16); xv[1] = __uint_as_float(u.x & 0xffff0000u);
                xv[2] = __uint_as_float(u.y << 16); xv[3] = __uint_as_float(u.y & 0xffff0000u);
            } else {
                unpack8(*(const uint4*)xp, xv);
            }
#pragma unroll
            for (int c = 0; c < CIN; ++c) {
                const float* wp = sw + ((ky * 3 + kx) * CIN + c) * ldw + oc0;
                const float4 w0 = *(const float4*)wp, w1 = *(const float4*)(wp + 4);
                acc[0] += xv[c] * w0.x; acc[1] += xv[c] * w0.y; acc[2] += xv[c] * w0.z; acc[3] += xv[c] * w0.w;
                acc[4] += xv[c] * w1.x; acc[5] += xv[c] * w1.y; acc[6] += xv[c] * w1.z; acc[7] += xv[c] * w1.w;
            }
        }
    *(uint4*)(out + m * cout + oc0) = pack8(acc);
    }
}

inline unsigned nblk(long long n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

extern "C" int t2v_ncfhw_to_tokens(const void* x, int dt, int b, int c, int f, int hw, void* out, int ldo, void* stream) {
    T2V_REQUIRE(x && out && b > 0 && c > 0 && f > 0 && hw > 0 && ldo >= c && dt >= 0 && dt <= 2, T2V_EINVAL, "t2v_ncfhw_to_tokens");
    hipLaunchKernelGGL(ncfhw_to_tokens_kernel, dim3(nblk((long long)b * f * hw)), dim3(256), 0, (hipStream_t)stream, x, dt, b,
                       c, f, hw, (bf16_t*)out, ldo);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_tokens_to_ncfhw(const void* tok, int tok_f32, int ld, int b, int c, int f, int hw, void* out, int dt,
                                   void* stream) {
    T2V_REQUIRE(tok && out && b > 0 && c > 0 && f > 0 && hw > 0 && ld >= c && dt >= 0 && dt <= 2, T2V_EINVAL, "t2v_tokens_to_ncfhw");
    hipLaunchKernelGGL(tokens_to_ncfhw_kernel, dim3(nblk((long long)b * f * hw)), dim3(256), 0, (hipStream_t)stream, tok,
                       tok_f32, ld, b, c, f, hw, out, dt);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_timestep_embedding(const void* t, int t_is_f32, int n, int dim, int guidance_style, void* out, void* stream) {
    T2V_REQUIRE(t && out && n > 0 && dim >= 4, T2V_EINVAL, "t2v_timestep_embedding");
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3(nblk((long long)n * (dim / 2))), dim3(256), 0, (hipStream_t)stream, t,
                       t_is_f32, n, dim, guidance_style, (bf16_t*)out);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_silu(const void* x, void* out, long long n, void* stream) {
    T2V_REQUIRE(x && out && n > 0, T2V_EINVAL, "t2v_silu");
    hipLaunchKernelGGL(silu_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)out, n);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
// Zero fill as a KERNEL (not hipMemsetAsync): every node of a captured launch list is then a kernel node, ordered like every
// other launch of the chain.  16-byte stores over the aligned body, byte stores for the (at most 15 + 15) edge bytes.
__global__ __launch_bounds__(256) void fill_zero_kernel(unsigned char* __restrict__ p, long long head, long long body16, long long nbytes) {
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    uint4* b = (uint4*)(p + head);
    for (long long i = i0; i < body16; i += step) b[i] = make_uint4(0, 0, 0, 0);
    const long long tail0 = head + body16 * 16;
    if (i0 < head) p[i0] = 0;
    if (i0 < nbytes - tail0) p[tail0 + i0] = 0;
}
extern "C" int t2v_fill_zero(void* p, long long nbytes, void* stream) {
    T2V_REQUIRE(p && nbytes > 0, T2V_EINVAL, "t2v_fill_zero");
    long long head = (16 - (long long)((uintptr_t)p & 15)) & 15;
    if (head > nbytes) head = nbytes;
    const long long body16 = (nbytes - head) / 16;
    long long blocks = (body16 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(fill_zero_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (unsigned char*)p, head, body16, nbytes);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_cast(const void* x, int dt_in, void* out, int dt_out, long long n, void* stream) {
    T2V_REQUIRE(x && out && n > 0 && dt_in >= 0 && dt_in <= 2 && dt_out >= 0 && dt_out <= 2, T2V_EINVAL, "t2v_cast");
    hipLaunchKernelGGL(cast_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, x, dt_in, out, dt_out, n);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_lincomb3(const float* x, const float* y, const float* z, const float* ca, const float* cb,
                            const float* cc, int nb, long long inner, float* out, void* stream) {
    T2V_REQUIRE(x && out && ca && nb > 0 && nb <= 64 && inner > 0, T2V_EINVAL, "t2v_lincomb3");
    T2V_REQUIRE((!y || cb) && (!z || cc), T2V_EINVAL, "t2v_lincomb3: missing coefficients");
    Coef3 k;
    for (int i = 0; i < nb; ++i) { k.a[i] = ca[i]; k.b[i] = cb ? cb[i] : 0.f; k.c[i] = cc ? cc[i] : 0.f; }
    hipLaunchKernelGGL(lincomb3_kernel, dim3(nblk(inner * nb)), dim3(256), 0, (hipStream_t)stream, x, y, z, k, inner,
                       inner * nb, out);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_lcm_step(const float* x, const void* eps, int eps_dt, const float* noise, float sa_t, float sb_t,
                            float c_skip, float c_out, float sa_p, float sb_p, long long n, float* prev, float* denoised,
                            void* stream) {
    T2V_REQUIRE(x && eps && prev && denoised && n > 0 && sa_t != 0.f, T2V_EINVAL, "t2v_lcm_step");
    hipLaunchKernelGGL(lcm_step_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, x, eps, eps_dt, noise, sa_t, sb_t,
                       c_skip, c_out, sa_p, sb_p, n, prev, denoised);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

extern "C" int t2v_conv3x3_small_cin(const void* x, int n_img, int h, int w, int cin, const float* wgt, const float* bias,
                                     int cout, void* out, void* stream) {
    T2V_REQUIRE(x && wgt && out && n_img > 0 && h > 0 && w > 0, T2V_EINVAL, "t2v_conv3x3_small_cin");
    T2V_REQUIRE((cin == 4 || cin == 8) && cout % 8 == 0 && (cout + 4) * 9 * cin * 4 <= 150 * 1024, T2V_ESHAPE,
                "t2v_conv3x3_small_cin: cin must be 4 or 8, cout a multiple of 8");
    const long long work = (long long)n_img * h * w * (cout / 8);
    const int smem = (cout + 4) * 9 * cin * 4;
    // as many blocks as stay resident at once (LDS-limited), at least 8 tokens' worth of work each
    const int per_cu = smem > 0 ? (160 * 1024) / smem : 1;
    long long blocks = 256LL * (per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu));
    if (blocks > (work + 255) / 256) blocks = (work + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
    if (cin == 4) {
        static bool set4 = false;
        if (!set4) { hipFuncSetAttribute((const void*)conv_small_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); set4 = true; }
        hipLaunchKernelGGL(conv_small_kernel<4>, dim3((unsigned)blocks), dim3(256), smem, s, (const bf16_t*)x, n_img, h, w, wgt, bias, cout, (bf16_t*)out);
    } else {
        static bool set8 = false;
        if (!set8) { hipFuncSetAttribute((const void*)conv_small_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); set8 = true; }
        hipLaunchKernelGGL(conv_small_kernel<8>, dim3((unsigned)blocks), dim3(256), smem, s, (const bf16_t*)x, n_img, h, w, wgt, bias, cout, (bf16_t*)out);
    }
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

// ---- optimizer / EMA over flat buffers ---------------------------------------------------------------
namespace {
__global__ void adamw_kernel(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2,
                             float eps, float wd, float bc1, float bc2_sqrt, float gscale) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        float4 pp = *(float4*)(p + i), gg = *(const float4*)(g + i), mm = *(float4*)(m + i), vv = *(float4*)(v + i);
        float* P = (float*)&pp; float* G = (float*)&gg; float* M = (float*)&mm; float* V = (float*)&vv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gr = G[e] * gscale;
            P[e] *= 1.0f - lr * wd;
            M[e] = b1 * M[e] + (1.0f - b1) * gr;
            V[e] = b2 * V[e] + (1.0f - b2) * gr * gr;
            P[e] -= (lr / bc1) * M[e] / (sqrtf(V[e]) / bc2_sqrt + eps);
        }
        *(float4*)(p + i) = pp; *(float4*)(m + i) = mm; *(float4*)(v + i) = vv;
    } else {
        for (long long j = i; j < n; ++j) {
            const float gr = g[j] * gscale;
            float pj = p[j] * (1.0f - lr * wd);
            const float mj = b1 * m[j] + (1.0f - b1) * gr, vj = b2 * v[j] + (1.0f - b2) * gr * gr;
            pj -= (lr / bc1) * mj / (sqrtf(vj) / bc2_sqrt + eps);
            p[j] = pj; m[j] = mj; v[j] = vj;
        }
    }
}
__global__ void ema_kernel(float* t, const float* s, float rate, long long n) {
#pragma clang fp contract(off)   // (two products and a sum, as this kernel has always been compiled: ema_multi_kernel must give the same bits)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t[i] = t[i] * rate + s[i] * (1.0f - rate);
}
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* x, long long n, float* ws) {
    __shared__ float sh[4];
    float a = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) a += x[i] * x[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* ws, int nblk, float* out) {
    __shared__ double sh[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) a += (double)ws[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)sh[0];
}
}  // namespace

extern "C" int t2v_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                              void* stream) {
    T2V_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && step >= 1, T2V_EINVAL, "t2v_adamw_step");
    T2V_REQUIRE(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0, T2V_ESHAPE,
                "t2v_adamw_step: buffers must be 16-byte aligned");
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adamw_kernel, dim3(nblk((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2), grad_scale);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_ema_update(float* target, const float* src, float rate, long long n, void* stream) {
    T2V_REQUIRE(target && src && n > 0, T2V_EINVAL, "t2v_ema_update");
    hipLaunchKernelGGL(ema_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, target, src, rate, n);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_sumsq(const float* x, long long n, float* ws, float* out, void* stream) {
    T2V_REQUIRE(x && ws && out && n > 0, T2V_EINVAL, "t2v_sumsq");
    const int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, n, ws);
    T2V_CHECK_LAUNCH();
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, blocks, out);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

// ---- block-wise 8-bit AdamW (optim.AdamW8bit) ----------------------------------------------------------
// One WAVE per quantisation block of 256 elements, 4 per lane: a 16-byte load each of the parameter and the gradient, one dword each
// of the two code arrays.  Both code books and the midpoints between neighbouring codes live in LDS (4 KiB, loaded once per
// workgroup: the grid is persistent); the nearest code of a value is the number of midpoints below it, an 8-step binary search.
// The two absmax reductions are wave shuffles: no workgroup barrier inside the loop.  Bandwidth: 16 B per element (fp32 moments: 28).
// Floating-point contraction is OFF in these kernels: the moments decide the stored absmax and codes, which optim.py's CPU
// restatement (separately rounded multiplies and adds) reproduces bit for bit only without fused multiply-adds.
namespace {
struct Book8 {
    float code[256];
    float mid[256];   // mid[i] = (code[i] + code[i + 1]) / 2, i < 255
};
__device__ __forceinline__ void book8_load(Book8& b, const float* code, int tid) {   // 256 threads
    const float c = code[tid];
    b.code[tid] = c;
    b.mid[tid] = tid < 255 ? 0.5f * (c + code[tid + 1]) : 3.0e38f;
}
__device__ __forceinline__ unsigned book8_nearest(const Book8& b, float x) {   // NaN -> 0; always in [0, 255]
    unsigned idx = 0;
#pragma unroll
    for (unsigned s = 128; s > 0; s >>= 1) idx += (b.mid[idx + s - 1] < x) ? s : 0u;
    return idx;
}
__device__ __forceinline__ uint32_t book8_quant4(const Book8& b, const float* v, float absmax) {
#pragma clang fp contract(off)
    uint32_t q = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) q |= book8_nearest(b, absmax > 0.f ? v[j] / absmax : 0.f) << (8 * j);
    return q;
}
// the 4 elements of this lane: how many are inside the tensor, and whether they can move as one 16-byte access
__device__ __forceinline__ int lane_count4(long long n, long long e0) {
    const long long rem = n - e0;
    return rem >= 4 ? 4 : rem > 0 ? (int)rem : 0;
}
__device__ __forceinline__ void load4(const float* base, long long e0, int k, bool vec, float* out) {
    if (k == 4 && vec) {
        const float4 t = *(const float4*)(base + e0);
        out[0] = t.x; out[1] = t.y; out[2] = t.z; out[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = j < k ? base[e0 + j] : 0.f;
    }
}
__device__ __forceinline__ void store4(float* base, long long e0, int k, bool vec, const float* v) {
    if (k == 4 && vec) {
        *(float4*)(base + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < k) base[e0 + j] = v[j];
    }
}

__global__ __launch_bounds__(256) void adamw8_kernel(const t2v_adamw8_tensor* table, int nt, long long nblocks, uint32_t* s1,
                                                     uint32_t* s2, float* am1, float* am2, float* f1, float* f2,
                                                     const float* code1, const float* code2, float b1, float b2, float eps,
                                                     float bc1, float bc2_sqrt, float gscale) {
#pragma clang fp contract(off)
    __shared__ Book8 book[2];
    book8_load(book[0], code1, threadIdx.x);
    book8_load(book[1], code2, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (long long blk = (long long)blockIdx.x * 4 + wave; blk < nblocks; blk += (long long)gridDim.x * 4) {
        int lo = 0, hi = nt - 1;   // the tensor that owns this work block: the last one with work0 <= blk (wave-uniform)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[mid].work0 <= blk) lo = mid; else hi = mid - 1;
        }
        const t2v_adamw8_tensor d = table[lo];
        const long long local = blk - d.work0;
        const long long e0 = local * T2V_ADAMW8_BLOCK + lane * 4;
        const int k = lane_count4(d.n, e0);   // 0 for the padding lanes of a last, partial block: they touch no parameter data
        const bool vec = (((uintptr_t)d.param | (uintptr_t)d.grad) & 15) == 0;
        const long long sb = d.state_block + local;
        const bool f32_state = (d.flags & T2V_ADAMW8_F32_STATE) != 0;
        float P[4], G[4], M[4], V[4];
        load4(d.param, e0, k, vec, P);
        load4(d.grad, e0, k, vec, G);
        if (f32_state) {
            load4(f1, sb * T2V_ADAMW8_BLOCK + lane * 4, 4, true, M);
            load4(f2, sb * T2V_ADAMW8_BLOCK + lane * 4, 4, true, V);
        } else {
            const uint32_t c1 = s1[sb * 64 + lane], c2 = s2[sb * 64 + lane];
            const float a1 = am1[sb], a2 = am2[sb];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                M[j] = book[0].code[(c1 >> (8 * j)) & 255u] * a1;
                V[j] = book[1].code[(c2 >> (8 * j)) & 255u] * a2;
            }
        }
        const float decay = 1.0f - d.lr * d.weight_decay, step_size = d.lr / bc1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < k) {   // t2v_adamw_step's order of operations
                const float gr = G[j] * gscale;
                P[j] *= decay;
                M[j] = b1 * M[j] + (1.0f - b1) * gr;
                V[j] = b2 * V[j] + (1.0f - b2) * gr * gr;
                P[j] -= step_size * M[j] / (sqrtf(V[j]) / bc2_sqrt + eps);
            } else {
                M[j] = 0.f; V[j] = 0.f;
            }
        }
        store4(d.param, e0, k, vec, P);   // from the fresh fp32 moments, not the re-quantised ones
        if (f32_state) {
            store4(f1, sb * T2V_ADAMW8_BLOCK + lane * 4, 4, true, M);
            store4(f2, sb * T2V_ADAMW8_BLOCK + lane * 4, 4, true, V);
        } else {
            const float mx1 = wave_max(fmaxf(fmaxf(fabsf(M[0]), fabsf(M[1])), fmaxf(fabsf(M[2]), fabsf(M[3]))));
            const float mx2 = wave_max(fmaxf(fmaxf(fabsf(V[0]), fabsf(V[1])), fmaxf(fabsf(V[2]), fabsf(V[3]))));
            s1[sb * 64 + lane] = book8_quant4(book[0], M, mx1);
            s2[sb * 64 + lane] = book8_quant4(book[1], V, mx2);
            if (lane == 0) { am1[sb] = mx1; am2[sb] = mx2; }
        }
    }
}
__global__ __launch_bounds__(256) void quant8_kernel(const float* x, long long n, long long nblocks, const float* code, uint32_t* codes,
                                                     float* absmax) {
    __shared__ Book8 book;
    book8_load(book, code, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool vec = ((uintptr_t)x & 15) == 0;
    for (long long blk = (long long)blockIdx.x * 4 + wave; blk < nblocks; blk += (long long)gridDim.x * 4) {
        const long long e0 = blk * T2V_ADAMW8_BLOCK + lane * 4;
        float X[4];
        load4(x, e0, lane_count4(n, e0), vec, X);   // padding lanes: 0
        const float mx = wave_max(fmaxf(fmaxf(fabsf(X[0]), fabsf(X[1])), fmaxf(fabsf(X[2]), fabsf(X[3]))));
        codes[blk * 64 + lane] = book8_quant4(book, X, mx);
        if (lane == 0) absmax[blk] = mx;
    }
}
__global__ __launch_bounds__(256) void dequant8_kernel(const uint32_t* codes, const float* absmax, const float* code, float* out,
                                                       long long n, long long nblocks) {
    __shared__ Book8 book;
    book8_load(book, code, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool vec = ((uintptr_t)out & 15) == 0;
    for (long long blk = (long long)blockIdx.x * 4 + wave; blk < nblocks; blk += (long long)gridDim.x * 4) {
        const long long e0 = blk * T2V_ADAMW8_BLOCK + lane * 4;
        const uint32_t c = codes[blk * 64 + lane];
        const float a = absmax[blk];
        float X[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) X[j] = book.code[(c >> (8 * j)) & 255u] * a;
        store4(out, e0, lane_count4(n, e0), vec, X);
    }
}
// persistent grid: 8 workgroups of 4 waves per CU of a 256-CU part fill every wave slot; fewer when there is less work
inline unsigned blocks8(long long nblocks) { return (unsigned)((nblocks + 3) / 4 < 2048 ? (nblocks + 3) / 4 : 2048); }
}  // namespace

extern "C" int t2v_adamw8_step(const t2v_adamw8_tensor* table, int n_tensors, long long n_blocks, unsigned char* state1,
                               unsigned char* state2, float* absmax1, float* absmax2, float* state1_f32, float* state2_f32,
                               const float* code1, const float* code2, float beta1, float beta2, float eps, int step,
                               float grad_scale, void* stream) {
    T2V_REQUIRE(table && code1 && code2 && n_tensors > 0 && n_blocks >= n_tensors && step >= 1, T2V_EINVAL, "t2v_adamw8_step");
    T2V_REQUIRE((state1 && state2 && absmax1 && absmax2) || (state1_f32 && state2_f32), T2V_EINVAL, "t2v_adamw8_step: no state arena");
    T2V_REQUIRE(!state1 == !state2 && !state1 == !absmax1 && !state1 == !absmax2 && !state1_f32 == !state2_f32, T2V_EINVAL,
                "t2v_adamw8_step: an arena is given for one moment only");
    T2V_REQUIRE(((uintptr_t)state1 | (uintptr_t)state2 | (uintptr_t)state1_f32 | (uintptr_t)state2_f32) % 16 == 0 && (uintptr_t)table % 8 == 0,
                T2V_ESHAPE, "t2v_adamw8_step: the state arenas must be 16-byte aligned (the table 8-byte)");
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adamw8_kernel, dim3(blocks8(n_blocks)), dim3(256), 0, (hipStream_t)stream, table, n_tensors, n_blocks,
                       (uint32_t*)state1, (uint32_t*)state2, absmax1, absmax2, state1_f32, state2_f32, code1, code2, beta1, beta2,
                       eps, bc1, sqrtf(bc2), grad_scale);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_quant8_blockwise(const float* x, long long n, const float* code, unsigned char* codes, float* absmax,
                                    void* stream) {
    T2V_REQUIRE(x && code && codes && absmax && n > 0, T2V_EINVAL, "t2v_quant8_blockwise");
    T2V_REQUIRE((uintptr_t)codes % 4 == 0, T2V_ESHAPE, "t2v_quant8_blockwise: codes must be 4-byte aligned");
    const long long nblocks = (n + T2V_ADAMW8_BLOCK - 1) / T2V_ADAMW8_BLOCK;
    hipLaunchKernelGGL(quant8_kernel, dim3(blocks8(nblocks)), dim3(256), 0, (hipStream_t)stream, x, n, nblocks, code,
                       (uint32_t*)codes, absmax);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_dequant8_blockwise(const unsigned char* codes, const float* absmax, const float* code, float* out, long long n,
                                      void* stream) {
    T2V_REQUIRE(codes && absmax && code && out && n > 0, T2V_EINVAL, "t2v_dequant8_blockwise");
    T2V_REQUIRE((uintptr_t)codes % 4 == 0, T2V_ESHAPE, "t2v_dequant8_blockwise: codes must be 4-byte aligned");
    const long long nblocks = (n + T2V_ADAMW8_BLOCK - 1) / T2V_ADAMW8_BLOCK;
    hipLaunchKernelGGL(dequant8_kernel, dim3(blocks8(nblocks)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)codes, absmax,
                       code, out, n, nblocks);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

// ---- EMA of MANY tensors in one launch (optim.update_ema) -----------------------------------------------
// One workgroup per work block of T2V_EMA_BLOCK elements of ONE tensor, found by binary search over work0 (wave-uniform: scalar
// loads of a table that stays in cache).  A lane keeps T2V_EMA_BLOCK / 256 = 16 elements: four 16-byte loads of the target and four
// (fp32) or two (bf16) of the source are issued before the first result is needed.  Pure stream: no LDS, no atomics.  The element
// expression is ema_kernel's, written the same way and like it without floating-point contraction (two rounded products and a
// rounded sum), so that both give the same bits.
namespace {
__device__ __forceinline__ float4 ema4(float4 t, const float* s, float rate) {
#pragma clang fp contract(off)
    t.x = t.x * rate + s[0] * (1.0f - rate);
    t.y = t.y * rate + s[1] * (1.0f - rate);
    t.z = t.z * rate + s[2] * (1.0f - rate);
    t.w = t.w * rate + s[3] * (1.0f - rate);
    return t;
}
__global__ __launch_bounds__(256) void ema_multi_kernel(const t2v_ema_tensor* __restrict__ table, int nt, long long nblocks, float rate) {
#pragma clang fp contract(off)
    constexpr int Q = T2V_EMA_BLOCK / (256 * 4);   // 4-element groups per lane and work block
    static_assert(Q >= 2 && Q % 2 == 0 && Q * 256 * 4 == T2V_EMA_BLOCK, "T2V_EMA_BLOCK: an even number of float4 per lane");
    const int tid = threadIdx.x;
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        int lo = 0, hi = nt - 1;   // the tensor that owns this work block: the last one with work0 <= blk
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[mid].work0 <= blk) lo = mid; else hi = mid - 1;
        }
        const t2v_ema_tensor d = table[lo];
        const long long e0 = (blk - d.work0) * T2V_EMA_BLOCK;
        if (e0 < 0 || e0 >= d.n) continue;   // a work block no tensor owns (a gap in work0): nothing is touched
        const long long left = d.n - e0;
        const int cnt = left < T2V_EMA_BLOCK ? (int)left : T2V_EMA_BLOCK;   // elements of this work block; every index below is < cnt
        float* t = d.target + e0;
        const bool bf = d.src_dt == T2V_BF16;
        if ((((uintptr_t)d.target | (uintptr_t)d.src) & 15) != 0) {   // a 4-byte-aligned view: scalar accesses
            if (bf) {
                const bf16_t* s = (const bf16_t*)d.src + e0;
#pragma unroll 1
                for (int i = tid; i < cnt; i += 256) t[i] = t[i] * rate + bf2f(s[i]) * (1.0f - rate);
            } else {
                const float* s = (const float*)d.src + e0;
#pragma unroll 1
                for (int i = tid; i < cnt; i += 256) t[i] = t[i] * rate + s[i] * (1.0f - rate);
            }
        } else if (bf) {   // (work blocks start at multiples of 4096 elements: t + e0 and s + e0 keep the 16-byte alignment)
            const bf16_t* s = (const bf16_t*)d.src + e0;
            float4 T[Q];
            uint4 S[Q / 2];
#pragma unroll
            for (int j = 0; j < Q / 2; ++j) {
                const int i = (j * 256 + tid) * 8;
                if (i + 8 <= cnt) {
                    T[2 * j] = *(const float4*)(t + i);
                    T[2 * j + 1] = *(const float4*)(t + i + 4);
                    S[j] = *(const uint4*)(s + i);
                }
            }
#pragma unroll
            for (int j = 0; j < Q / 2; ++j) {
                const int i = (j * 256 + tid) * 8;
                if (i + 8 <= cnt) {
                    float f[8];
                    unpack8(S[j], f);
                    *(float4*)(t + i) = ema4(T[2 * j], f, rate);
                    *(float4*)(t + i + 4) = ema4(T[2 * j + 1], f + 4, rate);
                } else {
#pragma unroll 1
                    for (int k = i; k < cnt; ++k) t[k] = t[k] * rate + bf2f(s[k]) * (1.0f - rate);
                }
            }
        } else {
            const float* s = (const float*)d.src + e0;
            float4 T[Q], S[Q];
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                const int i = (j * 256 + tid) * 4;
                if (i + 4 <= cnt) {
                    T[j] = *(const float4*)(t + i);
                    S[j] = *(const float4*)(s + i);
                }
            }
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                const int i = (j * 256 + tid) * 4;
                if (i + 4 <= cnt) {
                    *(float4*)(t + i) = ema4(T[j], (const float*)&S[j], rate);
                } else {
#pragma unroll 1
                    for (int k = i; k < cnt; ++k) t[k] = t[k] * rate + s[k] * (1.0f - rate);
                }
            }
        }
    }
}
}  // namespace

extern "C" int t2v_ema_multi(const t2v_ema_tensor* table, int n_tensors, long long n_blocks, float rate, void* stream) {
    T2V_REQUIRE(table && n_tensors > 0 && n_blocks > 0, T2V_EINVAL, "t2v_ema_multi");
    T2V_REQUIRE((uintptr_t)table % 8 == 0, T2V_ESHAPE, "t2v_ema_multi: the table must be 8-byte aligned");
    // grid-stride over the work blocks: up to 32 workgroups per CU of a 256-CU part, four rounds of the 8 that are resident at once
    const unsigned grid = (unsigned)(n_blocks < 8192 ? n_blocks : 8192);
    hipLaunchKernelGGL(ema_multi_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, table, n_tensors, n_blocks, rate);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

// ---- fp32 AdamW, gradient norm and gradient scaling of MANY tensors where they are (optim.AdamW, optim.clip_grad_norm_) ----
// One workgroup per work block of T2V_ADAMW_BLOCK elements of ONE tensor (binary search over work0, as above); persistent grid.  A
// lane keeps T2V_ADAMW_BLOCK / 256 = 16 elements of each of the four arrays: all sixteen 16-byte loads are issued before the first
// result is needed.  Pure stream, 28 B per element: no LDS, no atomics.  The element expression is the fp32-state branch of
// adamw8_kernel, written the same way and like it without floating-point contraction: on one build both give the same bits.
namespace {
struct AdamwRows {   // the hyper rows of one launch, by value in the kernel arguments: a moving lr costs no upload
    float lr[T2V_ADAMW_MAX_HYPER], wd[T2V_ADAMW_MAX_HYPER], b1[T2V_ADAMW_MAX_HYPER], b2[T2V_ADAMW_MAX_HYPER], eps[T2V_ADAMW_MAX_HYPER],
        bc1[T2V_ADAMW_MAX_HYPER], bc2_sqrt[T2V_ADAMW_MAX_HYPER];
};
struct AdamwK { float scale, decay, b1, b2, step_size, bc2_sqrt, eps; };
__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const AdamwK& k) {
#pragma clang fp contract(off)
    const float gr = g * k.scale;   // t2v_adamw_step's order of operations
    p *= k.decay;
    m = k.b1 * m + (1.0f - k.b1) * gr;
    v = k.b2 * v + (1.0f - k.b2) * gr * gr;
    p -= k.step_size * m / (sqrtf(v) / k.bc2_sqrt + k.eps);
}
// the tensor that owns work block `blk`: the last one with work0 <= blk
template <class T>
__device__ __forceinline__ int owner_of(const T* table, int nt, long long blk) {
    int lo = 0, hi = nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].work0 <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__global__ __launch_bounds__(256) void adamw_multi_kernel(const t2v_adamw_tensor* __restrict__ table, int nt, long long nblocks,
                                                          AdamwRows rows, int n_rows, float gscale, const float* gscale_dev) {
#pragma clang fp contract(off)
    constexpr int Q = T2V_ADAMW_BLOCK / (256 * 4);   // 4-element groups per lane and work block
    static_assert(Q >= 1 && Q * 256 * 4 == T2V_ADAMW_BLOCK, "T2V_ADAMW_BLOCK: whole float4 per lane");
    const int tid = threadIdx.x;
    const float scale = gscale * (gscale_dev ? *gscale_dev : 1.0f);
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const t2v_adamw_tensor d = table[owner_of(table, nt, blk)];
        const long long e0 = (blk - d.work0) * T2V_ADAMW_BLOCK;
        if (e0 < 0 || e0 >= d.n || d.hyper < 0 || d.hyper >= n_rows) continue;   // a work block no tensor owns: nothing is touched
        const long long left = d.n - e0;
        const int cnt = left < T2V_ADAMW_BLOCK ? (int)left : T2V_ADAMW_BLOCK;   // elements of this work block; every index below is < cnt
        const int h = d.hyper;
        AdamwK k;
        k.scale = scale;
        k.decay = 1.0f - rows.lr[h] * rows.wd[h];
        k.b1 = rows.b1[h]; k.b2 = rows.b2[h];
        k.step_size = rows.lr[h] / rows.bc1[h];
        k.bc2_sqrt = rows.bc2_sqrt[h]; k.eps = rows.eps[h];
        float* p = d.param + e0;
        const float* g = d.grad + e0;
        float* m = d.exp_avg + e0;
        float* v = d.exp_avg_sq + e0;
        if ((((uintptr_t)d.param | (uintptr_t)d.grad | (uintptr_t)d.exp_avg | (uintptr_t)d.exp_avg_sq) & 15) != 0) {
#pragma unroll 1
            for (int i = tid; i < cnt; i += 256) {   // a 4-byte-aligned view: scalar accesses
                float pi = p[i], mi = m[i], vi = v[i];
                adamw1(pi, g[i], mi, vi, k);
                p[i] = pi; m[i] = mi; v[i] = vi;
            }
            continue;
        }
        // (work blocks start at multiples of 4096 elements: the four pointers keep their 16-byte alignment)
        float4 P[Q], G[Q], M[Q], V[Q];
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const int i = (j * 256 + tid) * 4;
            if (i + 4 <= cnt) {
                P[j] = *(const float4*)(p + i);
                G[j] = *(const float4*)(g + i);
                M[j] = *(const float4*)(m + i);
                V[j] = *(const float4*)(v + i);
            }
        }
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const int i = (j * 256 + tid) * 4;
            if (i + 4 <= cnt) {
                adamw1(P[j].x, G[j].x, M[j].x, V[j].x, k);
                adamw1(P[j].y, G[j].y, M[j].y, V[j].y, k);
                adamw1(P[j].z, G[j].z, M[j].z, V[j].z, k);
                adamw1(P[j].w, G[j].w, M[j].w, V[j].w, k);
                *(float4*)(p + i) = P[j];
                *(float4*)(m + i) = M[j];
                *(float4*)(v + i) = V[j];
            } else {
#pragma unroll 1
                for (int e = i; e < cnt; ++e) {   // the (at most 3) elements past the last whole float4
                    float pe = p[e], me = m[e], ve = v[e];
                    adamw1(pe, g[e], me, ve, k);
                    p[e] = pe; m[e] = me; v[e] = ve;
                }
            }
        }
    }
}
// ws[blk] = sum of squares of the gradient elements of work block blk.  A lane adds its 16 squares one after the other, then the wave
// shuffle tree (6 levels), then the four waves pairwise (2 levels): a fixed order, so the same data gives the same bits.
__global__ __launch_bounds__(256) void sumsq_multi_kernel(const t2v_adamw_tensor* __restrict__ table, int nt, long long nblocks,
                                                          float* __restrict__ ws) {
    constexpr int Q = T2V_ADAMW_BLOCK / (256 * 4);
    __shared__ float sh[4];
    const int tid = threadIdx.x;
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const t2v_adamw_tensor d = table[owner_of(table, nt, blk)];
        const long long e0 = (blk - d.work0) * T2V_ADAMW_BLOCK;
        float a = 0.f;
        if (e0 >= 0 && e0 < d.n) {
            const long long left = d.n - e0;
            const int cnt = left < T2V_ADAMW_BLOCK ? (int)left : T2V_ADAMW_BLOCK;
            const float* g = d.grad + e0;
            if (((uintptr_t)d.grad & 15) != 0) {
#pragma unroll 1
                for (int i = tid; i < cnt; i += 256) a += g[i] * g[i];
            } else {
                float4 G[Q];
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    const int i = (j * 256 + tid) * 4;
                    if (i + 4 <= cnt) G[j] = *(const float4*)(g + i);
                }
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    const int i = (j * 256 + tid) * 4;
                    if (i + 4 <= cnt) {
                        a += G[j].x * G[j].x; a += G[j].y * G[j].y; a += G[j].z * G[j].z; a += G[j].w * G[j].w;
                    } else {
#pragma unroll 1
                        for (int e = i; e < cnt; ++e) a += g[e] * g[e];
                    }
                }
            }
        }
        a = wave_sum(a);
        if ((tid & 63) == 0) sh[tid >> 6] = a;
        __syncthreads();
        if (tid == 0) ws[blk] = (sh[0] + sh[1]) + (sh[2] + sh[3]);   // (0 for a work block that no tensor owns)
        __syncthreads();   // sh is written again in the next round
    }
}
// out[0] = sqrt(sum of the partials), summed in double in a fixed order (sumsq_final_kernel's); out[1] = the clip coefficient of
// torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)), a NaN norm giving a NaN coefficient as torch.clamp does.
__global__ __launch_bounds__(256) void sumsq_multi_final_kernel(const float* __restrict__ ws, long long nblk, float max_norm, float* out) {
    __shared__ double sh[256];
    double a = 0.0;
#pragma unroll 8
    for (long long i = threadIdx.x; i < nblk; i += 256) a += (double)ws[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(sh[0]);
        float coef = 1.0f;
        if (max_norm > 0.f) {
            coef = max_norm / (norm + 1e-6f);
            if (coef > 1.0f) coef = 1.0f;   // (a NaN stays)
        }
        out[0] = norm;
        out[1] = coef;
    }
}
__global__ __launch_bounds__(256) void scale_multi_kernel(const t2v_adamw_tensor* __restrict__ table, int nt, long long nblocks,
                                                          const float* __restrict__ coef_dev) {
    constexpr int Q = T2V_ADAMW_BLOCK / (256 * 4);
    const float c = *coef_dev;
    if (c == 1.0f) return;   // nothing to clip: g * 1.0f is g, bit for bit, and the gradients are not touched
    const int tid = threadIdx.x;
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const t2v_adamw_tensor d = table[owner_of(table, nt, blk)];
        const long long e0 = (blk - d.work0) * T2V_ADAMW_BLOCK;
        if (e0 < 0 || e0 >= d.n) continue;
        const long long left = d.n - e0;
        const int cnt = left < T2V_ADAMW_BLOCK ? (int)left : T2V_ADAMW_BLOCK;
        float* g = d.grad + e0;
        if (((uintptr_t)d.grad & 15) != 0) {
#pragma unroll 1
            for (int i = tid; i < cnt; i += 256) g[i] = g[i] * c;
            continue;
        }
        float4 G[Q];
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const int i = (j * 256 + tid) * 4;
            if (i + 4 <= cnt) G[j] = *(const float4*)(g + i);
        }
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const int i = (j * 256 + tid) * 4;
            if (i + 4 <= cnt) {
                *(float4*)(g + i) = make_float4(G[j].x * c, G[j].y * c, G[j].z * c, G[j].w * c);
            } else {
#pragma unroll 1
                for (int e = i; e < cnt; ++e) g[e] = g[e] * c;
            }
        }
    }
}
// persistent grid, sized as blocks8 is: 8 workgroups per CU of a 256-CU part; fewer when there is less work
inline unsigned blocks_multi(long long nblocks) { return (unsigned)(nblocks < 2048 ? nblocks : 2048); }
}  // namespace

extern "C" int t2v_adamw_multi(const t2v_adamw_tensor* table, int n_tensors, long long n_blocks, const t2v_adamw_hyper* hyper,
                               int n_hyper, float grad_scale, const float* grad_scale_dev, void* stream) {
    T2V_REQUIRE(table && hyper && n_tensors > 0 && n_blocks >= n_tensors && n_hyper >= 1 && n_hyper <= T2V_ADAMW_MAX_HYPER, T2V_EINVAL,
                "t2v_adamw_multi");
    T2V_REQUIRE((uintptr_t)table % 8 == 0, T2V_ESHAPE, "t2v_adamw_multi: the table must be 8-byte aligned");
    AdamwRows rows;
    for (int i = 0; i < T2V_ADAMW_MAX_HYPER; ++i) {
        const t2v_adamw_hyper& h = hyper[i < n_hyper ? i : 0];
        T2V_REQUIRE(h.step >= 1, T2V_EINVAL, "t2v_adamw_multi: step < 1");
        const float bc1 = 1.0f - powf(h.beta1, (float)h.step), bc2 = 1.0f - powf(h.beta2, (float)h.step);
        rows.lr[i] = h.lr; rows.wd[i] = h.weight_decay; rows.b1[i] = h.beta1; rows.b2[i] = h.beta2; rows.eps[i] = h.eps;
        rows.bc1[i] = bc1; rows.bc2_sqrt[i] = sqrtf(bc2);
    }
    hipLaunchKernelGGL(adamw_multi_kernel, dim3(blocks_multi(n_blocks)), dim3(256), 0, (hipStream_t)stream, table, n_tensors, n_blocks,
                       rows, n_hyper, grad_scale, grad_scale_dev);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_sumsq_multi(const t2v_adamw_tensor* table, int n_tensors, long long n_blocks, float* ws, float max_norm, float* out,
                               void* stream) {
    T2V_REQUIRE(table && ws && out && n_tensors > 0 && n_blocks >= n_tensors, T2V_EINVAL, "t2v_sumsq_multi");
    T2V_REQUIRE((uintptr_t)table % 8 == 0, T2V_ESHAPE, "t2v_sumsq_multi: the table must be 8-byte aligned");
    hipLaunchKernelGGL(sumsq_multi_kernel, dim3(blocks_multi(n_blocks)), dim3(256), 0, (hipStream_t)stream, table, n_tensors, n_blocks, ws);
    T2V_CHECK_LAUNCH();
    hipLaunchKernelGGL(sumsq_multi_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, n_blocks, max_norm, out);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}
extern "C" int t2v_scale_multi(const t2v_adamw_tensor* table, int n_tensors, long long n_blocks, const float* coef_dev, void* stream) {
    T2V_REQUIRE(table && coef_dev && n_tensors > 0 && n_blocks >= n_tensors, T2V_EINVAL, "t2v_scale_multi");
    T2V_REQUIRE((uintptr_t)table % 8 == 0, T2V_ESHAPE, "t2v_scale_multi: the table must be 8-byte aligned");
    hipLaunchKernelGGL(scale_multi_kernel, dim3(blocks_multi(n_blocks)), dim3(256), 0, (hipStream_t)stream, table, n_tensors, n_blocks,
                       coef_dev);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

// ---- decoded video -> uint8 frames (include/t2v_hip.h: t2v_video_to_u8) ------------------------------------------------------------
// (B,3,T,H,W) -> (B,T,H,W,3): a lane takes four consecutive pixels of one frame from the three channel planes (a 16- or 8-byte load
// each) and writes their twelve bytes as three words, so a wave writes 768 contiguous bytes.  A lane whose four addresses are not on
// their boundaries (an unaligned base, H * W not a multiple of 4) and the last lane of a frame with fewer than four pixels move
// element by element.  The value: every operation rounded to fp32 on its own, so that the bytes are torch's, bit for bit.
namespace {
#ifdef T2V_HOSTSIM   // (plain C++ on the host rounds every operation on its own)
__device__ __forceinline__ float u8_add(float a, float b) { return a + b; }
__device__ __forceinline__ float u8_mul(float a, float b) { return a * b; }
#else
__device__ __forceinline__ float u8_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float u8_mul(float a, float b) { return __fmul_rn(a, b); }
#endif
__device__ __forceinline__ uint32_t u8_of(float v) {
    if (v != v) return 0u;
    const float y = fminf(fmaxf(v, -1.0f), 1.0f);
    return (uint32_t)(int)u8_mul(u8_mul(u8_add(y, 1.0f), 0.5f), 255.0f);   // (in [0, 255]: truncation toward zero)
}
__device__ __forceinline__ float u8_h2f(uint32_t bits, int dt) {
    if (dt == T2V_BF16) return __uint_as_float(bits << 16);
    const uint16_t b = (uint16_t)bits;
    _Float16 h;
    memcpy(&h, &b, 2);
    return (float)h;
}
__global__ __launch_bounds__(256) void video_to_u8_kernel(const void* __restrict__ x, int dt, int T, long long HW, long long nq, long long total,
                                                          unsigned char* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const long long bt = gid / nq, p0 = (gid - bt * nq) * 4;
    const long long b = bt / T, t = bt - b * T;
    const int es = dt == T2V_F32 ? 4 : 2;
    const int n = HW - p0 < 4 ? (int)(HW - p0) : 4;
    long long src[3];
    uintptr_t bits = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        src[c] = ((b * 3 + c) * T + t) * HW + p0;
        bits |= (uintptr_t)x + (uintptr_t)(src[c] * es);
    }
    unsigned char* o = out + (bt * HW + p0) * 3;
    if (n == 4 && (bits & (uintptr_t)(4 * es - 1)) == 0 && ((uintptr_t)o & 3) == 0) {
        uint32_t v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (dt == T2V_F32) {
                const uint4 u = *(const uint4*)((const float*)x + src[c]);
                v[c][0] = u8_of(__uint_as_float(u.x)); v[c][1] = u8_of(__uint_as_float(u.y));
                v[c][2] = u8_of(__uint_as_float(u.z)); v[c][3] = u8_of(__uint_as_float(u.w));
            } else {
                const uint2 u = *(const uint2*)((const uint16_t*)x + src[c]);
                v[c][0] = u8_of(u8_h2f(u.x & 0xffffu, dt)); v[c][1] = u8_of(u8_h2f(u.x >> 16, dt));
                v[c][2] = u8_of(u8_h2f(u.y & 0xffffu, dt)); v[c][3] = u8_of(u8_h2f(u.y >> 16, dt));
            }
        }
        uint32_t* ow = (uint32_t*)o;   // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        ow[0] = v[0][0] | (v[1][0] << 8) | (v[2][0] << 16) | (v[0][1] << 24);
        ow[1] = v[1][1] | (v[2][1] << 8) | (v[0][2] << 16) | (v[1][2] << 24);
        ow[2] = v[2][2] | (v[0][3] << 8) | (v[1][3] << 16) | (v[2][3] << 24);
        return;
    }
    for (int p = 0; p < n; ++p)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * p + c] = (unsigned char)u8_of(load_as_f32(x, dt, src[c] + p));
}
}  // namespace

extern "C" int t2v_video_to_u8(const void* x, int dt, int B, int T, int H, int W, void* out, void* stream) {
    T2V_REQUIRE(x && out && B > 0 && T > 0 && H > 0 && W > 0, T2V_EINVAL, "t2v_video_to_u8: null pointer / non-positive size");
    T2V_REQUIRE(dt == T2V_F32 || dt == T2V_BF16 || dt == T2V_F16, T2V_ESHAPE, "t2v_video_to_u8: the video is fp32, bf16 or fp16");
    T2V_REQUIRE((uintptr_t)x % (dt == T2V_F32 ? 4 : 2) == 0, T2V_ESHAPE, "t2v_video_to_u8: the video is off its element boundary");
    const long long HW = (long long)H * W, nq = (HW + 3) / 4, total = (long long)B * T * nq;
    T2V_REQUIRE((total + 255) / 256 < (1ll << 31), T2V_ESHAPE, "t2v_video_to_u8: too many pixels for one launch");
    hipLaunchKernelGGL(video_to_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dt, T, HW, nq, total,
                       (unsigned char*)out);
    T2V_CHECK_LAUNCH();
    return T2V_OK;
}

// ---- library state ---------------------------------------------------------------------------------
static thread_local char g_err[256] = "";
void t2v_set_error(const char* msg) {
    size_t i = 0;
    for (; msg && msg[i] && i + 1 < sizeof(g_err); ++i) g_err[i] = msg[i];
    g_err[i] = 0;
}
static void* g_zero[64] = {nullptr};
const void* t2v_zero_page() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!g_zero[dev]) {
        void* p = nullptr;
        if (hipMalloc(&p, 4096) != hipSuccess) return nullptr;
        if (hipMemset(p, 0, 4096) != hipSuccess) return nullptr;
        g_zero[dev] = p;
    }
    return g_zero[dev];
}
extern "C" const char* t2v_last_error(void) { return g_err; }
extern "C" int t2v_version(void) { return 100; }
extern "C" int t2v_init(void) { return t2v_zero_page() ? T2V_OK : T2V_EHIP; }
