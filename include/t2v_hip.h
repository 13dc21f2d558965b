/*
 * t2v_hip.h — C-ABI of libt2v_hip.so: the MI355X (gfx950) kernels under the
 * t2v-turbo denoise hot path (VideoCrafter2 3D-UNet forward + KL-VAE decoder).
 *
 * The reference (Ji4chenLi/t2v-turbo) is 100 % Python and has no FFI layer; what
 * this library replaces is the set of ATen/cuDNN/cuBLAS/xformers calls its hot
 * path issues.  Each entry point cites the reference call site(s) it stands in
 * for (paths relative to the reference root).
 *
 * Conventions
 *  - plain C: raw device pointers, ints, a stream handle; no torch types.
 *  - activations are bf16, token-major ("NHWC"): row m = ((b*F + f)*H + y)*W + x,
 *    C contiguous channels per row (row stride `ld*` in elements).
 *  - the caller owns every buffer (inputs, outputs, workspaces); the library
 *    allocates nothing per call, never synchronises and launches only on the
 *    stream it is given (hipStream_t passed as void*; NULL = default stream).
 *  - every function returns 0 on success, a negative T2V_E* code on a bad
 *    argument / unsupported shape, and never throws across the boundary.
 */
#ifndef T2V_HIP_H
#define T2V_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define T2V_OK 0
#define T2V_EINVAL (-1)   /* bad argument */
#define T2V_ESHAPE (-2)   /* shape/alignment not supported by the kernel */
#define T2V_EHIP (-3)     /* HIP runtime error at launch */

/* element types of boundary tensors */
#define T2V_F32 0
#define T2V_BF16 1
#define T2V_F16 2

/* library version / build info; also forces lazy per-device state (16-byte zero page
 * used for conv zero padding) to exist before a stream capture starts. */
int t2v_version(void);
int t2v_init(void);
const char* t2v_last_error(void);

/* ---------------------------------------------------------------- GEMM / implicit-GEMM conv
 * out[M,N] = epilogue( alpha * gather(A)[M,K] * W[N,K]^T )
 *
 * Replaces: nn.Linear (lvdm/modules/attention.py:71-76,348,370,433,468,519,537-538;
 * openaimodel3d.py:403-430,172-178), nn.Conv2d 3x3 / 3x3-s2 / 1x1
 * (openaimodel3d.py:155-159,179-184,63-72,98-100,192-193,669; ae_modules.py:149-175,550-552),
 * nn.Conv3d (3,1,1) (openaimodel3d.py:274-296), nn.Conv1d k=1 (attention.py:425-431),
 * F.interpolate(nearest x2)+conv (openaimodel3d.py:104-111; ae_modules.py:118-121),
 * torch.cat skip concat feeding a conv (openaimodel3d.py:733), and the bmm pairs of the
 * VAE AttnBlock (ae_modules.py:59-69).
 */
#define T2V_GEMM_LINEAR 0      /* K = Cin; A row m is source row m                          */
#define T2V_GEMM_CONV3X3 1     /* 3x3, stride 1, pad 1; K = 9*Cin, tap-major (ky,kx) then c */
#define T2V_GEMM_CONV3X3_S2 2  /* 3x3, stride 2, pad 1                                      */
#define T2V_GEMM_CONV3X3_UP2 3 /* 3x3 s1 p1 over the nearest-x2 upsampled input (never materialised) */
#define T2V_GEMM_TCONV3 4      /* (3,1,1) temporal conv, pad (1,0,0); K = 3*Cin, tap = frame offset   */
#define T2V_GEMM_CONV3X3_S2_PAD01 5 /* 3x3 s2, pad right/bottom only (VAE encoder Downsample, ae_modules.py:98-102) */

#define T2V_ACT_NONE 0
#define T2V_ACT_GEGLU 1 /* out[m,j] = x*gelu(gate); W rows packed in 64-row groups [32 x | 32 gate]; out has N/2 cols */
#define T2V_ACT_SILU 2

/* Operand forms of the descriptor (t2v_gemm, t2v_conv_halo, t2v_linear_pr; what tests/gemm_form_cases.py holds the kernels to)
 *  - Every operand may be a view into a larger buffer.  Row strides (elements): lda0 >= c0, lda1 >= c1, ldw >= K (conv_halo:
 *    >= t2v_conv_halo_pack_cols), ldo >= n_out, ldr >= n_out, ld_rowvec >= n_out, ld_ln_out >= N, ld_lora_t >= 64 leaves,
 *    ld_lora_u >= 64, ld_rowstat >= N / 16, lnf_ld >= 2 lnf_nblk (n_out = N, or N / 2 with GEGLU).  A shorter stride is an invalid
 *    descriptor: every entry point that takes the descriptor — the *_supported / t2v_gemm_plan queries included — returns a negative
 *    code and launches nothing.  lda0, lda1, ldw % 8 == 0 and a0, a1, w 16-byte aligned (checked).  out, residual, bias, rowvec need no
 *    alignment: 16-byte aligned bases with ldo, ldr % 8 == 0, ld_rowvec % 4 == 0 and n_out % 4 == 0 select the vector store path, anything
 *    else the element-wise one (same values; GEGLU, split-K and the fused epilogues exist on the vector path only).
 *  - READ: columns [0, c0) / [0, c1) of the A rows the gather addresses; columns [0, K) of W rows [0, N); bias [0, N); rowvec rows
 *    [0, ceil(M / rowvec_div)) x columns [0, n_out); residual rows [0, M) x columns [0, n_out); lnf_stats rows [0, M) x floats
 *    [0, 2 lnf_nblk); lnf_s [0, N); lora_t rows [0, M) x columns [0, 64 leaves); lora_u rows [0, N) x columns [0, 64) — ALL 64: the
 *    rank columns beyond the leaf's rank must hold zero; the conv_halo pack's columns [0, t2v_conv_halo_pack_cols) of rows [0, N): the
 *    padding behind 9 C must hold zero.
 *  - NOT READ (may hold anything, NaN included): the stride gaps of every operand; A rows >= M of a LINEAR launch and every source row a
 *    padding tap would address — taps outside the (n_img, h, w) grid, in a TCONV3 launch outside the clip's frames, come from the
 *    library's zero page, never from the neighbouring row / image / clip; W rows >= N (the tail of the last channel tile is the zero
 *    page's); the tail of a weight row between K and ldw.
 *  - WRITTEN: columns [0, n_out) of out rows [0, M) (per batch element: at its o_stride offset); ln_out likewise over N columns;
 *    rowstat_out rows [0, M) x floats [0, N / 16); colstat_out [M / 32][N][2]; the first splits * batch * M * N floats of ws when K is
 *    split.  Nothing else: not the stride gaps, not rows >= M, not the workspace behind those floats, not the workspace at all when the
 *    launch runs in one split (t2v_gemm_plan tells).
 *  - Rounding: the product is accumulated in fp32 over K in an unspecified order (split-K: fp32 partial sums added in split order).  The
 *    epilogue is fp32 throughout — alpha * acc, + bias, GEGLU value * gelu(gate) (gate = alpha * acc + bias of the gate row; gelu =
 *    csrc/gelu_poly.h, |error| < 4.2e-5 for |gate| <= 8), dropout mask and scale, + rowvec, + residual (also in t2v_conv_halo: the
 *    residual meets the fp32 accumulator, not a rounded product), + the LoRA term, SiLU — and the result is rounded ONCE, to nearest
 *    even, when it is stored as bf16 (not at all with out_f32).  rowstat_out and ln_out are taken from the fp32 epilogue values,
 *    colstat_out from the bf16-rounded outputs.  ln_in / gn_coef (t2v_linear_pr) round the normalised A rows to bf16 before the product. */
typedef struct t2v_gemm_desc {
    /* A: bf16 activations; optional second source = virtual channel concat [a0 | a1] */
    const void* a0;
    const void* a1;
    int c0, c1;     /* channels per source (c1 = 0 without a1); c0, c1 multiples of 64 */
    int lda0, lda1; /* row strides, elements */
    int mode;       /* T2V_GEMM_* */
    int n_img, h_in, w_in; /* input grid for conv modes (n_img = B*F) */
    int frames;     /* TCONV3: frames per clip */
    int M, N;       /* output rows / cols (LINEAR: M = source rows) */
    /* W: bf16 [N][K], row stride ldw (elements), K = taps*(c0+c1) */
    const void* w;
    int ldw;
    /* batching: z in [0,batch): z0 = z / batch_inner, z1 = z % batch_inner; strides in elements */
    int batch, batch_inner;
    long long a_stride0, a_stride1, w_stride0, w_stride1, o_stride0, o_stride1;
    /* epilogue */
    float alpha;
    const float* bias;   /* [N] fp32 or NULL */
    const float* rowvec; /* fp32: += rowvec[(m / rowvec_div) * ld_rowvec + n], or NULL (time-embedding add) */
    int rowvec_div, ld_rowvec;
    const void* residual; /* bf16 [M][ldr] (batched with the o_strides), or NULL */
    int ldr;
    int act;     /* T2V_ACT_* */
    void* out;   /* bf16 (or fp32 if out_f32) [M][ldo] */
    int ldo;
    int out_f32;
    /* scheduling hints (0 = library heuristic): workgroup tile id and split-K factor.  Split-K needs a
     * caller workspace of >= split_k*batch*M*N*4 bytes; without one the library never splits. */
    int tile_cfg, split_k;
    void* ws;
    long long ws_bytes;
    /* dropout between the product and the residual (0 threshold = off): out = keep ? (alpha*acc + bias) / (1 - p) : 0, then
     * + rowvec + residual.  The mask is t2v_dropout_bf16's: one splitmix64 word per QUAD of adjacent elements of a
     * row-major [rows][drop_ncols] matrix in which this launch's output starts at column drop_col0 (both multiples of 4), 16 bits per
     * element against drop_thr >> 16 (drop_thr = p * 2^32): p is resolved to 2^-16, so the drop probability is p' = (drop_thr >> 16) / 65536
     * and the caller passes drop_inv_keep = 1 / (1 - p') = 65536 / (65536 - (drop_thr >> 16)) (E[out] = in exactly; p < 2^-16 keeps
     * everything at scale 1); the 64-bit seed is read from device memory.  LoraInjected*.forward's dropout(up(down(x))) * scale
     * (utils/lora.py:45-50) as the epilogue of the up-projection.  Not combined with GEGLU / split-K. */
    const void* drop_seed;
    unsigned drop_thr, drop_site;
    float drop_inv_keep;
    int drop_ncols, drop_col0;
    /* LayerNorm second output (NULL = off): ln_out[m][n] = (out[m][n] - mean_m) * rstd_m * ln_gamma[n] + ln_beta[n] over the N
     * columns of the row (fp32 statistics on the fp32 epilogue values, two-pass), bf16 [M][ld_ln_out].  The pre-LN residual
     * stream and its LayerNorm (BasicTransformerBlock._forward, attention.py:300-311) from one launch.  N == 320 only (the
     * 160x320 workgroup tile holds whole rows); no batch, no activation, bf16 out, alpha == 1. */
    const float* ln_gamma;
    const float* ln_beta;
    float ln_eps;
    void* ln_out;
    int ld_ln_out;
    /* ---- normalisation statistics as by-products of the producing GEMM, LayerNorm folded into the consuming one ----------
     * (all NULL = off; honoured by the fast kernels only: ask t2v_gemm_fuse_supported first, t2v_gemm refuses otherwise)
     *
     * rowstat_out [M][ld_rowstat] fp32: for every output row and every 32-column block b the pair (sum, sum of squares) of the
     * fp32 epilogue values at floats [2b, 2b+1] — the row statistics the NEXT LayerNorm needs (attention.py:300-311), written
     * by the GEMM that produces its input instead of a pass over the tensor.  N % 32 == 0, ld_rowstat >= N/16, % 4 == 0.
     *
     * colstat_out [M/32][N][2] fp32: for every 32-row slab and every column (sum, sum of squares) of the bf16-ROUNDED outputs —
     * what GroupNorm (openaimodel3d.py:223-254, lvdm/basics.py:78-89) reduces per (unit, group); t2v_group_norm_cs finishes
     * them for any unit whose row count is a multiple of 32.  M % 32 == 0.
     *
     * lnf_stats: this launch CONSUMES LayerNorm(x) without x ever being normalised in memory: A holds the raw rows x [M][C],
     * W holds W diag(gamma) (bf16), lnf_s[n] = sum_c W'[n][c] (fp32, of the bf16-rounded W'), bias[n] = b[n] + sum_c W[n][c]
     * beta[c]; with (mean_m, rstd_m) from the producer's rowstat (lnf_nblk blocks of 32 columns, C = 32 lnf_nblk):
     *     out[m][n] = rstd_m * (acc[m][n] - mean_m * lnf_s[n]) + bias[n]      (then GEGLU / activation as usual)
     * LINEAR mode, no batch, no residual / rowvec / dropout, alpha == 1. */
    float* rowstat_out;
    int ld_rowstat;
    float* colstat_out;
    const float* lnf_stats;
    int lnf_ld, lnf_nblk;
    float lnf_eps;
    const float* lnf_s;
    /* ---- LoRA branch in the base leaf's epilogue (NULL = off; fast kernels only: ask t2v_gemm_fuse_supported first) ------------
     * lora_t [M][ld_lora_t] bf16: the rank-64 down-projections t_l = x (*) D_l of the leaves this launch's N columns belong to,
     * leaf l (columns [l * lora_n_leaf, (l + 1) * lora_n_leaf)) at columns [64 l, 64 l + 64);  lora_u [N][ld_lora_u] bf16: row n
     * = the up-projection row of output channel n (rank zero-padded to 64).  The launch then computes
     *     out = epilogue( acc + bias + rowvec + residual + lora_scale * dropout( t_l u_n^T ) )
     * i.e. LoraInjected*.forward (utils/lora.py:45-50,124-129,204-209) in ONE launch after the down-projection: the M x N
     * up-projection z is never written or re-read.  With lora_t set, the drop_* fields mask the LoRA product only (drop_thr = 0:
     * no dropout); the mask is t2v_dropout_bf16's over the [M][drop_ncols] matrix, so it is bit-identical to the three-launch form.
     * lora_n_leaf % 32 == 0, no GEGLU / batch / split-K, alpha == 1, bf16 out.
     * Validated on the host SIMT simulator (tests/test_hostsim_gemm_fuse.py) and, in the last seconds of round 3's GPU budget, on
     * MI355X (tests/test_gpu_gemm_fuse.py at the UNet's shapes; the gradient engine at tiny width against the reference's LoRA
     * gradients and with replayed train-mode masks).  NOT YET TIMED: the engines use it only with T2V_LORA_EPILOGUE=1. */
    const void* lora_t;
    int ld_lora_t;
    const void* lora_u;
    int ld_lora_u;
    int lora_n_leaf;
    float lora_scale;
    /* ---- LayerNorm of the INPUT rows, applied while the activation panel is filled (t2v_linear_pr only; 0 = off) ---------------------
     * ln_in != 0: the launch computes epilogue( LayerNorm(A)[M, K] x W^T ) with LayerNorm over the K = c0 columns of every A row
     * (ln_gamma / ln_beta fp32 [K], ln_eps; two-pass fp32 statistics, the normalised rows rounded to bf16 exactly as a t2v_layernorm
     * launch would have written them): norm1 / norm2 / norm3 of BasicTransformerBlock (attention.py:300-311) where their output feeds
     * ONE Linear — no LayerNorm launch, no normalised tensor in memory.  ln_out must be NULL; not combined with a residual.
     * t2v_gemm and t2v_conv_halo refuse a descriptor with ln_in set. */
    int ln_in;
    /* ---- GroupNorm applied to the INPUT rows while the activation panel is filled (t2v_linear_pr only; NULL = off) -----------------------
     * gn_coef fp32 [units][2][K]: the per-channel affine t2v_gn_coef_cs made of the producers' column statistics (coef[u][0][c] = rstd
     * gamma[c], coef[u][1][c] = beta[c] - mean rstd gamma[c]); unit of row m = m / gn_rows_per_unit.  The launch computes
     * epilogue( (A * coef[u][0] + coef[u][1]) x W^T ), the normalised rows rounded to bf16 as t2v_group_norm_cs would have written them —
     * SpatialTransformer / TemporalTransformer: x = proj_in(norm(x)) (attention.py:373-389,471-513) without the normalised tensor in
     * memory.  gn_rows_per_unit a multiple of the panel height (160 rows at K = 320, 96 at K = 640: ask t2v_linear_pr_supported), no
     * SiLU, plain epilogue (bias only), not combined with ln_in.  t2v_gemm and t2v_conv_halo refuse a descriptor with gn_coef set. */
    const float* gn_coef;
    int gn_rows_per_unit;
} t2v_gemm_desc;

int t2v_gemm(const t2v_gemm_desc* d, void* stream);
/* 1 if t2v_gemm would honour the descriptor's rowstat_out / colstat_out / lnf_stats fields (it resolves the tile and the
 * split-K factor exactly as the launch does: fast kernel, one K split, a tile that carries the fused epilogue), 0 if the
 * caller has to use the standalone normalisation kernels, negative on an invalid descriptor.  Launches nothing. */
int t2v_gemm_fuse_supported(const t2v_gemm_desc* d);
/* The tile id and the K-split count t2v_gemm would use for the descriptor (resolved exactly as the launch does; launches nothing).
 * The gradient engine asks with the PLAIN descriptor before it attaches a LoRA epilogue (lora_*: one K split only): where the plain
 * launch would split K, the three-launch form (up-projection launches + split base leaf) is faster. */
int t2v_gemm_plan(const t2v_gemm_desc* d, int* tile_cfg, int* splits);
/* 3x3 convolution (stride 1, pad 1) with the activation tile's halo slab RESIDENT in LDS across all nine filter taps
 * (csrc/conv_halo.hip): same descriptor as t2v_gemm (mode T2V_GEMM_CONV3X3, virtual concat allowed; no batch / split-K /
 * dropout / GEGLU / fp32 output; epilogue: bias, rowvec, residual, SiLU, colstat_out), EXCEPT that `w` holds the SLAB-MAJOR pack:
 * K order (32-channel sub-slab, tap, channel) = [N][C/32][9][32] instead of t2v_gemm's tap-major [N][9][C] — one
 * (sub-slab, tap) pair is 64 contiguous bytes of a weight row, a stage of pairs one contiguous run — with every row zero-padded
 * to t2v_conv_halo_pack_cols(C) elements (ldw >= that).  Replaces the same reference call sites as t2v_gemm's 3x3 mode
 * (openaimodel3d.py:155-159,179-184).  tile_cfg 40 / 41 / 42 / 43 force the 320x160 / 320x80 / 160x80 (16-wide grid) / 160x80
 * (32-wide grid) workgroup tile (tokens x channels), anything else lets the library choose by grid fill.
 * t2v_conv_halo_supported: 0 = not taken (use t2v_gemm with the tap-major pack), 1 = taken; negative = invalid descriptor.
 * Launches nothing. */
int t2v_conv_halo(const t2v_gemm_desc* d, void* stream);
int t2v_conv_halo_supported(const t2v_gemm_desc* d);
int t2v_conv_halo_pack_cols(int channels);
int t2v_conv_halo_force_config(int cfg);
int t2v_conv_halo_debug(int bits);   /* ablation bits; honoured by -DT2V_HALO_ABLATE tool builds only */
/* Short-K linear layers (K = 320 / 640) with the activation panel RESIDENT in LDS and the weights streamed into registers in MFMA
 * fragment order (csrc/linear_pr.hip): same descriptor as t2v_gemm (mode T2V_GEMM_LINEAR, one source, no batch / split-K / rowvec /
 * dropout / fused statistics / fp32 output; epilogue: bias, then GEGLU, or an optional residual), EXCEPT that `w` holds the
 * FRAGMENT pack of the [N][K] matrix t2v_gemm takes (for GEGLU: of its 64-row [32 value | 32 gate] interleave), N % 64 == 0:
 *     pack[chunk q = n / 64][step s = k / 16][block b = (n % 64) / 32][lane l][e = 0..7]  (bf16, N * K elements)
 *         = W[64 q + 32 b + 16 ((i >> 2) & 1) + 4 (i >> 3) + (i & 3)][16 s + 8 (l >> 5) + e],   i = l & 31
 * i.e. every (chunk, step, block) is the 1 KiB v_mfma_f32_32x32x16_bf16 A operand of 32 output rows x 16 K, lane-major, with the
 * rows of a block permuted so that a lane's 16 accumulator registers are 16 consecutive output channels.
 * Replaces the same reference call sites as t2v_gemm's LINEAR mode at these widths: the GEGLU projection
 * (lvdm/modules/attention.py:516-523), q | k | v (:71-76), to_out (:164), proj_in / proj_out (:373-389,471-513).
 * t2v_linear_pr_supported: 0 = not taken (use t2v_gemm with the plain [N][K] matrix), 1 = taken; negative = invalid descriptor.
 * Launches nothing. */
int t2v_linear_pr(const t2v_gemm_desc* d, void* stream);
int t2v_linear_pr_supported(const t2v_gemm_desc* d);
int t2v_linear_pr_debug(int bits);         /* ablation bits; honoured by -DT2V_LPR_ABLATE tool builds only */
int t2v_linear_pr_force_split(int ny);     /* tuning hook: column splits (workgroup rows) for every following call, 0 = library rule */
/* tuning/test hooks: override tile id / split-K factor for every following call (0 = off) */
int t2v_gemm_force_config(int cfg);
#ifdef T2V_EXPERIMENTAL /* measured negative results: compiled and exported by a T2V_EXPERIMENTAL=1 build (libt2v_hip_exp.so) only */
/* t2v_gemm's second kernel family (csrc/gemm2.hip: static-schedule main loop, 80x80 wave tiles; tile ids 50 = 320x160, 51 = 160x160)
 * for LINEAR / TCONV3 launches with a plain epilogue (bias, residual, SiLU, colstat_out).  Measured slower than the tuned first-family
 * tiles on the UNet's shapes (operand-delivery bound), so it is OFF by default: t2v_gemm2_enable(1) (or T2V_GEMM2=1) lets the library
 * route long-K launches to it by its own rule, a forced tile id 50 / 51 puts an eligible launch on it whatever its K. */
int t2v_gemm2_enable(int on);
#endif
int t2v_gemm_force_split(int splits);
int t2v_gemm_num_configs(void);

#ifdef T2V_EXPERIMENTAL
/* The GEGLU feed-forward of a BasicTransformerBlock, LayerNorm and residual included, in ONE launch (measured slower than the three
 * launches it replaces: profiles/r03_ffn_fused_pmc.csv):
 *     out = x + W2 . [value . gelu(gate)] + b2,   [value | gate] = W1 . LayerNorm(x) + b1
 * (lvdm/modules/attention.py:300-311 `x = self.ff(self.norm3(x)) + x`, :516-542 FeedForward / GEGLU).  The 4C-wide hidden
 * activation never reaches memory.  x, out: bf16 [M][ld] (not in place); C = 320 (and 64 for tests): t2v_ffn_fused_supported.
 * The weights come PRE-PACKED in MFMA fragment order, LayerNorm's affine folded into W1 / b1 (W1 diag(gamma), b1 + W1 beta):
 *   w1p bf16 [C/8 chunks][4 row tiles: value a | gate a | value b | gate b][C/32 k-steps][64 lanes][8]:
 *       lane l = W1'[row][32 s + 8 (l >> 4) .. +8], row = (gate ? 4C : 0) + 32 chunk + 16 (b ? 1 : 0) + (l & 15)
 *   b1p fp32 [C/8][4][16] in the same row order
 *   w2p bf16 [C/8 chunks][C/16 row tiles][64 lanes][8]: lane l = W2[16 t + (l & 15)][32 chunk + h], h = 4 (l >> 4) + e for
 *       e < 4 (pair a), 16 + 4 (l >> 4) + e - 4 for e >= 4 (pair b)
 *   b2 fp32 [C] */
int t2v_ffn_fused_supported(int C);
int t2v_ffn_fused(const void* x, int ldx, int M, int C, const void* w1p, const float* b1p, const void* w2p, const float* b2,
                  float ln_eps, void* out, int ldo, void* stream);
#endif

/* direct 3x3 s1 p1 conv for tiny Cin (the 4-channel latent): x bf16 [M][cin] (cin <= 8),
 * w fp32 [cout][9][cin], bias fp32 [cout], out bf16 [M][cout]; x and out are contiguous (no row strides), taps outside an image are zero
 * (never the neighbouring row / image), fp32 accumulation, one rounding to bf16.
 * Replaces input_blocks.0 (openaimodel3d.py:435) and Decoder.conv_in (ae_modules.py:550-552). */
int t2v_conv3x3_small_cin(const void* x, int n_img, int h, int w, int cin, const float* wgt,
                          const float* bias, int cout, void* out, void* stream);

/* ---------------------------------------------------------------- normalisation
 * GroupNorm(32) in two phases over token-major data with optional virtual concat.
 * A "unit" is the statistics extent: one frame (ResBlock / SpatialTransformer / VAE, 4-D input)
 * or all frames of a clip (TemporalConvBlock / TemporalTransformer, 5-D input):
 * rows_per_unit consecutive rows.  Replaces GroupNormSpecific / nn.GroupNorm (+ nn.SiLU)
 * (lvdm/basics.py:78-89; openaimodel3d.py:155-157,179-181,275-292,666-668;
 * attention.py:340-342,422-424; ae_modules.py:11-19).
 * ws: fp32 workspace of t2v_gn_ws_floats(...) floats.  stats out: [n_units][groups][2] = (mean, rstd).
 * Row strides: multiples of 8, ld0 >= c0, ld1 >= c1, ldo >= c0 + c1 (checked; the same holds for every normalisation entry point below
 * and for their backward forms).  Only the c0 / c1 columns of a row are read, only the first c0 + c1 columns of an output row and the
 * first *_ws_floats floats of a workspace are written. */
long long t2v_gn_ws_floats(int n_units, int rows_per_unit, int groups);
int t2v_gn_stats(const void* x0, int c0, int ld0, const void* x1, int c1, int ld1, int n_units,
                 int rows_per_unit, int groups, float eps, float* ws, float* stats, void* stream);
int t2v_gn_apply(const void* x0, int c0, int ld0, const void* x1, int c1, int ld1, int n_units,
                 int rows_per_unit, int groups, const float* stats, const float* gamma,
                 const float* beta, int silu, void* out, int ldo, void* stream);
/* GroupNorm(+SiLU) in one call (what the engines use): statistics + normalise — ONE launch (a workgroup per (group, unit), the group's
 * slice of the unit in registers, ws untouched) where a group has a multiple of 8 channels and rows_per_unit * channels-per-group / 8
 * <= 4096 and no prefetch hint is given; else 2 launches for tensors with few row slabs, 3 otherwise.
 * ws: t2v_group_norm_ws_floats(n_units, rows_per_unit, groups, c0 + c1) floats.
 * prefetch / prefetch_bytes (NULL / 0 = off): a buffer the NEXT launch will stream — the weights of the conv that follows every
 * GroupNorm of the UNet — touched with streaming loads by the normalise pass so that it sits in the 256 MB Infinity Cache when
 * that launch starts (a UNet step walks 2.8 GB of weights: nothing survives from the previous step).  Hint only. */
long long t2v_group_norm_ws_floats(int n_units, int rows_per_unit, int groups, int channels);
int t2v_group_norm(const void* x0, int c0, int ld0, const void* x1, int c1, int ld1, int n_units, int rows_per_unit,
                   int groups, float eps, const float* gamma, const float* beta, int silu, float* ws, void* out, int ldo,
                   const void* prefetch, long long prefetch_bytes, void* stream);

/* GroupNorm(+SiLU) whose statistics pass reads the column statistics the producing t2v_gemm launches wrote
 * (t2v_gemm_desc::colstat_out) instead of the tensor: cs0 [rows/32][c0][2] for x0, cs1 [rows/32][c1][2] for the second part of
 * a virtual concat (NULL without one, required with c1 > 0); rows_per_unit % 32 == 0, cs0 / cs1 8-byte aligned, ldo >= c0 + c1 (all
 * checked: T2V_ESHAPE).  Two launches; ws: t2v_group_norm_cs_ws_floats(...) floats.
 * Same result as t2v_group_norm up to the summation order of the statistics (fixed: deterministic).  The statistics launch has two
 * forms, chosen by shape: one block per (group, unit) that leaves the per-channel affine (rstd gamma, beta - mean rstd gamma) in ws and
 * an apply pass that streams with it (even channels per group, at most 512 of them — 1 024 threads per block above 256 —, c0 even,
 * cs0 / cs1 16-byte aligned, 2 (c0 + c1) <= the ws floats per unit, at most 32 slabs per thread, and not fewer than 16 channels per
 * group where the statistics exceed 8 MB), or per-slab-block partial sums that every block of the apply pass finishes for itself. */
long long t2v_group_norm_cs_ws_floats(int n_units, int rows_per_unit, int groups);
int t2v_group_norm_cs(const float* cs0, const float* cs1, const void* x0, int c0, int ld0, const void* x1, int c1, int ld1,
                      int n_units, int rows_per_unit, int groups, float eps, const float* gamma, const float* beta, int silu,
                      float* ws, void* out, int ldo, const void* prefetch, long long prefetch_bytes, void* stream);
/* (mean, rstd) per (unit, group) — the `stats` of t2v_gn_stats — from the column statistics alone: the training engine keeps them
 * for the GroupNorm backward and normalises with t2v_gn_apply (openaimodel3d.py:223-254 under autograd).  cs1 / c1: second part of
 * a virtual concat (NULL / 0: none).  ws: t2v_group_norm_cs_ws_floats floats.  rows_per_unit % 32 == 0, c0 + c1 <= 4096 and a
 * multiple of groups, cs0 / cs1 8-byte aligned (T2V_ESHAPE otherwise); the same two statistics forms as t2v_group_norm_cs. */
int t2v_gn_stats_cs(const float* cs0, int c0, const float* cs1, int c1, int n_units, int rows_per_unit, int groups, float eps,
                    float* ws, float* stats, void* stream);

/* LayerNorm over the channel dim, eps, affine; bf16 in/out (attention.py:279-281).  C % 8 == 0, ldx, ldo multiples of 8 and >= C. */
int t2v_layernorm(const void* x, int ldx, int M, int C, const float* gamma, const float* beta,
                  float eps, void* out, int ldo, void* stream);

/* row softmax in place on bf16 [rows][ld]: cols [0,n) normalised, cols [n, n_pad) set to 0
 * (score matrix of the GEMM-formulated attention: attention.py:143, ae_modules.py:61).  n_pad % 8 == 0, n_pad <= ld, ld % 8 == 0.
 * Columns [n, n_pad) are loaded but their values are never used (any bit pattern, NaN included); columns [n_pad, ld) are neither
 * read nor written. */
int t2v_softmax_rows(void* s, long long rows, int n, int n_pad, int ld, void* stream);

/* ---------------------------------------------------------------- attention
 * Fused spatial attention (flash style), head dim 64: softmax(Q K^T * scale) V per (image, head).
 * q: bf16 rows (img*seq_q + i), head h at columns [h*64, h*64+64); k likewise over seq_kv rows;
 * vt: V transposed per image: bf16 [img_kv][heads*64][ld_vt] (keys contiguous); vt_img_stride = elements
 * between consecutive kv images (0 = heads*64*ld_vt; larger when several layers' V^T share one buffer).
 * ld_vt >= seq_kv rounded up to 64; the padding columns up to that multiple of 64 are read (their probability is exactly 0) and
 * must hold finite values; columns beyond it, and the space between two images when vt_img_stride > heads*64*ld_vt, are not read.
 * K rows past seq_kv are not read (the tail of the last key tile comes from the library's zero page).  ldq, ldk % 8 == 0, ldo % 4 == 0,
 * all >= heads*64.  The probabilities enter the P V product rounded to bf16 (fp32 accumulation).
 * kv image of q image b is b / kv_div (text cross-attention shares K/V across the frames of a clip).
 * Replaces CrossAttention.forward / efficient_forward (attention.py:102-164,166-240 = xformers
 * memory_efficient_attention). */
int t2v_attn_spatial(const void* q, int ldq, const void* k, int ldk, const void* vt, int ld_vt,
                     long long vt_img_stride, void* out, int ldo, int n_img, int seq_q, int seq_kv,
                     int heads, int kv_div, float scale, void* stream);

/* The same kernel for spatial SELF-attention (seq_q == seq_kv == seq, kv_div == 1) with V in its token rows: q, k and v are bf16 rows
 * (img*seq + i), head h at columns [h*64, h*64+64) — typically three column ranges of one q|k|v Linear's output.  The V tile goes
 * to LDS row-major and is consumed through the transposing LDS read of gfx950; rows past seq of the last key tile come from the
 * library's zero page for K and V alike, so no operand is padded or zero-filled and nothing outside the n_img*seq rows and the
 * heads*64 columns of each operand is read.  The products are summed in the order of t2v_attn_spatial: for equal operands the two
 * entry points give bit-identical outputs.  ldq, ldk, ldv % 8 == 0, ldo % 4 == 0, all >= heads*64. */
int t2v_attn_spatial_rm(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                        int n_img, int seq, int heads, float scale, void* stream);

/* Temporal self-attention, head dim 64, sequence = frames: for every (clip b, pixel p, head h)
 * softmax(Q K^T * scale) V over the F frames, reading rows ((b*F+f)*HW + p) directly from the
 * token-major q/k/v (no '(b h w) t c' rearrange copies, attention.py:475-511,102-164).
 * probs (optional, fp32 [(b*HW+p)*heads+h][F][F]) = CrossAttention.attention_probs
 * (attention.py:124-126).  Row strides: multiples of 8, >= heads*64; only the heads*64 columns of a row are read / written. */
int t2v_attn_temporal(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                      void* out, int ldo, int n_clips, int frames, int hw, int heads, float scale,
                      float* probs, void* stream);

/* ---------------------------------------------------------------- layout / elementwise
 * (b,c,f,h,w) tensor of dtype `dt` <-> token-major bf16/fp32 rows (openaimodel3d.py:714,739). */
int t2v_ncfhw_to_tokens(const void* x, int dt, int b, int c, int f, int hw, void* out, int ldo,
                        void* stream);
int t2v_tokens_to_ncfhw(const void* tok, int tok_f32, int ld, int b, int c, int f, int hw,
                        void* out, int dt, void* stream);
/* sinusoidal embedding cos||sin of t (int64) -> bf16 [n][dim] (utils_diffusion.py:8-32);
 * flip_sin_cos=1, scale: sin||cos of t*scale with the (half-1) divisor = guidance embedding
 * (pipeline/t2v_turbo_vc2_pipeline.py:99-120) taking fp32 t. */
int t2v_timestep_embedding(const void* t, int t_is_f32, int n, int dim, int guidance_style,
                           void* out_bf16, void* stream);
int t2v_silu(const void* x, void* out, long long n, void* stream); /* bf16 -> bf16 */
/* stream-ordered memset(0) of a caller buffer (padding columns of the GEMM-formulated attention) */
int t2v_fill_zero(void* p, long long nbytes, void* stream);
int t2v_cast(const void* x, int dt_in, void* out, int dt_out, long long n, void* stream);
/* out = ca[b]*x + cb[b]*y + cc[b]*z over (b, inner) fp32 tensors; y/z may be NULL. Host coefficient
 * arrays of length nb (<= 64).  The scheduler / consistency-distillation elementwise family
 * (t2v_turbo_scheduler.py:437-462,470-495; utils/common_utils.py:87-133; ode_solver/ddim_solver.py:67-97). */
int t2v_lincomb3(const float* x, const float* y, const float* z, const float* ca, const float* cb,
                 const float* cc, int nb, long long inner, float* out, void* stream);
/* fused LCM step: x0=(x-sb_t*eps)/sa_t; den=c_out*x0+c_skip*x; prev=sa_p*den+sb_p*noise
 * (t2v_turbo_scheduler.py:437-462). eps may be bf16 or fp32; x/noise/prev/den fp32. */
int t2v_lcm_step(const float* x, const void* eps, int eps_dt, const float* noise, float sa_t,
                 float sb_t, float c_skip, float c_out, float sa_p, float sb_p, long long n,
                 float* prev, float* denoised, void* stream);
/* Decoded video -> frames: x (B,3,T,H,W) contiguous, fp32 / bf16 / fp16 (what decode_first_stage_2DAE returns) -> out (B,T,H,W,3)
 * uint8, one launch: the tail every entry point of the reference runs as clamp / +1 / /2 / *255 / to(uint8) / permute
 * (predict.py:129-137, app.py, motion_prior_sample.py:299-301).  Per element: the stored value converted to fp32, NaN -> 0, otherwise
 * y = clamp(v, -1, 1); ((y + 1) * 0.5) * 255 with every operation rounded to fp32 on its own (explicit round-to-nearest adds and
 * multiplies, nothing contracted), truncated toward zero.  That is ((v.float().clamp(-1, 1) + 1.0) / 2.0 * 255).to(torch.uint8) bit for
 * bit, so equality is the bound.  The reference script does the same arithmetic in the tensor's own half precision; in fp32 on the same
 * stored values every intermediate is rounded no more coarsely, so the result is never further from the exact value.
 * A lane takes four consecutive pixels of one frame from the three channel planes and writes their twelve contiguous bytes;
 * neighbouring lanes write neighbouring bytes.  Lanes whose addresses are off their 4-pixel boundaries (an unaligned base, H * W
 * not a multiple of 4) and the last pixels of such a frame move element by element.
 * Refused before any launch: null pointers, non-positive sizes: T2V_EINVAL; a dtype code outside the above, x off its element
 * boundary, more than 2^31 workgroups: T2V_ESHAPE. */
int t2v_video_to_u8(const void* x, int dt, int B, int T, int H, int W, void* out, void* stream);

/* ---------------------------------------------------------------- diagnostics (tools/ only)
 * Ablation bits for tools/gemm_one.py and tools/attn_one.py.  They only act in libraries built with
 * -DT2V_GEMM_ABLATE / -DT2V_ATTN_ABLATE (runtime branches inside the K / KV loops cost ~20 %, so the product build
 * compiles them out and these calls just store the value). */
int t2v_gemm_debug(int bits);
int t2v_attn_debug(int bits);
/* t2v_group_norm has a ONE-launch form (registers hold the tensor, per-unit inter-workgroup barrier) for tensors that fit:
 * t2v_gn_coop_enable(1) / environment T2V_GN_COOP=1 selects it (default off: measured slower than the three-launch form on
 * MI355X for cache-resident tensors); t2v_gn_coop_error() returns 1 if a
 * barrier of the one-launch form ever timed out on the current device (workgroups not co-resident), -1 on a HIP error. */
int t2v_gn_coop_enable(int on);
int t2v_gn_coop_error(void);

/* ---------------------------------------------------------------- backward (dX) pieces of the VAE decoder
 * Reward-gradient branch (train_t2v_turbo_v1_lora.py:1047-1098: autograd through vae.decode, ae_modules.py:602-641).
 * Conv / linear data gradients are t2v_gemm launches on re-packed weights; these are the non-GEMM parts.
 * t2v_gn_bwd: dx = d/dx [act(GroupNorm(x))] . dy (+ resid), act = SiLU or identity; stats = (mean, rstd) per
 *   (unit, group) from t2v_gn_stats of the forward; ws: t2v_gn_bwd_ws_floats() floats.  x, dy, resid, dx bf16.
 * t2v_softmax_bwd_rows: dp <- p * (dp - sum_j p_j dp_j) per row (columns [n, n_pad) set to 0; their p / dp inputs are loaded but never
 *   used: any bit pattern; columns [n_pad, ld) neither read nor written).
 * t2v_transpose_bf16: out[b][c][r] = in[b][r][c].   t2v_sumpool2x2: adjoint of nearest-x2 upsampling (token-major). */
long long t2v_gn_bwd_ws_floats(int n_units, int rows_per_unit, int groups);
int t2v_gn_bwd(const void* x, int ldx, int C, int n_units, int rows_per_unit, int groups, const float* stats,
               const float* gamma, const float* beta, int silu, const void* dy, int ldy, const void* resid, int ldr,
               float* ws, void* dx, int ldo, void* stream);
int t2v_softmax_bwd_rows(const void* p, void* dp, long long rows, int n, int n_pad, int ld, void* stream);
int t2v_transpose_bf16(const void* in, int ld_in, int rows, int cols, void* out, int ld_out, int batch,
                       long long in_stride, long long out_stride, void* stream);
int t2v_sumpool2x2(const void* in, int n_img, int h, int w, int C, void* out, void* stream);

/* ---------------------------------------------------------------- backward (dX) pieces of the UNet
 * d(loss)/d(latents) through UNetModel.forward (openaimodel3d.py:672-740) for losses on the output and on the recorded
 * temporal attention probabilities: motion_prior_sample.py:59-84 (autograd.grad(loss, latents)) and the data half of the
 * student's backward (train_t2v_turbo_v1_lora.py:1190).  Convolution / linear / spatial-attention gradients are t2v_gemm
 * launches; these are the rest.  STATUS: written after the round's GPU budget was spent - the engine's dataflow is verified on
 * CPU against autograd with an emulation of exactly these semantics, and on MI355X against the emulation and autograd (tests/test_gpu_unet_grad.py).
 * t2v_gn_bwd2: t2v_gn_bwd over a virtual channel concat [x0 | x1] (the skip connections), up to 4096 channels.
 * t2v_layernorm_bwd: dx = d/dx LayerNorm(x) . dy (+ resid); statistics recomputed per row (attention.py:279-281).
 * t2v_geglu_fwd / _bwd: h = packed pre-activation [M][2*inner] in 64-column groups [32 value | 32 gate] (the layout
 *   T2V_ACT_GEGLU consumes); out = value * gelu(gate); dh in the same packed layout (attention.py:516-523).
 * t2v_scatter2x: out[n][2y][2x] = src[n][y][x], zero elsewhere, H in {2h-1, 2h}: the gradient of a 3x3 s2 p1 conv is the
 *   flipped 3x3 s1 p1 conv over this (openaimodel3d.py:63-72).
 * t2v_add_bf16: out = a + b over [M][C] with row strides (gradient fan-in at the skip connections).
 * t2v_attn_temporal_bwd: (dq, dk, dv) of t2v_attn_temporal from d(out) and, optionally, d(probs)
 *   (fp32 [(b*HW+p)*heads+h][F][F], the layout of the forward's probs output); frames <= 16; input row strides % 8, gradient row
 *   strides % 4, all >= heads*64; P and dS enter the MFMAs rounded to bf16.
 * Every row stride of this section must be >= the row's width (checked). */
int t2v_gn_bwd2(const void* x0, int c0, int ld0, const void* x1, int c1, int ld1, int n_units, int rows_per_unit, int groups,
                const float* stats, const float* gamma, const float* beta, int silu, const void* dy, int ldy, const void* resid,
                int ldr, float* ws, void* dx, int ldo, void* stream);
int t2v_layernorm_bwd(const void* x, int ldx, int M, int C, const float* gamma, float eps, const void* dy, int ldy,
                      const void* resid, int ldr, void* dx, int ldo, void* stream);
int t2v_geglu_fwd(const void* h, int ldh, long long M, int inner, void* out, int ldo, void* stream);
int t2v_geglu_bwd(const void* h, int ldh, const void* dy, int ldy, long long M, int inner, void* dh, int ldd, void* stream);
int t2v_scatter2x(const void* src, int n_img, int h, int w, int C, int H, int W, void* out, void* stream);
int t2v_add_bf16(const void* a, int lda, const void* b, int ldb, void* out, int ldo, long long M, int C, void* stream);
int t2v_attn_temporal_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* dout, int ldo,
                          const float* dprobs, void* dq, int ldq2, void* dk, int ldk2, void* dv, int ldv2, int n_clips, int frames,
                          int hw, int heads, float scale, void* stream);

/* ---------------------------------------------------------------- motion-prior loss on the recorded probabilities
 * The loss between the temporal attention probabilities of two forwards (utils/common_utils.py:446-478: sort, scatter, boolean
 * gather, MSE) and its gradient w.r.t. the differentiated ones, for every recorded layer in ONE launch pair.
 * Per problem (layer) p with rows_p rows of n values: an entry is SELECTED when fewer than rank_k entries of its row beat it, where
 * "beat" is a larger ref, or an equal ref at a higher index (the last rank_k places of a stable ascending sort);
 *   loss[p] = sum over the selected entries of (gen - ref)^2 / (rows_p * rank_k)
 *   d_gen   = alpha * 2 / (rows_p * rank_k) * (gen - ref) on the selected entries, 0 elsewhere (every element is written).
 * 1 <= n <= 64, 1 <= rank_k <= n (T2V_ESHAPE), 1 <= n_problems <= T2V_RANK_LOSS_MAX (T2V_EINVAL).  ws: one float per workgroup,
 * ws_floats >= sum over p of ceil(rows_p / (T2V_RANK_LOSS_WG_LANES / nh)), nh = the power of two >= n (T2V_ESHAPE below that).
 * The sums are taken in a fixed order (per-workgroup partials, then one small launch): same inputs, same bits. */
#define T2V_RANK_LOSS_MAX 16
#define T2V_RANK_LOSS_WG_LANES 2048
typedef struct t2v_rank_loss_problem {
    const float* ref;   /* [rows, n] contiguous: reference probabilities                    */
    const float* gen;   /* [rows, n] contiguous                                             */
    float* d_gen;       /* [rows, n] out, EVERY element written (zeros where not selected)  */
    long long rows;
} t2v_rank_loss_problem;
int t2v_rank_loss(const t2v_rank_loss_problem* p, int n_problems, int n, int rank_k, float alpha, float* ws, long long ws_floats,
                  float* loss /* [n_problems] */, void* stream);

/* ---------------------------------------------------------------- optimizer / EMA over flat fp32 buffers
 * Replace bitsandbytes AdamW8bit / torch AdamW on the LoRA tensors (train_t2v_turbo_v1_lora.py:765-803),
 * accelerator.clip_grad_norm_ (:1193) and update_ema (utils/common_utils.py:307-319).
 * t2v_adamw_step: decoupled weight decay, bias-corrected (torch.optim.AdamW semantics); grad_scale multiplies
 * the gradient first (fold the clip coefficient in).  t2v_sumsq: out[0] = sum(x^2), deterministic two-pass;
 * ws = workspace of >= 1024 floats. */
int t2v_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                   void* stream);
int t2v_ema_update(float* target, const float* src, float rate, long long n, void* stream);
int t2v_sumsq(const float* x, long long n, float* ws, float* out, void* stream);

/* ---------------------------------------------------------------- block-wise 8-bit AdamW (optim.AdamW8bit; Dettmers et al. 2021)
 * The two moments of every parameter tensor are stored as one byte per element — an index into a 256-entry fp32 code book of values
 * in [-1, 1] (first moment) / [0, 1] (second moment) — plus one fp32 absmax per QUANTISATION BLOCK of 256 consecutive elements of
 * ONE tensor: value = code[byte] * absmax[block].  Each tensor's state is padded up to whole blocks (no block straddles two
 * tensors); the padding bytes of a last, partial block hold the code of 0 and take no part in the block's absmax.
 *
 * t2v_adamw8_step updates MANY tensors in one launch.  `table` is a DEVICE array of n_tensors descriptors, one per tensor that
 * has a gradient this step, ordered by work0: the launch covers work blocks [0, n_blocks), tensor i owning
 * [work0, work0 + ceil(n / 256)).  Parameters and gradients are contiguous fp32 anywhere in memory; a tensor whose param or grad
 * pointer is not 16-byte aligned is read and written with scalar accesses (chosen in the kernel: views into gradient buckets may
 * be 4-byte aligned), the arenas must be 16-byte aligned.  Flag T2V_ADAMW8_F32_STATE: the tensor keeps fp32 moments (small
 * tensors), at state_block * 256 floats into state1_f32 / state2_f32; otherwise its codes are at state_block * 256 bytes into
 * state1 / state2 and its absmax at absmax1 / absmax2 [state_block ...].  An arena that no tensor of the table uses may be NULL.
 * Arithmetic: torch.optim.AdamW (decoupled decay, bias correction by `step`), in the operation order of t2v_adamw_step; the
 * parameter is updated from the fresh fp32 moments, which are then re-quantised to the nearest code (ties to the lower code).
 * code1 / code2: 256 strictly increasing floats each.
 * t2v_quant8_blockwise / t2v_dequant8_blockwise: fp32 <-> codes (ceil(n / 256) * 256 bytes) + absmax (ceil(n / 256) floats). */
#define T2V_ADAMW8_BLOCK 256
#define T2V_ADAMW8_F32_STATE 1
typedef struct t2v_adamw8_tensor {
    float* param;
    const float* grad;
    long long state_block; /* first block of this tensor's state in the 8-bit (or, with F32_STATE, the fp32) arenas */
    long long n;           /* elements */
    long long work0;       /* first work block of this tensor in this launch */
    float lr;
    float weight_decay;
    int flags;
    int reserved;
} t2v_adamw8_tensor;
int t2v_adamw8_step(const t2v_adamw8_tensor* table, int n_tensors, long long n_blocks, unsigned char* state1,
                    unsigned char* state2, float* absmax1, float* absmax2, float* state1_f32, float* state2_f32,
                    const float* code1, const float* code2, float beta1, float beta2, float eps, int step,
                    float grad_scale, void* stream);
int t2v_quant8_blockwise(const float* x, long long n, const float* code, unsigned char* codes, float* absmax,
                         void* stream);
int t2v_dequant8_blockwise(const unsigned char* codes, const float* absmax, const float* code, float* out, long long n,
                           void* stream);

/* ---------------------------------------------------------------- EMA of many tensors in one launch (optim.update_ema)
 * The target network of train_latent_t2v_turbo_v2.py --use_target_unet (:1272-1276) follows the student by update_ema
 * (utils/common_utils.py:307-319): targ.mul_(rate).add_(src.to(targ.dtype), alpha = 1 - rate) over every parameter pair, ~ 3 000
 * small launches.  t2v_ema_multi updates MANY tensors in one launch, where they are.  `table` is a DEVICE array of n_tensors
 * descriptors ordered by work0 (8-byte aligned): the launch covers work blocks [0, n_blocks), tensor i owning
 * [work0, work0 + ceil(n / T2V_EMA_BLOCK)); a work block that no tensor owns touches nothing.  Targets are contiguous fp32, sources
 * contiguous fp32 or bf16 (widened first, exactly).  A tensor whose target and source are both 16-byte aligned moves in 16-byte
 * accesses, any other one in scalar accesses (chosen in the kernel, per tensor: parameters may be 4-byte-aligned views); tails are
 * handled per element and nothing outside [target, target + n) is written.  Arithmetic: per element t = t * rate + s * (1.0f - rate),
 * the expression of t2v_ema_update: on one build both give the same bits for the same data.
 * T2V_EINVAL: NULL table, n_tensors <= 0, n_blocks <= 0. */
#define T2V_EMA_BLOCK 4096
typedef struct t2v_ema_tensor {
    float* target;        /* fp32, contiguous, updated in place */
    const void* src;      /* contiguous, same element count */
    long long n;          /* elements */
    long long work0;      /* first work block of this tensor in this launch */
    int src_dt;           /* T2V_F32 or T2V_BF16 (the reference's src.to(targ.dtype)) */
    int reserved;
} t2v_ema_tensor;
int t2v_ema_multi(const t2v_ema_tensor* table /* device */, int n_tensors, long long n_blocks, float rate, void* stream);

/* ---------------------------------------------------------------- fp32 AdamW and gradient clipping of many tensors where they are
 * (optim.AdamW, optim.clip_grad_norm_): the trainers' default optimizer side, torch.optim.AdamW over per-tensor parameters
 * (train_latent_t2v_turbo_v2.py:787-845) after accelerator.clip_grad_norm_ (:1265-1268).  All three entry points walk ONE table: a
 * DEVICE array of n_tensors descriptors ordered by work0 (8-byte aligned).  The launch covers work blocks [0, n_blocks), tensor i
 * owning [work0, work0 + ceil(n / T2V_ADAMW_BLOCK)); a work block that no tensor owns touches nothing.  param, grad, exp_avg and
 * exp_avg_sq are contiguous fp32 anywhere in memory.  Access width is chosen per tensor in the kernel: 16-byte accesses when every
 * pointer the entry point uses is 16-byte aligned (t2v_adamw_multi: all four; the other two: grad), scalar accesses otherwise; tails
 * are handled per element and nothing outside [ptr, ptr + n) is read or written.
 *
 * t2v_adamw_multi: `hyper` is a HOST array of n_hyper <= T2V_ADAMW_MAX_HYPER rows, handed to the kernel by value (a moving learning
 * rate costs no upload; the device table changes only when a pointer does); a tensor's `hyper` field is its row (a tensor whose row
 * is outside [0, n_hyper) is not touched).  The bias corrections are formed here, as in t2v_adamw8_step:
 * bc1 = 1.0f - powf(beta1, (float)step), sqrtf(1.0f - powf(beta2, (float)step)).  Per element, every product and sum rounded on its
 * own (no contraction), the order of the fp32-state branch of t2v_adamw8_step, whose bits it reproduces on one build:
 *     gr = g * scale;  p *= 1 - lr * wd;  m = b1 * m + (1 - b1) * gr;  v = b2 * v + (1 - b2) * gr * gr;
 *     p -= (lr / bc1) * m / (sqrtf(v) / bc2_sqrt + eps)
 * with scale = grad_scale * (grad_scale_dev ? *grad_scale_dev : 1.0f): grad_scale_dev is a DEVICE scalar (the clip coefficient that
 * t2v_sumsq_multi left there) or NULL.  T2V_EINVAL: NULL table or hyper, n_tensors <= 0, n_blocks < n_tensors, n_hyper outside
 * 1..T2V_ADAMW_MAX_HYPER, a step < 1.  T2V_ESHAPE: a table that is not 8-byte aligned.
 *
 * t2v_sumsq_multi reads grad, n and work0 only.  Every work block writes one fp32 partial to ws[block] (ws: n_blocks floats; 0 for a
 * block no tensor owns); a finishing launch adds the partials in a fixed order, in double, and writes out[0] = sqrt(sum) and
 * out[1] = max_norm > 0 ? min(1, max_norm / (out[0] + 1e-6f)) : 1 — the coefficient of torch.nn.utils.clip_grad_norm_; a NaN norm
 * gives a NaN coefficient, as torch.clamp does.  Deterministic: the same data gives the same bits.
 * t2v_scale_multi: grad *= *coef_dev in place over the table; a workgroup that reads exactly 1.0f returns without touching gradient
 * memory (bitwise the same result). */
#define T2V_ADAMW_BLOCK 4096
#define T2V_ADAMW_MAX_HYPER 16
typedef struct t2v_adamw_tensor {
    float* param;
    float* grad;           /* read by t2v_adamw_multi and t2v_sumsq_multi, scaled in place by t2v_scale_multi */
    float* exp_avg;
    float* exp_avg_sq;
    long long n;           /* elements */
    long long work0;       /* first work block of this tensor in this launch */
    int hyper;             /* row of the launch's t2v_adamw_hyper array */
    int reserved;
} t2v_adamw_tensor;
typedef struct t2v_adamw_hyper {
    float lr;
    float weight_decay;
    float beta1;
    float beta2;
    float eps;
    int step;              /* >= 1: the step being taken (bias correction) */
} t2v_adamw_hyper;
int t2v_adamw_multi(const t2v_adamw_tensor* table /* device */, int n_tensors, long long n_blocks, const t2v_adamw_hyper* hyper /* host */,
                    int n_hyper, float grad_scale, const float* grad_scale_dev, void* stream);
int t2v_sumsq_multi(const t2v_adamw_tensor* table /* device */, int n_tensors, long long n_blocks, float* ws, float max_norm, float* out,
                    void* stream);
int t2v_scale_multi(const t2v_adamw_tensor* table /* device */, int n_tensors, long long n_blocks, const float* coef_dev, void* stream);

/* ---------------------------------------------------------------- LoRA training path (utils/lora.py:45-50,124-129,204-209)
 * t2v_gather_f32: indexed re-layout of fp32 data.  accumulate = 0: out[i] = idx[i] >= 0 ? alpha*src[idx[i]] : 0;
 * accumulate = 1: out[i] += alpha*src[idx[i]] where idx[i] >= 0.  out is fp32 (T2V_F32) or bf16 (T2V_BF16).
 * One launch packs every lora_down / lora_up tensor (flat fp32 parameters) into the bf16 GEMM operand layouts, and one
 * launch scatters every LoRA weight gradient from the GEMM output layout into the flat gradient buffer the
 * all-reduce and the optimizer work on (what autograd's AccumulateGrad does per tensor in the reference,
 * train_t2v_turbo_v1_lora.py:1190). */
int t2v_gather_f32(const float* src, const int* idx, float alpha, void* out, int dt_out, int accumulate, long long n,
                   void* stream);
/* t2v_attn_spatial_bwd: flash-style backward of the spatial SELF-attention (head dim 64): dQ, dK, dV from token-major Q / K / V /
 * dO and the forward's O, the [queries x keys] probabilities recomputed tile by tile (never written to memory).  Two launches:
 * per query block (statistics L = log2-sum-exp and D = sum_c dO O into l2 / dsum, then dQ), per key block (dK, dV).
 * q, k, dout, o, dq, dk, dv: bf16 [n_img*seq][ld], head h at column 64 h.  v: bf16, row r of (img, head) at
 * v + img*v_img_stride + head*v_head_stride + r*ldv (token-major buffer or the per-head [keys][64] transpose of V^T).
 * kt, qt, dot: K^T, Q^T, dO^T per image, [n_img][heads*64][ld] with the sequence zero-padded to a multiple of 64
 * (t2v_transpose_pad_bf16): the padding columns up to that multiple of 64 ARE read and must be zero, columns beyond it are not read.
 * V rows r >= seq_kv (the padding rows of the per-head layout) and K / Q / dO rows past the sequence are not read (zero page).
 * l2, dsum: fp32 workspaces [n_img*heads][ld_stat], ld_stat >= seq_q; only columns [0, seq_q) are written.
 * D is computed from the bf16 O the caller passes; P and dS enter the MFMAs rounded to bf16.  seq_q != seq_kv is supported (K / V / kt /
 * dk / dv over seq_kv rows per image, the rest over seq_q).  Strides: ldq, ldk, ldv, ld_kt, ld_qt, ldo, ldoo % 8, lddq, lddk, lddv % 4,
 * token-major strides >= heads*64, ldv >= 64, ld_kt >= roundup(seq_kv, 64), ld_qt >= roundup(seq_q, 64) (checked).
 * Replaces the autograd backward of CrossAttention.forward for attn1 of the spatial transformers (attention.py:102-164). */
int t2v_attn_spatial_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, long long v_img_stride,
                         long long v_head_stride, const void* kt, int ld_kt, const void* qt, const void* dot, int ld_qt,
                         const void* dout, int ldo, const void* o, int ldoo, float* l2, float* dsum, int ld_stat, void* dq, int lddq,
                         void* dk, int lddk, void* dv, int lddv, int n_img, int seq_q, int seq_kv, int heads, float scale,
                         void* stream);
/* t2v_wgrad_tn: out[R][C] (fp32, row stride ldo) = alpha * a[:, :R]^T b[:, :C] for two TOKEN-MAJOR bf16 operands a [M][lda],
 * b [M][ldb] — the token-contracted LoRA weight gradients (dU = s dy^T t, dD = G^T x) and per-clip column sums without transposed
 * operand copies, and the base-weight gradients of full fine-tuning (dW = dy^T x, dy^T xcol).  The token range is split over
 * workgroups (splits = 0: library choice); fp32 partial tiles go through the caller's workspace ws (>= splits*R*C*4 bytes, the split
 * count shrinks to fit) and are added in a fixed order.  With ONE split — a product with enough output tiles to fill the chip, or an
 * output larger than the workspace — the tiles are written to `out` directly and ws is not touched.  Output tile 64 x 64, or
 * 128 x 128 where both extents reach 128 and pad to multiples of 128 within 10 % (T2V_WGRAD_TILE128=0: always 64 x 64).
 * lda >= R, ldb >= C, ldo >= C (checked; lda, ldb % 8 == 0 and a, b 16-byte aligned, out 4-byte aligned at any ldo).  Only rows [0, M) and
 * columns [0, R) / [0, C) of the operands are read — the kernel contracts over tokens, so a row past M would reach every output — only
 * columns [0, C) of out rows [0, R) and the first splits * R * C floats of ws are written; fp32 accumulation, alpha applied in fp32, a
 * fixed summation order (two launches with the same arguments give the same bits).  The same holds per problem of t2v_wgrad_tn_group. */
int t2v_wgrad_tn(const void* a, int lda, const void* b, int ldb, long long M, int R, int C, float alpha, float* out, int ldo, float* ws,
                 long long ws_bytes, int splits, void* stream);
/* t2v_wgrad_tn_group: up to T2V_WGRAD_GROUP_MAX such products in one launch pair (main + fixed-order reduce): the weight gradients
 * of ONE LoRA group — dU of each of its leaves and dD (utils/lora.py:45-50 under autograd) — whose operands all exist once the
 * rank-r gradient is there.  Same arithmetic and summation structure per product as t2v_wgrad_tn; the token splits are chosen for
 * the group as a whole.  ws: fp32 workspace for the partial slabs of all products. */
#define T2V_WGRAD_GROUP_MAX 8
typedef struct t2v_wgrad_problem {
    const void* a;      /* bf16 [M][lda], columns [0, R) */
    const void* b;      /* bf16 [M][ldb], columns [0, C) */
    float* out;         /* fp32 [R][ldo] = alpha * a^T b */
    long long M;
    int lda, ldb, ldo, R, C;
    float alpha;
} t2v_wgrad_problem;
int t2v_wgrad_tn_group(const t2v_wgrad_problem* problems, int n, float* ws, long long ws_bytes, void* stream);
/* t2v_gn_coef_cs: the per-channel affine of a GroupNorm alone, from the producers' column statistics (t2v_gemm_desc::colstat_out layout,
 * one array per part of a virtual concat): coef fp32 [n_units][2][c0 + c1] — for consumers that normalise in their own load phase
 * (t2v_gemm_desc::gn_coef).  t2v_gn_coef_cs_supported: 1 where the direct statistics form of t2v_group_norm_cs takes the shape and the
 * pointers (up to 512 channels per group), 0 otherwise (else t2v_group_norm_cs, which writes the normalised tensor); t2v_gn_coef_cs
 * refuses a shape whose answer is 0 with T2V_ESHAPE. */
int t2v_gn_coef_cs_supported(const float* cs0, int c0, const float* cs1, int c1, int n_units, int rows_per_unit, int groups);
int t2v_gn_coef_cs(const float* cs0, int c0, const float* cs1, int c1, int n_units, int rows_per_unit, int groups, float eps,
                   const float* gamma, const float* beta, float* coef, void* stream);
/* ---- base-weight gradients for FULL fine-tuning (csrc/full_grad.hip; train_latent_t2v_turbo_v2.py:798-816,1262) ----------------------
 * t2v_im2col_bf16: the shifted-row matrix of a conv leaf in the K order of the forward's tap-major pack,
 *     out[m][tap * C + c] = x[src(m, tap)][c]   (0 outside the grid; x = virtual concat [x0 | x1], C = c0 + c1, channels % 8 == 0)
 * for mode = T2V_GEMM_CONV3X3 / _S2 / _S2_PAD01 / _UP2 (9 taps, (ky, kx) row-major) or T2V_GEMM_TCONV3 (3 taps = frame offsets; n_img =
 * clips x frames) on the (n_img, h, w) INPUT grid; out: bf16 [t2v_im2col_rows(mode, n_img, h, w)][ldo], ldo >= taps * C.  With it the
 * weight gradient of a conv leaf, dW[n][tap][c] = sum_m dy[m][n] out[m][tap * C + c], is one t2v_wgrad_tn(dy, out) product. */
long long t2v_im2col_rows(int mode, int n_img, int h, int w);
int t2v_im2col_bf16(const void* x0, int c0, int ld0, const void* x1, int c1, int ld1, int mode, int n_img, int h, int w, int frames, void* out,
                    int ldo, void* stream);
/* t2v_norm_affine_grad: per-channel sums over token rows, `sum_rows` consecutive rows per output row u (rows % sum_rows == 0):
 *     dgamma[u][c] = sum dz[m][c] xhat[m][c],   dbeta[u][c] = sum dz[m][c]
 * kind 0: xhat from GroupNorm statistics stats[row / rows_per_unit][group][2] = (mean, rstd) of the forward (lvdm/basics.py:78-89);
 * kind 1: xhat = LayerNorm's (x - mean_row) * rstd_row, recomputed per row with ln_eps (attention.py:300-311);
 * kind 2: no norm — dbeta = plain column sums of dy (bias gradients; per-clip sums = d(loss)/d(time embedding row); c0 = columns of dy).
 * silu != 0 (kinds 0, 1): the forward applied SiLU behind the norm (openaimodel3d.py:223-254), dz = dy * silu'(xhat gamma + beta); else
 * dz = dy.  x = [x0 | x1] bf16 (the norm's INPUT), dy bf16 [rows][ldy] over the C = c0 + c1 channels (C % 8 == 0; C <= 2560 for kinds 0 / 1); dgamma /
 * dbeta fp32 with row strides ld_dgamma / ld_dbeta (either may be NULL for kind 2 / when not wanted).  ws: fp32 workspace of
 * t2v_norm_affine_grad_ws_floats(rows, sum_rows, C) floats.  Two launches, fixed summation order (no float atomics). */
long long t2v_norm_affine_grad_ws_floats(long long rows, long long sum_rows, int channels);
int t2v_norm_affine_grad(const void* x0, int c0, int ld0, const void* x1, int c1, int ld1, long long rows, long long sum_rows, int kind,
                         int rows_per_unit, int groups, const float* stats, float ln_eps, const float* gamma, const float* beta, int silu,
                         const void* dy, int ldy, float* dgamma, int ld_dgamma, float* dbeta, int ld_dbeta, float* ws, void* stream);
/* t2v_repack_conv_f32: a conv leaf's fp32 parameter w [N][C][taps] (taps = 9: (ky, kx) row-major, or 3: frame offsets; <= 9) into one of
 * the bf16 packs the launch lists read, cast (round to nearest even) included:
 *     kind 0   out[n][t * C + c] = w[n][c][t]                   the tap-major forward pack (t2v_gemm's K order), ldo >= taps * C
 *     kind 1   out[c][(taps - 1 - t) * N + n] = w[n][c][t]      the data-gradient pack: the same conv over dy with channels and filters
 *                                                               swapped and the taps mirrored, ldo >= taps * N
 * Full fine-tuning re-makes every pack per optimizer step IN PLACE (the recorded launch lists keep their pointers); this replaces
 * torch's permute / flip / cast chain for the conv leaves (70 % of the UNet's parameters).  Pure data movement: every element is the
 * round-to-nearest-even bf16 of one parameter; ldo below the pack row is refused, columns behind the pack row are not written. */
int t2v_repack_conv_f32(const float* w, int N, int C, int taps, int kind, void* out, int ldo, void* stream);
/* ---- the B-row conditioning branch of the training routes (csrc/full_grad.hip) -----------------------------------------------------
 * The time / fps / guidance MLPs (time_embed, fps_embedding, time_cond_proj, motion_cond_proj, combine_proj: openaimodel3d.py:683-706) and
 * the SiLU -> Linear emb_layers of every ResBlock (openaimodel3d.py:172-178) have M = B rows, B = clips of the batch.  Three entries run
 * their forward, data gradient and weight gradient — and, composed, the LoRA branch of an injected leaf (down -> up -> mask * scale -> add:
 * utils/lora.py:45-50) — in fp32 on the master parameters IN PLACE: no packs, nothing to refresh after an optimizer step.  They replace the
 * F.linear / F.silu calls of those lines and their autograd nodes.
 * Shared conventions: 1 <= B <= T2V_ROWLIN_MAX_ROWS rows; activations and gradients fp32 [B][ld]; weights [N][ldw] fp32, or bf16 with
 * w_bf16 != 0, read with 16-byte loads where the base is 16-byte aligned and ldw a multiple of 16 bytes (element loads otherwise — same
 * sums in the same order); a TABLE of n problems per call, all of them in one launch (pair); tables of any length are taken (split into
 * launches of 24 problems inside the library).  Only rows [0, B) and columns [0, K) / [0, N) of any operand are read or written: padding
 * columns behind a row and rows past B are never touched.  fp32 accumulation in a fixed order, no float atomics: two calls with the same
 * arguments give the same bits.  SiLU and its derivative are evaluated in double and rounded once.  Refused before anything is launched:
 * a null table or operand and B outside 1..8 (T2V_EINVAL), a row stride shorter than the row (T2V_ESHAPE). */
#define T2V_ROWLIN_MAX_ROWS 8
typedef struct t2v_rowlin_problem {
    const float* x;     /* fwd, wgrad: the leaf's input [B][ldx], columns [0, K).  bwd_data: the saved pre-activation of dx (silu != 0), else unused */
    const void* w;      /* fwd, bwd_data: weights [N][ldw], columns [0, K); fp32, or bf16 if w_bf16.  wgrad: unused */
    const float* bias;  /* fwd: [N] or NULL */
    const float* res;   /* fwd: residual [B][ldr], columns [0, N), or NULL */
    float* y;           /* fwd: the output [B][ldy], columns [0, N) (written).  bwd_data, wgrad: dy, the gradient of that output (read) */
    float* dx;          /* bwd_data: the input gradient [B][ldo], columns [0, K) (written, or added to if accumulate) */
    float* dw;          /* wgrad: the weight gradient [N][ldo], columns [0, K), fp32 (written, or added to if accumulate) */
    float* db;          /* wgrad: the bias gradient [N] (as dw), or NULL */
    int K, N;           /* input / output features */
    int ldx, ldw, ldy, ldr, ldo;
    int w_bf16;         /* weights are bf16 (the reference sums use the bf16 values as they are) */
    int silu;           /* fwd, wgrad: f = SiLU on the input x (else identity).  bwd_data: g = silu'(x) on the result (else 1) */
    int accumulate;     /* bwd_data, wgrad: += into dx / dw / db */
    float alpha;        /* scale of the problem's sum: fwd y = bias + alpha sum (+ res); bwd_data: alpha_p on problem p's sum; wgrad: dw (db is not scaled) */
    int reserved;
} t2v_rowlin_problem;
/* t2v_rowlin_fwd, per problem:  y[b][n] = bias[n] + alpha sum_k f(x[b][k]) w[n][k] (+ res[b][n]).  One pass over w: a wave owns four rows, a lane the
 * 16-byte chunks l, l + 64, ... of each with B accumulators per row, then a butterfly.  f(x) of a problem waits in LDS: B * K <= 16384
 * (T2V_ESHAPE beyond).  y must not overlap x or res of the same table. */
int t2v_rowlin_fwd(const t2v_rowlin_problem* problems, int n, int B, void* stream);
/* t2v_rowlin_bwd_data:  dx[b][k] (+)= g(x[b][k]) * sum_p alpha_p sum_n dy_p[b][n] w_p[n][k], the outer sum over ALL problems of the table that name
 * the same dx (the 22 emb_layers behind one d(silu(emb)); a LoRA leaf's base weight and its down-projection): they must agree on K, ldo,
 * silu, accumulate (and x, ldx if silu), T2V_EINVAL otherwise.  The contraction runs over the weight's row index, so N is split over
 * workgroups in runs of 64 rows: partial sums [split][B][K] go to ws (t2v_rowlin_ws_floats(problems, n, B) floats, fp32; ws_floats is
 * checked) and a second launch adds them per dx — problems in table order, their splits in order — applies g and writes.  Only the first
 * t2v_rowlin_ws_floats floats of ws are written. */
long long t2v_rowlin_ws_floats(const t2v_rowlin_problem* problems, int n, int B);
int t2v_rowlin_bwd_data(const t2v_rowlin_problem* problems, int n, int B, float* ws, long long ws_floats, void* stream);
/* t2v_rowlin_wgrad:  dw[n][k] (+)= alpha sum_b dy[b][n] f(x[b][k]),  db[n] (+)= sum_b dy[b][n]  (b in order 0 .. B - 1), fp32, straight into the
 * gradient tensor the caller names (row stride ldo >= K; 16-byte stores where dw is 16-byte aligned and ldo % 4 == 0): a streaming write. */
int t2v_rowlin_wgrad(const t2v_rowlin_problem* problems, int n, int B, void* stream);
/* t2v_dropout_bf16 (below) on fp32 rows, same mask bit for bit: out[r][c] = keep(r, c) ? x[r][c] / (1 - p') : 0 (+ resid[r][c]) — the dropout of
 * the conditioning leaves' B-row LoRA branches (utils/lora.py:45-50).  ncols even, strides >= ncols (checked); in place allowed. */
int t2v_dropout_f32(const float* x, int ldx, const float* resid, int ldr, float* out, int ldo, long long rows, int ncols, float p,
                    const void* seed, unsigned site, void* stream);
/* t2v_timestep_embedding with an fp32 result [n][dim] (contiguous): the input of the fp32 conditioning branch above. */
int t2v_timestep_embedding_f32(const void* t, int t_is_f32, int n, int dim, int guidance_style, float* out, void* stream);
/* t2v_transpose_pad_bf16: out[b][c][r] = in[b][r][c] for r < rows and 0 for rows <= r < roundup(rows, 64) — the K-contiguous,
 * K-padded operand of the token-contracted weight-gradient GEMMs (dU = dy^T t, dD = G^T x) in one pass; 16-byte accesses on both
 * sides: cols % 8 == 0, ld_in % 8 == 0, ld_out % 8 == 0 and >= roundup(rows, 64), 16-byte aligned bases, batch strides % 8. */
int t2v_transpose_pad_bf16(const void* in, int ld_in, int rows, int cols, void* out, int ld_out, int batch, long long in_stride,
                           long long out_stride, void* stream);
/* t2v_dropout_bf16: out[r][c] = keep(r, c) ? x[r][c] / (1 - p') : 0  (+ resid[r][c]) over rows x ncols bf16 (ncols even), p' = ((p * 2^32) >> 16) / 65536
 * (the probability the 16-bit mask really drops with: the scale keeps E[out] = x exactly), where
 * keep is a pure function of (*seed, site, i = r * ncols + c): word = splitmix64(seed + site * 0x9E3779B97F4A7C15 + (i >> 2) *
 * 0xD1B54A32D192ED03) in 64-bit wrapping arithmetic, splitmix64 being the FINALISER alone (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9;
 * z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 — no increment of its own), element i keeps iff bits [16 (i & 3), +16) of the word >= (p * 2^32) >> 16 (p resolved to 2^-16).  The backward calls it again with the same (seed,
 * site) on the gradient.  seed: device pointer to one uint64 (a replayed launch list follows the step's seed).  In-place is
 * allowed (out == x).  ncols, ldx, ldr, ldo even, every stride >= ncols, 4-byte aligned bases (checked); only columns [0, ncols) of a row
 * are read / written; the scale and the residual add are fp32, one rounding to bf16.  Replaces nn.Dropout in LoraInjected*.forward (utils/lora.py:45-50,124-129) and TemporalConvBlock
 * (openaimodel3d.py:280-297); the random stream is not torch's (train-mode parity is statistical). */
int t2v_dropout_bf16(const void* x, int ldx, const void* resid, int ldr, void* out, int ldo, long long rows, int ncols, float p,
                     const void* seed, unsigned site, void* stream);

/* ---------------------------------------------------------------- consistency head of the v2 step (csrc/train.hip)
 * What train_latent_t2v_turbo_v2.py computes between the student's forward and its backward when no reward model is used, on
 * activations laid out [B][per_clip] (contiguous; per_clip = C * F * H * W of the latent), in three launches and a small finishing
 * one.  Per clip b with solver index i = index[b]:
 *   t_s = ddim_timesteps[i], t_e = max(t_s - topk, 0)                                   (:996-1000)
 *   alpha(t) = sqrt(alphas_cumprod[t]), sigma(t) = sqrt(1 - alphas_cumprod[t]), a_prev = ddim_alpha_cumprods_prev[i]
 *   c_skip(t) = 0.25 / (s^2 + 0.25), c_out(t) = s / sqrt(s^2 + 0.25), s = timestep_scaling * t
 *                                                        (scalings_for_boundary_conditions with sigma_data = 0.5, :1003-1015)
 * The kernels look every per-clip coefficient up themselves: the host runs no B-row op and never synchronises.  The device cannot
 * validate index without such a synchronisation: table reads are CLAMPED (index to [0, n_ddim), timesteps to [0, n_train)), so no
 * value reads out of bounds; the Python layer validates index while it is still a CPU tensor.  Coefficients are formed in double and
 * rounded to fp32 once; an element then takes two or three fp32 fused multiply-adds.
 *
 * t2v_cd_solver_step (no gradient; replaces :1169-1233 with use_scale = False, which the script asserts at :714):
 *   x0  = x0c + w (x0c - x0u),   x0c = (z - sigma(t_s) c) / alpha(t_s),   x0u likewise with u
 *   eps = c + w (c - u) - motion_gs * sqrt(1 - alpha_m) * score
 *         alpha_m = alpha(t_s) where use_motion_guide[b] != 0 and i >= motion_min_index, else 1; no such term when score is NULL.
 *         (1 - alpha)^0.5 is taken with alpha = sqrt(alphas_cumprod), as the script writes it (:1215-1226).
 *   x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps, rounded to nearest even into dt_out.
 *   z_t, cond, uncond, score: one dtype code dt_in (T2V_F32 / T2V_BF16 / T2V_F16); w, motion_gs: fp32 [B]; use_motion_guide: bytes [B].
 *
 * t2v_cd_loss_fwd (replaces :1056-1065, :1246-1260):
 *   model_pred = c_skip(t_s) z      + c_out(t_s) (z      - sigma(t_s) noise_pred)        / alpha(t_s)      -> model_pred (fp32)
 *   target     = c_skip(t_e) x_prev + c_out(t_e) (x_prev - sigma(t_e) target_noise_pred) / alpha(t_e)
 *   d = model_pred - target;  loss = mean over the N = B * per_clip elements of sqrt(d^2 + huber_c^2) - huber_c  (T2V_CD_HUBER)
 *                                                                              or of d^2                         (T2V_CD_L2)
 *   u = d loss / d model_pred = d / (N sqrt(d^2 + huber_c^2))  or  2 d / N                                       -> u (fp32)
 *   noise_pred, target_noise_pred: fp32 or bf16 (a code each); z_t, x_prev: any of the three codes (x_prev as the solver step stored it).
 *   The sum is taken in a fixed order: one partial per workgroup (T2V_CD_WG_ELEMS elements of one clip) in ws, then one launch of one
 *   workgroup adds the partials in double.  Same inputs, same bits.  ws_floats >= t2v_cd_loss_ws_floats(B, per_clip).
 *
 * t2v_cd_loss_bwd (the autograd nodes of the above):
 *   d_noise_pred = k_b (g_loss u + g_model_pred),   k_b = -c_out(t_s) sigma(t_s) / alpha(t_s)
 *   g_loss: device scalar, NULL = 1.  g_model_pred: fp32, NULL = 0 (non-NULL when a reward branch sent a gradient into model_pred).
 *   d_noise_pred: fp32 or bf16.
 *
 * Every entry point refuses before any launch: null pointers, non-positive sizes, an unknown loss type: T2V_EINVAL; a dtype code
 * outside the above, a workspace that is too small, B > T2V_CD_MAX_CLIPS (a clip is one row of the launch grid): T2V_ESHAPE.
 * 16-byte accesses when every activation pointer is 16-byte aligned (a clip that starts off a 16-byte boundary has a scalar head and
 * tail); scalar accesses otherwise. */
#define T2V_CD_WG_ELEMS 2048
#define T2V_CD_MAX_CLIPS 65535
#define T2V_CD_HUBER 0
#define T2V_CD_L2 1
typedef struct t2v_cd_sched {
    const float* alphas_cumprod;           /* [n_train] fp32, device                                   */
    const long long* ddim_timesteps;       /* [n_ddim] int64, device (DDIMSolver.ddim_timesteps)       */
    const float* ddim_alpha_cumprods_prev; /* [n_ddim] fp32, device                                    */
    const long long* index;                /* [B] int64, device: the solver index of every clip        */
    int n_train, n_ddim, topk;
    float timestep_scaling;
} t2v_cd_sched;
int t2v_cd_solver_step(const t2v_cd_sched* s, const void* z_t, const void* cond, const void* uncond, const void* score, int dt_in,
                       const float* w, const float* motion_gs, const unsigned char* use_motion_guide, int motion_min_index, void* x_prev,
                       int dt_out, int B, long long per_clip, void* stream);
long long t2v_cd_loss_ws_floats(int B, long long per_clip);
int t2v_cd_loss_fwd(const t2v_cd_sched* s, const void* noise_pred, int dt_np, const void* target_noise_pred, int dt_tnp, const void* z_t,
                    int dt_z, const void* x_prev, int dt_xp, int loss_type, float huber_c, float* model_pred, float* u, float* ws,
                    long long ws_floats, float* loss, int B, long long per_clip, void* stream);
int t2v_cd_loss_bwd(const t2v_cd_sched* s, const float* u, const float* g_loss, const float* g_model_pred, void* d_noise_pred, int dt_out,
                    int B, long long per_clip, void* stream);

/* ---------------------------------------------------------------- producer of the v2 latent records (csrc/train.hip)
 * What preprocess_scripts/preprocess_with_motion_prior.py:328-409 computes BETWEEN the teacher's forwards when it makes the records the
 * v2 step trains on, on activations laid out [B][per_clip] as above, with the tables of t2v_cd_sched (topk and timestep_scaling are
 * not read): one launch each, every per-clip coefficient looked up on the device, no host synchronisation.  Table reads are clamped
 * as above; coefficients are formed in double and rounded to fp32 once; an element takes one product and one fused multiply-add.
 *
 * t2v_cd_add_noise (scheduler/t2v_turbo_scheduler.py:470-495 at t_s = ddim_timesteps[index[b]]):
 *   z = sqrt(alphas_cumprod[t_s]) x + sqrt(1 - alphas_cumprod[t_s]) noise                                         -> z (fp32)
 *   x, noise: a dtype code each (T2V_F32 / T2V_BF16 / T2V_F16).  z_lp: NULL, or a copy of z rounded to nearest even into dt_lp
 *   (T2V_BF16 / T2V_F16): the UNet's input.
 *
 * t2v_ddim_reverse_step (ode_solver/ddim_solver.py ddim_reverse_step inside motion_prior_sample.py:27-37): inversion step i
 * (0 <= i < n_ddim) of EVERY clip; the inverted latent x stays fp32, in place, between the steps.  Per clip b with
 * idx = clamp(index[b]):
 *   i >  idx: the clip's inversion is over: x is not written; x_lp (when given) is rewritten from it.
 *   i == idx and prev != NULL: prev <- x first (z_example_prev; the original latent when idx == 0, :351-355), then the step.
 *   i <= idx: t = ddim_timesteps[i], t_p = max(t - step_ratio, 0), a_n = alphas_cumprod[t], a = alphas_cumprod[t_p],
 *             x <- (x - sqrt(1 - a) eps) sqrt(a_n / a) + sqrt(1 - a_n) eps;  x_lp (when given) <- x rounded to nearest even.
 *   eps: fp32 or bf16 (the teacher's prediction at (x_lp, t)).  prev: fp32 or NULL.  x_lp: bf16 / fp16 or NULL.
 *
 * t2v_pack_f16_multi: up to T2V_PACK_MAX tensors converted into ONE fp16 buffer in one launch (the hand-over of a batch of records:
 * one launch and then one copy to the host instead of a cast and a copy per tensor).  `table` is a HOST array, handed to the kernel by
 * value; entry j holds `rows` rows of n contiguous elements and writes row r to dst[dst_off + r * dst_stride, ... + n) (rows = 1: one
 * flat tensor; rows = B with dst_stride = the record length: one tensor of every clip into a clip-by-clip layout).  Entries must not
 * overlap each other in dst (not checked).  The conversion is torch.Tensor.to(torch.float16): round to nearest even, overflow
 * to +-inf, NaN stays NaN (the quiet NaN without a payload keeps its bits, 0x7E00), subnormals are produced, -0 is kept.  A workgroup moves T2V_PACK_BLOCK elements
 * of one row; 16-byte accesses between the destination's first and last 16-byte boundary inside the row when the source is
 * 16-byte aligned there, scalar accesses for the rest; nothing outside the rows' destination ranges is written.
 *
 * Refused before any launch: null pointers, non-positive sizes, a step outside [0, n_ddim), a negative step_ratio or offset, an entry
 * count outside 1..T2V_PACK_MAX: T2V_EINVAL; a dtype code outside the above, B > T2V_CD_MAX_CLIPS, a source off its element boundary,
 * an entry whose rows overlap (dst_stride < n) or that ends past dst_numel: T2V_ESHAPE. */
#define T2V_PACK_MAX 16
#define T2V_PACK_BLOCK 2048
typedef struct t2v_pack_entry {
    const void* src;      /* [rows][n] contiguous, device */
    long long n;          /* elements of a row */
    long long rows;
    long long dst_off;    /* first element of row 0 in dst */
    long long dst_stride; /* elements between the starts of two rows in dst (not read when rows == 1) */
    int dt;               /* T2V_F32, T2V_BF16 or T2V_F16 */
    int reserved;
} t2v_pack_entry;
int t2v_cd_add_noise(const t2v_cd_sched* s, const void* x, int dt_x, const void* noise, int dt_noise, float* z, void* z_lp, int dt_lp,
                     int B, long long per_clip, void* stream);
int t2v_ddim_reverse_step(const t2v_cd_sched* s, int i, int step_ratio, float* x, const void* eps, int dt_eps, float* prev, void* x_lp,
                          int dt_lp, int B, long long per_clip, void* stream);
int t2v_pack_f16_multi(const t2v_pack_entry* table /* host */, int n_entries, void* dst, long long dst_numel, void* stream);

/* ---------------------------------------------------------------- head of one step of the motion-prior guided sampler (csrc/train.hip)
 * What motion_prior_sample.py:180-196, 283-292 computes BETWEEN the forwards of sampling step i: one launch for the whole batch.  All
 * clips share step i, passed by value: t2v_cd_sched::index is not read and may be NULL (topk and timestep_scaling are not read
 * either).  The latent x stays fp32, in place, between the steps, as t2v_ddim_reverse_step keeps the inverted latent.  With
 *   t = ddim_timesteps[i], a = sqrt(alphas_cumprod[t]), sg = sqrt(1 - alphas_cumprod[t]), ap = ddim_alpha_cumprods_prev[i], w = guidance_scale:
 *   x0c = (x - sg cond) / a, x0u = (x - sg uncond) / a       (x0_cond and x0_uncond both NULL), or
 *   x0c = x0_cond, x0u = x0_uncond                          (both given: a cached motion_intermediate entry, used as is)
 *   x0  = x0c + w (x0c - x0u)
 *   eps = cond + w (cond - uncond) - sqrt(1 - a) score      (score NULL: no motion term; note a, not alphas_cumprod: the script writes
 *                                                            (1 - alphas) ** 0.5 with alphas = sqrt(alphas_cumprod[t]); no motion_gs factor)
 *   x  <- sqrt(ap) x0 + sqrt(1 - ap) eps
 * cond / uncond share dt_eps, x0_cond / x0_uncond share dt_x0, score has dt_score: fp32, bf16 or fp16 each.  Optional outputs: x_lp,
 * the new x rounded to nearest even into bf16 / fp16 (the UNet's next input); pred_x0, the CFG x0 in dt_p (fp32 / bf16 / fp16); rec,
 * fp16 [B][5][per_clip]: the step's motion_intermediate entry in the order cond_pred_x_0 | uncond_pred_x_0 | cond_pred_noise |
 * uncond_pred_noise | score (zeros when score is NULL), converted with the semantics documented for t2v_pack_f16_multi.
 * Coefficients are formed in double and rounded to fp32 once (1 / a, sg / a, sqrt(ap), sqrt(1 - ap), sqrt(1 - a)); x0c and x0u are
 * each rounded to fp32 once (they are outputs), then one fused multiply-add per line above.  Table reads are clamped; 16-byte accesses
 * when every pointer is 16-byte aligned (rec: and per_clip a multiple of 8), scalar accesses otherwise.
 * Refused before any launch: null x / cond / uncond / schedule tables, non-positive sizes, exactly one of x0_cond / x0_uncond given,
 * i outside [0, n_ddim): T2V_EINVAL; a dtype code outside the above, B > T2V_CD_MAX_CLIPS: T2V_ESHAPE. */
int t2v_mp_guided_step(const t2v_cd_sched* s, int i, float guidance_scale, float* x, const void* cond, const void* uncond, int dt_eps,
                       const void* x0_cond, const void* x0_uncond, int dt_x0, const void* score, int dt_score, void* x_lp, int dt_lp,
                       void* pred_x0, int dt_p, void* rec, int B, long long per_clip, void* stream);

/* ---------------------------------------------------------------- recorded launch lists
 * The reference has no counterpart: its hot path is issued op by op from Python (and that is what bounds a small-batch step on
 * the host).  The engines of this library record a forward / backward once and replay it; t2v_replay walks such a recording —
 * a flat array of 64-bit words [function id, n, n argument slots] ... — inside the library, one host call per LIST instead of
 * one per launch.  Function ids come from t2v_replay_lookup(name) (-1: not a replayable entry point).  A slot holds an integer
 * or pointer value as is, a float as its 32 bits (low half), a double as its 64 bits; the stream parameter (always last in the
 * entry point's signature) is not stored: every launch goes to the stream given here.  Returns the first non-zero return code
 * and its launch index in *failed_index (may be NULL). */
int t2v_replay_lookup(const char* name);
int t2v_replay(const unsigned long long* prog, long long nwords, void* stream, int* failed_index);

#ifdef __cplusplus
}
#endif
#endif /* T2V_HIP_H */
