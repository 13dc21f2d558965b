"""The GEMM family at the ENGINES' operand forms, with poisoned padding — one table, two backends (the companion of
tests/operand_form_cases.py, whose helpers it imports).

Entries: t2v_gemm (tile and store-path sweep, the six gather modes with strided A, split-K, per-head batching, GEGLU / SiLU / alpha /
M = 2 / N = 4, the fused epilogues rowstat_out / colstat_out / lnf_* / ln_out / dropout / LoRA), t2v_conv_halo, t2v_linear_pr,
t2v_wgrad_tn and t2v_wgrad_tn_group, t2v_conv3x3_small_cin, t2v_dropout_bf16, t2v_repack_conv_f32.  ``tests/test_hostsim_gemm_forms.py``
runs the table on the host SIMT simulator, ``tests/test_gpu_gemm_forms.py`` on the device.

Operands (everything stays inside one allocation per tensor; no case makes an out-of-bounds access):
  * A (both parts of a virtual concat), W, the residual, rowvec, lora_t, lora_u, lnf_stats and the wgrad operands are views into larger
    buffers: row stride > width, a column offset, spare rows before and after.  Bytes include/t2v_hip.h says are NOT read hold NaN: the
    stride gaps, the spare rows (so: A rows >= M, W rows >= N, the tail of a weight row between K and ldw, the rows a conv padding tap
    would find in the neighbouring row / image / clip).  Bytes it says ARE read hold what it demands (the zero-padded rank columns of
    lora_u, the zero padding of the conv_halo pack up to t2v_conv_halo_pack_cols).  Flat fp32 vectors sit inside NaN-padded flats.
  * outputs (out, ln_out, rowstat_out, colstat_out, the wgrad outputs, the split-K / wgrad workspaces) are ``Out`` allocations: the
    must-write region is pre-filled with NaN and must come back finite, everything else holds a sentinel compared BIT FOR BIT.

Reference: fp64 torch, written here from the definitions in include/t2v_hip.h (never tests/emu_ops.py): the gathers as index
arithmetic, the GEGLU interleave, the splitmix64 mask, the LoRA / lnf / statistics epilogues and their rounding points.

Assertions per output tensor: (1) worst ROW and (2) worst COLUMN of e = ||got - ref|| / max(||ref||, 0.1 rms norm) below
max(project tolerance of the family, 2 x the same metric of the reference rounded to the documented types); (3) worst ELEMENT:
    |got - ref| <= 2^-8 |ref| + 2 (K + splits) 2^-24 (|A| |W|^T |alpha|) + 8 2^-24 (|bias| + |rowvec| + |residual| + |lora term|)
(first term dropped for fp32 outputs; SiLU / GEGLU: the linear terms carried through the activation's slope, plus twice the measured
approximation error of the activation: ``ACT_ERR``).  Exact data movement (t2v_repack_conv_f32, which elements a dropout zeroes) is
compared bit for bit.  ``REPORT`` (shared with operand_form_cases) collects (rounding, bound, observed) per tensor; the element check
reports observed / limit (bound 1).

Where a tensor gets fewer than the three assertions, and what the table does not combine:
  * t2v_linear_pr with ln_in / gn_coef (5 of its 19 cases): rows and columns only.  The kernel rounds the NORMALISED A rows to bf16 before
    the product; the reference does the same in fp64, and an element that lies within an fp32 ulp of a bf16 rounding boundary may round the
    other way on the device — a whole bf16 ulp of one input, for which the element bound (built for exact inputs) has no term.
  * ln_out, rowstat_out, colstat_out: rows and columns (the element formula is stated for the product's output; these are reductions over
    it, bounded by STAT_TOL / BF16_TOL against their own rounding); the main output of the same launch gets all three.
  * every t2v_gemm case hands the library a guarded workspace of exactly max(split_k, 1) * M * N floats, so a launch that did not ask for
    a K split cannot take the library's automatic one (it shrinks to the workspace: one split): the gather-mode cases with deep K
    (9 x 192) run unsplit, and gathers meet split-K only in the explicit CONV3X3 / LINEAR split-K cases.

Tile classes of t2v_gemm (ids that share workgroup tile bm x bn, K step bk and staging path run the same load / store index code and
differ only in wave layout and ring depth): DMA-staged  128x128x64: 1 4 10 30 31 | 128x64x64: 2 5 | 256x64x64: 3 9 | 256x128x64: 6 7 13 |
64x128x64: 8 | 128x256x64: 11 14 | 256x256x64: 12 15 | 256x128x32: 16 19 | 128x256x32: 17 | 128x128x32: 18 32 33 | 256x256x32: 20 21 24 |
160x320x64: 22 | 160x320x32: 23;  register-staged (experimental)  25 26 27 28 29, one class each.  ``CLASS_REPS`` holds the first id of
each class; the gather-mode cases run on the representatives, the tile / store-path sweep on every id.

Measured figures (worst over a family's cases; rounding = the metric of the fp64 reference rounded to the documented types, i.e. of the
reference alone; bound = what the cases assert; "elem" rows: observed error / element limit, bound 1; pattern / pack / second-launch rows:
number of differing elements): the MEASURED table below, ``report_table()`` of the device file's 472 cases on both backends, merged line by line.  The element
ratios sit just under 1 by construction (a bf16 result whose only error is its final rounding reaches 2^-8 |ref| next to a power of two);
the wgrad products, fp32 throughout, use under 1 % of their limit.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from t2v_turbo_amd import native as nt
from tests.operand_form_cases import (BF, BF16_TOL, BWD_TOL, F32, NAN, REPORT, SENT, STAT_TOL, Out, _CUR, _raw, _with_stride, bfr, close,  # noqa: F401
                                      exact, f32r, inbuf, inflat, refuses, rnd, row_err, run, run_refusal)

MEASURED = """
    family                 tensor                    cases  rounding  bound     simulator  MI355X
    conv_halo              colstat                       5  3.1e-08   1.0e-04   6.8e-08    6.8e-08
    conv_halo              colstat cols                  5  4.0e-08   1.0e-04   1.7e-07    1.7e-07
    conv_halo              colstat vs reference          5  3.1e-08   4.0e-03   5.7e-05    7.8e-05
    conv_halo              out                          35  2.3e-03   4.7e-03   2.3e-03    2.3e-03
    conv_halo              out cols                     35  2.1e-03   4.2e-03   2.1e-03    2.1e-03
    conv_halo              out elem                     35  0.0e+00   1.0e+00   9.5e-01    9.5e-01
    conv_halo              second launch                35  0.0e+00   0.0e+00   0.0e+00    0.0e+00
    conv_halo              second launch colstat         5  0.0e+00   0.0e+00   0.0e+00    0.0e+00
    conv_small_cin         out                           4  2.1e-03   4.3e-03   2.1e-03    2.1e-03
    conv_small_cin         out cols                      4  2.0e-03   4.0e-03   2.0e-03    2.0e-03
    conv_small_cin         out elem                      4  0.0e+00   1.0e+00   9.9e-01    9.9e-01
    dropout                dropped pattern               6  0.0e+00   0.0e+00   0.0e+00    0.0e+00
    dropout                out                           6  2.1e-03   4.2e-03   3.2e-03    3.2e-03
    dropout                out cols                      6  2.5e-03   5.0e-03   3.3e-03    3.3e-03
    gemm                   out                         318  2.3e-03   4.7e-03   2.3e-03    2.3e-03
    gemm                   out cols                    318  3.0e-03   6.0e-03   3.0e-03    3.0e-03
    gemm                   out elem                    318  0.0e+00   1.0e+00   9.9e-01    9.9e-01
    gemm-M2                out                           3  1.8e-03   4.0e-03   1.8e-03    1.8e-03
    gemm-M2                out cols                      3  3.6e-03   7.1e-03   3.6e-03    3.6e-03
    gemm-M2                out elem                      3  0.0e+00   1.0e+00   9.4e-01    9.4e-01
    gemm-N4                out                           3  2.9e-03   5.9e-03   2.9e-03    2.9e-03
    gemm-N4                out cols                      3  1.8e-03   4.0e-03   1.8e-03    1.8e-03
    gemm-N4                out elem                      3  0.0e+00   1.0e+00   9.7e-01    9.7e-01
    gemm-act               gelu abs err                  1  0.0e+00   3.7e-05   3.6e-05    3.6e-05
    gemm-act               silu abs err                  1  0.0e+00   6.7e-07   6.7e-07    6.7e-07
    gemm-alpha             out                           3  2.0e-03   4.0e-03   2.0e-03    2.0e-03
    gemm-alpha             out cols                      3  2.0e-03   4.0e-03   2.0e-03    2.0e-03
    gemm-alpha             out elem                      3  0.0e+00   1.0e+00   9.8e-01    9.8e-01
    gemm-batched           out                           4  2.0e-03   4.0e-03   2.0e-03    2.0e-03
    gemm-batched           out cols                      4  2.0e-03   4.1e-03   2.0e-03    2.0e-03
    gemm-batched           out elem                      4  0.0e+00   1.0e+00   9.8e-01    9.8e-01
    gemm-colstat           colstat                       7  2.7e-08   1.0e-04   4.0e-08    4.0e-08
    gemm-colstat           colstat cols                  7  4.7e-08   1.0e-04   1.3e-07    1.3e-07
    gemm-colstat           colstat vs reference          7  2.7e-08   4.0e-03   4.0e-08    4.0e-08
    gemm-colstat           out                           7  2.1e-03   4.2e-03   2.1e-03    2.1e-03
    gemm-colstat           out cols                      7  2.4e-03   4.8e-03   2.4e-03    2.4e-03
    gemm-colstat           out elem                      7  0.0e+00   1.0e+00   9.8e-01    9.8e-01
    gemm-dropout           dropped pattern              11  0.0e+00   0.0e+00   0.0e+00    0.0e+00
    gemm-dropout           out                          11  2.2e-03   4.3e-03   2.2e-03    2.2e-03
    gemm-dropout           out cols                     11  2.1e-03   4.1e-03   2.1e-03    2.1e-03
    gemm-dropout           out elem                     11  0.0e+00   1.0e+00   9.9e-01    9.9e-01
    gemm-dropout           t2v_dropout_bf16 pattern     11  0.0e+00   0.0e+00   0.0e+00    0.0e+00
    gemm-geglu             out                           5  2.6e-03   5.3e-03   2.6e-03    2.6e-03
    gemm-geglu             out cols                      5  2.5e-03   5.0e-03   2.5e-03    2.5e-03
    gemm-geglu             out elem                      5  0.0e+00   1.0e+00   9.4e-01    9.4e-01
    gemm-ln_out            ln_out                        2  1.9e-03   4.0e-03   1.9e-03    1.9e-03
    gemm-ln_out            ln_out cols                   2  2.1e-03   4.2e-03   2.1e-03    2.1e-03
    gemm-ln_out            out                           2  1.9e-03   4.0e-03   1.9e-03    1.9e-03
    gemm-ln_out            out cols                      2  2.1e-03   4.2e-03   2.1e-03    2.1e-03
    gemm-ln_out            out elem                      2  0.0e+00   1.0e+00   9.9e-01    9.9e-01
    gemm-lnf               out                           4  2.8e-03   5.7e-03   2.8e-03    2.8e-03
    gemm-lnf               out cols                      4  2.4e-03   4.7e-03   2.4e-03    2.4e-03
    gemm-lnf               out elem                      4  0.0e+00   1.0e+00   9.8e-01    9.8e-01
    gemm-lora              colstat                       1  2.8e-08   1.0e-04   4.2e-08    4.2e-08
    gemm-lora              colstat cols                  1  3.7e-08   1.0e-04   6.5e-08    6.5e-08
    gemm-lora              colstat vs reference          1  2.8e-08   4.0e-03   4.2e-08    4.2e-08
    gemm-lora              out                           9  2.1e-03   4.2e-03   2.1e-03    2.1e-03
    gemm-lora              out cols                      9  2.1e-03   4.2e-03   2.1e-03    2.1e-03
    gemm-lora              out elem                      9  0.0e+00   1.0e+00   9.9e-01    9.9e-01
    gemm-rowstat           out                           3  2.0e-03   4.0e-03   2.0e-03    2.0e-03
    gemm-rowstat           out cols                      3  2.1e-03   4.2e-03   2.1e-03    2.1e-03
    gemm-rowstat           out elem                      3  0.0e+00   1.0e+00   9.7e-01    9.7e-01
    gemm-rowstat           rowstat                       3  6.1e-08   1.0e-04   1.6e-07    1.6e-07
    gemm-rowstat           rowstat cols                  3  3.8e-08   1.0e-04   1.1e-07    1.1e-07
    gemm-silu              out                           3  2.3e-03   4.5e-03   2.3e-03    2.3e-03
    gemm-silu              out cols                      3  2.4e-03   4.8e-03   2.4e-03    2.4e-03
    gemm-silu              out elem                      3  0.0e+00   1.0e+00   9.9e-01    9.9e-01
    gemm-splitk2           out                           4  2.1e-03   4.2e-03   2.1e-03    2.1e-03
    gemm-splitk2           out cols                      4  2.0e-03   4.0e-03   2.0e-03    2.0e-03
    gemm-splitk2           out elem                      4  0.0e+00   1.0e+00   8.5e-01    8.5e-01
    gemm-splitk3           out                           6  2.1e-03   4.2e-03   2.1e-03    2.1e-03
    gemm-splitk3           out cols                      6  2.1e-03   4.1e-03   2.1e-03    2.1e-03
    gemm-splitk3           out elem                      6  0.0e+00   1.0e+00   8.6e-01    8.6e-01
    gemm-splitk5           out                           4  2.3e-03   4.5e-03   2.3e-03    2.3e-03
    gemm-splitk5           out cols                      4  1.9e-03   4.0e-03   1.9e-03    1.9e-03
    gemm-splitk5           out elem                      4  0.0e+00   1.0e+00   8.9e-01    8.9e-01
    linear_pr              out                          19  2.2e-03   4.3e-03   2.2e-03    2.2e-03
    linear_pr              out cols                     19  2.6e-03   5.1e-03   2.6e-03    2.6e-03
    linear_pr              out elem                     14  0.0e+00   1.0e+00   9.5e-01    9.5e-01
    repack_conv            pack                          4  0.0e+00   0.0e+00   0.0e+00    0.0e+00
    wgrad                  group out                     4  3.4e-08   2.0e-04   8.7e-08    8.4e-08
    wgrad                  group out cols                4  3.3e-08   2.0e-04   8.2e-08    7.9e-08
    wgrad                  group out elem                4  0.0e+00   1.0e+00   3.4e-03    4.2e-03
    wgrad                  group second launch           4  0.0e+00   0.0e+00   0.0e+00    0.0e+00
    wgrad                  out                          13  3.2e-08   2.0e-04   1.5e-07    1.2e-07
    wgrad                  out cols                     13  5.9e-08   2.0e-04   6.9e-07    6.6e-07
    wgrad                  out elem                     13  0.0e+00   1.0e+00   8.6e-03    5.1e-03
    wgrad                  second launch                13  0.0e+00   0.0e+00   0.0e+00    0.0e+00
"""

WGRAD_TOL = 2e-4
# twice these (measured on the simulator by ``case_act_probe``: fp32 output of a GEGLU / SiLU launch whose product is exactly the probe
# value, against the fp64 function over every bf16 value in [-8, 8]) is the activation allowance of the element check
# measured: gelu 3.64e-05 on both backends (csrc/gelu_poly.h states < 4.2e-5); silu 6.66e-07 on both (fp32 rounding at |x| = 8)
ACT_ERR = {"gelu": 3.7e-5, "silu": 6.7e-7}

DMA_REPS = [1, 2, 3, 6, 8, 11, 12, 16, 17, 18, 20, 22, 23]
RS_IDS = [25, 26, 27, 28, 29]
CLASS_REPS = DMA_REPS + RS_IDS
VALIDATED = list(range(1, 24)) + [30, 31, 32, 33]
EXPERIMENTAL = list(range(24, 30))     # device: only with T2V_TEST_EXPERIMENTAL_TILES=1
BK = {**{i: 64 for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 22, 25, 26, 30, 31)},
      **{i: 32 for i in (16, 17, 18, 19, 20, 21, 23, 24, 27, 28, 29, 32, 33)}}
EPS24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ helpers
def close_rc(name, got, ref, ref_rounded, tol):
    """Worst row and worst column."""
    close(name, got, ref, ref_rounded, tol)
    close(name + " cols", got.t(), ref.t(), ref_rounded.t(), tol)


def elem(name, got, ref, slack, half_ulp=2.0 ** -8):
    """|got - ref| <= half_ulp |ref| + slack, element by element; reports the worst observed / limit."""
    lim = half_ulp * ref.abs() + slack
    ratio = (got.double() - ref).abs() / lim.clamp_min(1e-300)
    worst = float(ratio.max())
    REPORT.append((_CUR[0], name + " elem", 0.0, 1.0, worst))
    if worst > 1.0:
        idx = [int(i) for i in (ratio == ratio.max()).nonzero()[0]]
        raise AssertionError(f"{name}: element {idx} off by {worst:.2f} x its limit (got {float(got[tuple(idx)]):.6g}, want {float(ref[tuple(idx)]):.6g})")


class Arena(Out):
    """An output allocation [rows, ld] with rectangular must-write regions (r0, r1, c0, c1); the rest is sentinel."""

    def __init__(self, rows, ld, regions, dev, dtype=F32, init=None):
        full = torch.full((rows, ld), SENT, dtype=dtype)
        self.mask = torch.zeros(rows, ld, dtype=torch.bool)
        for r0, r1, c0, c1 in regions:
            full[r0:r1, c0:c1] = NAN if init is None else init
            self.mask[r0:r1, c0:c1] = True
        self.regions, self.snap, self.full = regions, full.clone(), full.to(dev)
        self.views = [self.full[r0:r1, c0:c1] for r0, r1, c0, c1 in regions]

    def check(self, what):
        got = self.guard(what)
        outs = [got[r0:r1, c0:c1] for r0, r1, c0, c1 in self.regions]
        for i, o in enumerate(outs):
            fin = torch.isfinite(o.double())
            assert bool(fin.all()), f"{what}[{i}]: non-finite / unwritten at (row, col) {(~fin).nonzero()[0].tolist()}"
        return outs


class Workspace:
    """The backend's split-K / wgrad workspace replaced by ``n`` fp32 of a guarded allocation for the duration of a case: the launch is
    told ws_bytes = 4 n, the floats behind them hold the sentinel."""

    def __init__(self, ops, dev, n):
        assert n % 4 == 0
        self.out = Arena(3, n + 16, [(1, 2, 0, n)], dev, F32, init=0.0)
        self.ops = ops
        self.bytes = self.out.views[0].reshape(-1).view(torch.uint8)

    def __enter__(self):
        d = self.bytes.device
        self.key = (d.type, d.index)
        self.saved = self.ops._ws.get(self.key)
        self.ops._ws[self.key] = self.bytes
        return self

    def __exit__(self, *exc):
        if self.saved is None:
            self.ops._ws.pop(self.key, None)
        else:
            self.ops._ws[self.key] = self.saved

    def untouched(self):
        return self.out.untouched()

    def guard(self, what):
        return self.out.guard(what)


def same_pattern(name, got, base, contrib, keep):
    """Which elements were dropped, bit for bit: a dropped element IS ``base`` (zero, or the bf16 residual / row-vector sum), a kept one
    is not — judged where the kept contribution is large enough to move ``base`` at all (> 2^-6 |base|; nearly everywhere)."""
    distinct = contrib.abs() > 2.0 ** -6 * base.abs()
    assert float(distinct.double().mean()) > 0.97, name
    dropped = _raw(got) == _raw(base.to(F32).to(BF))
    exact(name, (dropped & distinct).to(torch.int32), (~keep & distinct).to(torch.int32))


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def silu64(x):
    return x * torch.sigmoid(x)


# ------------------------------------------------------------------------------------------------------------------ gather (t2v_hip.h: T2V_GEMM_*)
def out_grid(mode, n_img, h, w):
    if mode in (nt.GEMM_LINEAR, nt.GEMM_TCONV3, nt.GEMM_CONV3X3):
        return h, w
    if mode == nt.GEMM_CONV3X3_UP2:
        return 2 * h, 2 * w
    if mode == nt.GEMM_CONV3X3_S2:
        return (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    return (h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1      # S2_PAD01: pad right / bottom only


def gather(x, mode, n_img=0, h=0, w=0, frames=0):
    """x [source rows, C] -> the implicit-GEMM A matrix [M, taps * C], K order tap-major then channel; taps outside the grid are 0."""
    C = x.shape[1]
    if mode == nt.GEMM_LINEAR:
        return x
    if mode == nt.GEMM_TCONV3:   # tap t = frame offset t - 1 inside the clip
        x5 = x.reshape(n_img // frames, frames, h * w, C)
        out = torch.zeros(n_img // frames, frames, h * w, 3, C, dtype=x.dtype)
        for t in range(3):
            for f in range(frames):
                if 0 <= f + t - 1 < frames:
                    out[:, f, :, t] = x5[:, f + t - 1]
        return out.reshape(-1, 3 * C)
    stride = 2 if mode in (nt.GEMM_CONV3X3_S2, nt.GEMM_CONV3X3_S2_PAD01) else 1
    pad = 0 if mode == nt.GEMM_CONV3X3_S2_PAD01 else 1
    ups = 1 if mode == nt.GEMM_CONV3X3_UP2 else 0
    ho, wo = out_grid(mode, n_img, h, w)
    x4 = x.reshape(n_img, h, w, C)
    out = torch.zeros(n_img, ho, wo, 9, C, dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            for oy in range(ho):
                uy = oy * stride + ky - pad
                if not 0 <= uy < (h << ups):
                    continue
                for ox in range(wo):
                    ux = ox * stride + kx - pad
                    if 0 <= ux < (w << ups):
                        out[:, oy, ox, ky * 3 + kx] = x4[:, uy >> ups, ux >> ups]
    return out.reshape(-1, 9 * C)


# ------------------------------------------------------------------------------------------------------------------ dropout mask (t2v_hip.h: t2v_dropout_bf16)
def drop_thr16(p):
    t = float(p) * 4294967296.0
    return (0xFFFFFFFF if t >= 4294967295.0 else int(t)) >> 16


def keep_mask(seed, site, rows, ncols, p):
    """keep[r][c] of the [rows][ncols] matrix: word = splitmix64 finaliser of seed + site * 0x9E3779B97F4A7C15 + (i >> 2) * 0xD1B54A32D192ED03,
    element i = r * ncols + c keeps iff bits [16 (i & 3), +16) of the word >= (p * 2^32) >> 16."""
    m64 = (1 << 64) - 1
    key = (int(seed) + int(site) * 0x9E3779B97F4A7C15) & m64
    i = np.arange(rows * ncols, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(key) + (i >> np.uint64(2)) * np.uint64(0xD1B54A32D192ED03)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    bits = (z >> (np.uint64(16) * (i & np.uint64(3)))) & np.uint64(0xFFFF)
    return torch.from_numpy((bits >= np.uint64(drop_thr16(p))).reshape(rows, ncols))


def inv_keep(p):
    return float(np.float32(65536.0) / np.float32(65536.0 - drop_thr16(p)))


def seed_tensor(dev, value=0x1234_5678_9ABC):
    return inflat(torch.tensor([value], dtype=torch.int64), dev, torch.int64, pad=2)


# ------------------------------------------------------------------------------------------------------------------ t2v_gemm
class Gemm:
    """One t2v_gemm problem: fp64 data, the poisoned device operands and the fp64 reference with its element slack."""

    def __init__(self, dev, *, M, N, c0, c1=0, mode=nt.GEMM_LINEAR, n_img=0, h=0, w=0, frames=0, bias=True, rowvec_div=0, residual=False,
                 act=nt.ACT_NONE, alpha=1.0, out="vec", seed=0, wscale=None, ashift=0.0):
        self.dev, self.M, self.N, self.mode, self.act, self.alpha = dev, M, N, mode, act, alpha
        self.geo = dict(n_img=n_img, h=h, w=w, frames=frames)
        taps = {nt.GEMM_LINEAR: 1, nt.GEMM_TCONV3: 3}.get(mode, 9)
        self.K = K = taps * (c0 + c1)
        rows = M if mode == nt.GEMM_LINEAR else n_img * h * w
        if mode != nt.GEMM_LINEAR:
            ho, wo = out_grid(mode, n_img, h, w)
            assert M == n_img * ho * wo
        self.n_out = n_out = N // 2 if act == nt.ACT_GEGLU else N
        self.a = rnd(rows, c0 + c1, seed=seed + 1, shift=ashift)
        self.wt = rnd(N, K, seed=seed + 2, scale=wscale or K ** -0.5)
        self.bias = f32r(rnd(N, seed=seed + 3)) if bias else None
        self.rowvec_div = rowvec_div
        self.rv = f32r(rnd((M + rowvec_div - 1) // rowvec_div, n_out, seed=seed + 4)) if rowvec_div else None
        self.res = rnd(M, n_out, seed=seed + 5) if residual else None
        # device operands: every 2-D one a view (rows [2, 2 + n), a column offset) of a NaN buffer with a longer row stride
        self.a0_d = inbuf(self.a[:, :c0], c0 + 16, dev, col0=8)
        self.a1_d = inbuf(self.a[:, c0:], c1 + 24, dev, col0=16) if c1 else None
        self.w_d = inbuf(self.wt, K + 16, dev, col0=8)
        self.bias_d = None if self.bias is None else inflat(self.bias, dev)
        scalar = out == "scalar"
        self.rv_d = None if self.rv is None else inbuf(self.rv, n_out + (7 if scalar else 12), dev, F32, col0=3 if scalar else 4)
        self.res_d = None if self.res is None else inbuf(self.res, n_out + 10 if scalar else (n_out + 31) // 8 * 8, dev, col0=2 if scalar else 16)
        if out == "vec":        # ldo % 8 == 0, 16-byte aligned base: the vector store path (the fast kernels where n_out % 16 == 0)
            self.out = Out(M, (n_out + 23) // 8 * 8, [(8, 8 + n_out)], dev)
        elif scalar:            # ldo an odd multiple of 2, base 4 bytes off: the scalar store path
            self.out = Out(M, n_out + 6, [(2, 2 + n_out)], dev)
        else:                   # fp32
            self.out = Out(M, (n_out + 15) // 8 * 8, [(4, 4 + n_out)], dev, F32)
        self.f32 = out == "f32"

    def kw(self, **more):
        return dict(dict(M=self.M, N=self.N, a1=self.a1_d, mode=self.mode, n_img=self.geo["n_img"], h=self.geo["h"], wd=self.geo["w"],
                         frames=self.geo["frames"], bias=self.bias_d, rowvec=self.rv_d, rowvec_div=self.rowvec_div, residual=self.res_d,
                         act=self.act, alpha=self.alpha), **more)

    def reference(self, splits=1, keep=None, p_drop=0.0, lora=None, lnf=None):
        """-> (ref fp64 [M, n_out], element slack, fp32 epilogue value before the activation / store)."""
        G = gather(self.a, self.mode, **self.geo)
        acc = G @ self.wt.t()
        dot = 2.0 * (self.K + splits) * EPS24 * abs(self.alpha) * (G.abs() @ self.wt.abs().t())
        v = self.alpha * acc
        add = torch.zeros_like(v)
        if lnf is not None:   # out = rstd (acc - mean s[n]) + bias[n]
            mean, rstd, s = lnf
            v = rstd[:, None] * (acc - mean[:, None] * s[None, :])
            # (mean and rstd are fp32 results of fp32 sums: a few ulp each, carried by the terms they multiply)
            dot = rstd[:, None].abs() * (dot + 16.0 * EPS24 * (mean[:, None] * s[None, :]).abs()) + 8.0 * EPS24 * v.abs()
        if self.bias is not None:
            v = v + self.bias
            add = add + self.bias.abs()
        if self.act == nt.ACT_GEGLU:   # W rows in 64-row groups [32 value | 32 gate]; out column 32 g + j
            vg, sg = v.reshape(self.M, -1, 2, 32), (dot + 8.0 * EPS24 * add).reshape(self.M, -1, 2, 32)
            val, gate = vg[:, :, 0].reshape(self.M, -1), vg[:, :, 1].reshape(self.M, -1)
            ref = val * gelu64(gate)
            slack = (sg[:, :, 0].reshape(self.M, -1) * gelu64(gate).abs() + 1.13 * sg[:, :, 1].reshape(self.M, -1) * val.abs()
                     + 2.0 * ACT_ERR["gelu"] * val.abs())
            return ref, slack, None
        if keep is not None and lora is None:
            v = torch.where(keep, v * inv_keep(p_drop), torch.zeros_like(v))
            dot, add = dot * inv_keep(p_drop), add * inv_keep(p_drop)
        if self.rv is not None:
            r = self.rv[torch.arange(self.M) // self.rowvec_div]
            v, add = v + r, add + r.abs()
        if self.res is not None:
            v, add = v + self.res, add + self.res.abs()
        if lora is not None:   # + lora_scale * dropout(t_l u_n^T): the mask on the LoRA product only
            t, u, n_leaf, scale = lora
            z = torch.cat([t[:, 64 * l:64 * l + 64] @ u[l * n_leaf:(l + 1) * n_leaf, :64].t() for l in range(self.N // n_leaf)], dim=1)
            za = torch.cat([t[:, 64 * l:64 * l + 64].abs() @ u[l * n_leaf:(l + 1) * n_leaf, :64].abs().t() for l in range(self.N // n_leaf)], dim=1)
            sc = scale * (inv_keep(p_drop) if keep is not None else 1.0)
            z, za = z * sc, za * abs(sc)
            if keep is not None:
                z, za = torch.where(keep, z, torch.zeros_like(z)), torch.where(keep, za, torch.zeros_like(za))
            v, add = v + z, add + z.abs()
            dot = dot + 2.0 * 65 * EPS24 * za
        slack = dot + 8.0 * EPS24 * add
        if self.act == nt.ACT_SILU:
            return silu64(v), 1.1 * slack + 2.0 * ACT_ERR["silu"], v
        return v, slack, v

    def check(self, name, ref, slack, tol=BF16_TOL):
        got = self.out.check(name)[0]
        rr = f32r(ref) if self.f32 else bfr(ref)
        close_rc(name, got, ref, rr, tol)
        elem(name, got, ref, slack, 0.0 if self.f32 else 2.0 ** -8)
        return got


def case_gemm(ops, dev, cfg, out="vec", split=0, expect_splits=None, **shape):
    """Plain / split-K t2v_gemm on tile ``cfg`` in output form ``out``; with ``split``: the guarded workspace holds exactly
    split * M * N floats, the plan must report ``expect_splits`` (1: the launch cannot split and falls back)."""
    g = Gemm(dev, out=out, **shape)
    kw = g.kw(tile_cfg=cfg, split_k=split)
    n_ws = (max(split, 1) * g.M * g.N + 3) // 4 * 4
    with Workspace(ops, dev, n_ws) as ws:
        _, splits = ops.gemm_plan(g.a0_d, g.w_d, g.out.views[0], **kw)
        if expect_splits is not None:
            assert splits == expect_splits, f"plan: {splits} K splits, expected {expect_splits}"
        ops.gemm(g.a0_d, g.w_d, g.out.views[0], **kw)
        ws.guard("split-K workspace")
        if splits == 1:
            assert ws.untouched(), "a one-split launch wrote to the workspace"
    ref, slack, _ = g.reference(splits=splits)
    g.check("out", ref, slack)


def case_gemm_batched(ops, dev, cfg, zero="outer"):
    """The engines' per-head form: batch = 6 = 2 images x 3 heads (batch_inner = 3), A = q[:, :64] slices with a_strides = (M ld, 64),
    output slice dqk[:, inner:inner + 64] with o_strides = (M ld, 64).  ``zero`` = "outer": W = k[:, :64] with w_strides = (0, 64) (the
    images share the keys, one slice per head); "inner": w_strides = (N ldw, 0) (one weight matrix per image, shared by its heads)."""
    imgs, heads, M, N, alpha = 2, 3, 40, 64, 0.125
    inner = heads * 64
    q = rnd(imgs * M, inner, seed=1)
    k = rnd(N, inner, seed=2, scale=0.125) if zero == "outer" else rnd(imgs * N, 64, seed=2, scale=0.125)
    lda, ldw, ldo = inner + 16, k.shape[1] + 24, 2 * inner + 8
    q_d, k_d = inbuf(q, lda, dev, col0=8), inbuf(k, ldw, dev, col0=16)
    out = Out(imgs * M, ldo, [(inner, 2 * inner)], dev)
    ops.gemm(q_d[:M, :64], k_d[:N, :64], out.views[0][:M, :64], M=M, N=N, alpha=alpha, batch=imgs * heads, batch_inner=heads,
             a_strides=(M * lda, 64), w_strides=(0, 64) if zero == "outer" else (N * ldw, 0), o_strides=(M * ldo, 64), tile_cfg=cfg)
    got = out.check("dqk")[0]
    wsel = (lambda i, hd: k[:, 64 * hd:64 * hd + 64]) if zero == "outer" else (lambda i, hd: k[i * N:(i + 1) * N])
    ref = torch.cat([torch.cat([alpha * q[i * M:(i + 1) * M, 64 * hd:64 * hd + 64] @ wsel(i, hd).t() for hd in range(heads)], dim=1)
                     for i in range(imgs)])
    dot = torch.cat([torch.cat([q[i * M:(i + 1) * M, 64 * hd:64 * hd + 64].abs() @ wsel(i, hd).abs().t() for hd in range(heads)], dim=1)
                     for i in range(imgs)])
    close_rc("out", got, ref, bfr(ref), BF16_TOL)
    elem("out", got, ref, 2.0 * 65 * EPS24 * alpha * dot)


def case_act_probe(ops, dev):
    """The approximation error of the epilogue activations alone: A = I (64 x 64) and weights whose rows hold one probe value each make
    the fp32 product EXACTLY that value (value row: 1); fp32 output = fast_gelu / silu of it.  Every bf16 value in [-8, 8] (the cases' gates and
    SiLU arguments stay inside: beyond the polynomial's clamp at 4.5 the error grows as 3.4e-6 |x|)."""
    vals = torch.arange(-(2 ** 15), 2 ** 15, dtype=torch.int32).to(torch.int16).view(BF).double()
    vals = vals[torch.isfinite(vals) & (vals.abs() <= 8.0)]
    n = (vals.numel() + 63) // 64 * 64
    x = torch.zeros(n, dtype=torch.float64)
    x[:vals.numel()] = vals
    eye = torch.zeros(64, 64, dtype=torch.float64)
    eye[torch.arange(64), torch.arange(64)] = 1.0
    worst = {}
    for name, act, fn in (("gelu", nt.ACT_GEGLU, gelu64), ("silu", nt.ACT_SILU, silu64)):
        err = 0.0
        for c in range(0, n, 2048):
            xs = x[c:c + 2048]
            m = xs.numel()
            if act == nt.ACT_GEGLU:   # groups of 64 rows: 32 value rows (column 0 = 1) | 32 gate rows (column 0 = the probe)
                wt = torch.zeros(m // 32, 2, 32, 64, dtype=torch.float64)
                wt[:, 0, :, 0], wt[:, 1, :, 0] = 1.0, xs.reshape(-1, 32)
                wt = wt.reshape(2 * m, 64)
            else:
                wt = torch.zeros(m, 64, dtype=torch.float64)
                wt[:, 0] = xs
            out = Out(64, m + 8, [(4, 4 + m)], dev, F32)
            ops.gemm(inbuf(eye, 80, dev, col0=8), inbuf(wt, 80, dev, col0=8), out.views[0], M=64, N=wt.shape[0], act=act, tile_cfg=4)
            got = out.check("probe")[0][0].double()
            err = max(err, float((got - fn(xs)).abs().max()))
            lim = 2.0 * ACT_ERR[name]   # (what the element checks allow)
            assert bool(((got - fn(xs)).abs() <= lim).all()), f"{name}: approximation error {float((got - fn(xs)).abs().max()):.3e} at some probe"
        worst[name] = err
        REPORT.append((_CUR[0], name + " abs err", 0.0, ACT_ERR[name], err))


# ------------------------------------------------------------------------------------------------------------------ fused epilogues
def _fuse_ok(ops, g, **kw):
    assert ops.gemm_fuse_supported(g.a0_d, g.w_d, g.out.views[0], **kw), "t2v_gemm_fuse_supported says no on a tile that carries the epilogue"


def case_rowstat(ops, dev, cfg, M=77, N=96, c0=64):
    """rowstat_out [M][ld_rowstat > N / 16]: (sum, sum of squares) per 32-column block of the fp32 epilogue values."""
    g = Gemm(dev, M=M, N=N, c0=c0, rowvec_div=7, residual=True, seed=11)
    nb = N // 32
    rs = Out(M, (2 * nb + 7) // 4 * 4, [(0, 2 * nb)], dev, F32)
    kw = g.kw(tile_cfg=cfg, rowstat=rs.views[0])
    _fuse_ok(ops, g, **kw)
    ops.gemm(g.a0_d, g.w_d, g.out.views[0], **kw)
    ref, slack, v = g.reference()
    g.check("out", ref, slack)
    blk = v.reshape(M, nb, 32)
    st = torch.stack([blk.sum(dim=2), (blk * blk).sum(dim=2)], dim=2).reshape(M, 2 * nb)
    blk_r = f32r(v).reshape(M, nb, 32)
    st_r = f32r(torch.stack([blk_r.sum(dim=2), (blk_r * blk_r).sum(dim=2)], dim=2).reshape(M, 2 * nb))
    close_rc("rowstat", rs.check("rowstat")[0], st, st_r, STAT_TOL)


def case_colstat(ops, dev, cfg, M=64, N=96, c0=64, act=nt.ACT_NONE):
    """colstat_out [M / 32][N][2]: (sum, sum of squares) per column and 32-row slab of the bf16-ROUNDED outputs."""
    g = Gemm(dev, M=M, N=N, c0=c0, residual=True, act=act, seed=12)
    cs = Out(1, M // 32 * N * 2 + 8, [(0, M // 32 * N * 2)], dev, F32, pre=1, post=1)
    kw = g.kw(tile_cfg=cfg, colstat=cs.views[0].reshape(M // 32, N, 2))
    _fuse_ok(ops, g, **kw)
    ops.gemm(g.a0_d, g.w_d, g.out.views[0], **kw)
    ref, slack, _ = g.reference()
    got = g.check("out", ref, slack)
    _colstat_check(cs, got, ref, M, N)


def _colstat_check(cs, got, ref, M, N):
    """Against the fp64 sums of the bf16-rounded REFERENCE within the statistics tolerance widened by what one bf16 rounding flip per
    element can move a sum, and against the sums of the outputs the kernel itself stored within STAT_TOL."""
    st = cs.check("colstat")[0].reshape(M // 32, N, 2)
    y = got.double().reshape(M // 32, 32, N)
    own = torch.stack([y.sum(dim=1), (y * y).sum(dim=1)], dim=2)
    close_rc("colstat", st.reshape(-1, 2 * N), own.reshape(-1, 2 * N), f32r(own).reshape(-1, 2 * N), STAT_TOL)
    yr = bfr(ref).reshape(M // 32, 32, N)
    want = torch.stack([yr.sum(dim=1), (yr * yr).sum(dim=1)], dim=2)
    close("colstat vs reference", st.reshape(-1, 2 * N), want.reshape(-1, 2 * N), f32r(want).reshape(-1, 2 * N), BF16_TOL)


def case_lnf(ops, dev, cfg, M=77, N=128, C=128, act=nt.ACT_NONE):
    """lnf_*: this launch consumes LayerNorm(x) from the producer's per-32-column (sum, sum of squares) pairs: mean = S1 / C,
    var = max(S2 / C - mean^2, 0), out = rstd (acc - mean lnf_s[n]) + bias[n]; lnf_stats a row-strided view, lnf_s in a NaN-padded flat."""
    g = Gemm(dev, M=M, N=N, c0=C, act=act, seed=13, ashift=0.5)
    nb = C // 32
    blk = g.a.reshape(M, nb, 32)
    stats = f32r(torch.stack([blk.sum(dim=2), (blk * blk).sum(dim=2)], dim=2).reshape(M, 2 * nb))
    s_vec = f32r(g.wt.sum(dim=1))
    eps = 1e-5
    mean = stats[:, 0::2].sum(dim=1) / C
    rstd = 1.0 / torch.sqrt((stats[:, 1::2].sum(dim=1) / C - mean * mean).clamp_min(0.0) + eps)
    kw = g.kw(tile_cfg=cfg, lnf=(inbuf(stats, 2 * nb + 8, dev, F32, col0=4), eps, inflat(s_vec, dev)))
    _fuse_ok(ops, g, **kw)
    ops.gemm(g.a0_d, g.w_d, g.out.views[0], **kw)
    ref, slack, _ = g.reference(lnf=(mean, rstd, s_vec))
    g.check("out", ref, slack)


def case_ln_out(ops, dev, M=77, K=64):
    """ln_out (N == 320, the 160x320 tile): LayerNorm of the fp32 epilogue values as a second output at ld_ln_out > 320."""
    N = 320
    g = Gemm(dev, M=M, N=N, c0=K, rowvec_div=7, residual=True, seed=14)
    gamma, beta = f32r(rnd(N, seed=21, scale=0.2, shift=1.0)), f32r(rnd(N, seed=22, scale=0.1))
    ln = Out(M, N + 16, [(8, 8 + N)], dev)
    ops.gemm(g.a0_d, g.w_d, g.out.views[0], **g.kw(ln=(inflat(gamma, dev), inflat(beta, dev), 1e-5, ln.views[0])))
    ref, slack, v = g.reference()
    g.check("out", ref, slack)
    ln_ref = F.layer_norm(v, (N,), gamma, beta, 1e-5)
    close_rc("ln_out", ln.check("ln_out")[0], ln_ref, bfr(F.layer_norm(f32r(v), (N,), gamma, beta, 1e-5)), BF16_TOL)


def case_gemm_dropout(ops, dev, cfg, p, residual=True, generic=False, M=200, N=96, K=64):
    """The dropout epilogue (drop_col0 = 64 inside drop_ncols = 192): out = keep ? (alpha acc + bias) / (1 - p') : 0, + residual.  The
    zero pattern must be the header formula's, bit for bit, and t2v_dropout_bf16's over the same [M][192] matrix.  ``generic``: alpha != 1
    and a row vector keep the launch on the generic kernel; otherwise it rides on the fast kernel of the tile (ids 4, 5, 23 have one)."""
    ncols, col0, site = 192, 64, 5
    g = Gemm(dev, M=M, N=N, c0=K, residual=residual, alpha=0.5 if generic else 1.0, rowvec_div=7 if generic else 0, seed=15, wscale=1.0)
    seed_d = seed_tensor(dev)
    keep = keep_mask(0x1234_5678_9ABC, site, M, ncols, p)
    ops.gemm(g.a0_d, g.w_d, g.out.views[0], **g.kw(tile_cfg=cfg, dropout=(p, seed_d, site, ncols, col0)))
    kp = keep[:, col0:col0 + N] if drop_thr16(p) else torch.ones(M, N, dtype=torch.bool)
    ref, slack, _ = g.reference(keep=kp, p_drop=p)
    got = g.check("out", ref, slack)
    # which elements are dropped: exactly 0 (or exactly the residual) there, and nowhere else (|alpha acc + bias| > 0 on the kept ones)
    base = g.res if residual else torch.zeros(M, N, dtype=torch.float64)
    if generic:
        base = base + g.rv[torch.arange(M) // 7]
    same_pattern("dropped pattern", got, base, g.reference(keep=torch.ones_like(kp), p_drop=p)[0] - base, kp)
    # the standalone kernel over the whole [M][ncols] matrix draws the same mask
    x = rnd(M, ncols, seed=16).abs() + 0.5
    o2 = Out(M, ncols + 8, [(0, ncols)], dev)
    ops.dropout(inbuf(x, ncols + 16, dev, col0=8), None, o2.views[0], ncols, p, seed_d, site)
    same_pattern("t2v_dropout_bf16 pattern", o2.check("dropout")[0], torch.zeros_like(x), x, keep if drop_thr16(p) else torch.ones_like(keep))


def case_gemm_lora(ops, dev, cfg, leaves, p, colstat=False, M=200, K=128, N=96):
    """The LoRA epilogue: out = acc + bias + residual + lora_scale * dropout(t_l u_n^T); lora_t [M][64 leaves] and lora_u [N][64] views
    with longer strides, the rank columns [rank, 64) of lora_u hold zero (read), everything beyond column 64 NaN."""
    n_leaf, rank, scale, ncols, col0, site = N // leaves, 48, 0.75, N + 32, 16, 9
    g = Gemm(dev, M=M, N=N, c0=K, residual=True, seed=17)
    t = rnd(M, 64 * leaves, seed=31)
    u = rnd(N, 64, seed=32, scale=0.2)
    u[:, rank:] = 0.0
    t_d, u_d = inbuf(t, 64 * leaves + 16, dev, col0=8), inbuf(u, 80, dev, col0=8)
    seed_d = seed_tensor(dev)
    kw = g.kw(tile_cfg=cfg, lora=(t_d, u_d, n_leaf, scale), dropout=(p, seed_d, site, ncols, col0) if p else None)
    cs = None
    if colstat:
        cs = Out(1, M // 32 * N * 2 + 8, [(0, M // 32 * N * 2)], dev, F32, pre=1, post=1)
        kw["colstat"] = cs.views[0].reshape(M // 32, N, 2)
    _fuse_ok(ops, g, **kw)
    ops.gemm(g.a0_d, g.w_d, g.out.views[0], **kw)
    keep = keep_mask(0x1234_5678_9ABC, site, M, ncols, p)[:, col0:col0 + N] if p and drop_thr16(p) else None
    ref, slack, _ = g.reference(keep=keep, p_drop=p, lora=(t, u, n_leaf, scale))
    got = g.check("out", ref, slack)
    if cs is not None:
        _colstat_check(cs, got, ref, M, N)


# ------------------------------------------------------------------------------------------------------------------ t2v_conv_halo
def case_conv_halo(ops, dev, cfg, h, w, c0, N, c1=0, n_img=2, ups=0, residual=False, rowvec=False, act=nt.ACT_NONE, colstat=False):
    """t2v_conv_halo on tile ``cfg``: the slab-major pack at ldw > t2v_conv_halo_pack_cols(C) (zeros up to it: read; NaN beyond), spare
    NaN rows before the first image and after the last, residual at ldr != ldo; launched twice into the same output: same bits."""
    mode = nt.GEMM_CONV3X3_UP2 if ups else nt.GEMM_CONV3X3
    M = (n_img * h * w) << (2 * ups)
    div = (h * w) << (2 * ups)
    g = Gemm(dev, M=M, N=N, c0=c0, c1=c1, mode=mode, n_img=n_img, h=h, w=w, rowvec_div=div if rowvec else 0, residual=residual, act=act,
             seed=40 + cfg)
    pack = nt.pack_conv_slab(g.wt.to(BF)).double()
    assert pack.shape[1] == nt.conv_halo_pack_cols(c0 + c1)
    w_d = inbuf(pack, pack.shape[1] + 16, dev, col0=8)
    kw = g.kw(tile_cfg=cfg)
    cs = None
    if colstat:
        cs = Out(1, M // 32 * N * 2 + 8, [(0, M // 32 * N * 2)], dev, F32, pre=1, post=1)
        kw["colstat"] = cs.views[0].reshape(M // 32, N, 2)
    assert ops.conv_halo_supported(g.a0_d, w_d, g.out.views[0], **kw) == 1, "the halo kernel does not take the case"
    ops.conv_halo(g.a0_d, w_d, g.out.views[0], **kw)
    ref, slack, _ = g.reference()
    got = g.check("out", ref, slack)
    if cs is not None:
        _colstat_check(cs, got, ref, M, N)
        first = cs.full.cpu().clone()
    ops.conv_halo(g.a0_d, w_d, g.out.views[0], **kw)
    exact("second launch", g.out.check("out")[0], got)
    if cs is not None:
        exact("second launch colstat", cs.full.cpu(), first)


# ------------------------------------------------------------------------------------------------------------------ t2v_linear_pr
def case_linear_pr(ops, dev, M, K, N, ny=0, act=nt.ACT_NONE, residual=False, ln_in=False, gn_rpu=0, bias=True):
    """t2v_linear_pr: A at lda > K with NaN gaps, out at ldo > n_out, residual at ldr != ldo, sentinel rows after M; ``ny`` forces the
    column split.  ln_in / gn_coef: the normalised rows enter the product rounded to bf16 (t2v_hip.h)."""
    g = Gemm(dev, M=M, N=N, c0=K, act=act, residual=residual, bias=bias, seed=50 + ny, ashift=0.25 if (ln_in or gn_rpu) else 0.0)
    wp_d = inflat(nt.pack_linear_pr(g.wt.to(BF)), dev, BF, pad=8)
    kw = g.kw()
    kw.pop("rowvec"), kw.pop("rowvec_div")
    a_eff = g.a
    if ln_in:
        gamma, beta = f32r(rnd(K, seed=61, scale=0.2, shift=1.0)), f32r(rnd(K, seed=62, scale=0.3))
        kw["ln_in"] = (inflat(gamma, dev), inflat(beta, dev), 1e-5)
        a_eff = bfr(F.layer_norm(g.a, (K,), gamma, beta, 1e-5))
    if gn_rpu:
        units = M // gn_rpu
        coef = f32r(torch.stack([rnd(units, K, seed=63, scale=0.3, shift=1.0), rnd(units, K, seed=64, scale=0.5)], dim=1))
        kw["gn_in"] = (inflat(coef, dev), gn_rpu)
        u = torch.arange(M) // gn_rpu
        a_eff = bfr(g.a * coef[u, 0] + coef[u, 1])
    ops.lib.t2v_linear_pr_force_split(ny)
    try:
        assert ops.linear_pr_supported(g.a0_d, wp_d, g.out.views[0], **kw) == 1, "the panel-resident kernel does not take the case"
        ops.linear_pr(g.a0_d, wp_d, g.out.views[0], **kw)
    finally:
        ops.lib.t2v_linear_pr_force_split(0)
    raw, g.a = g.a, a_eff
    ref, slack, _ = g.reference()
    g.a = raw
    if ln_in or gn_rpu:   # a normalised element within half a bf16 ulp of a rounding boundary may round the other way in fp32: the row /
        got = g.out.check("out")[0]   # column metric carries these cases (the element bound has no term for a flipped input bit)
        close_rc("out", got, ref, bfr(ref), BF16_TOL)
    else:
        g.check("out", ref, slack)


# ------------------------------------------------------------------------------------------------------------------ t2v_wgrad_tn
def _wgrad_ref(a, b, alpha, splits):
    ref = alpha * (a.t() @ b)
    return ref, 2.0 * (a.shape[0] + splits) * EPS24 * abs(alpha) * (a.abs().t() @ b.abs())


def case_wgrad(ops, dev, M, R, C, splits, aligned=True, alpha=0.5):
    """out [R][C] = alpha a^T b: a, b views with lda > R, ldb > C and NaN rows after M (a read past M poisons every output); out at
    ldo > C, 16-byte aligned or 4 bytes off; the workspace holds exactly max(splits, 1) slabs; a second launch gives the same bits."""
    a, b = rnd(M, R, seed=1, scale=0.5), rnd(M, C, seed=2, scale=0.5)
    a_d, b_d = inbuf(a, (R + 23) // 8 * 8, dev, col0=8), inbuf(b, (C + 31) // 8 * 8, dev, col0=16)
    out = Out(R, C + (8 if aligned else 3), [(4, 4 + C)] if aligned else [(1, 1 + C)], dev, F32)
    slabs = splits or 8          # (splits = 0: the library's choice, shrunk to the workspace it is given)
    with Workspace(ops, dev, (slabs * R * C + 3) // 4 * 4) as ws:
        ops.wgrad_tn(a_d, b_d, out.views[0], alpha=alpha, splits=splits)
        got = out.check("out")[0]
        ws.guard("wgrad workspace")
        if splits == 1:
            assert ws.untouched(), "a one-split launch wrote to the workspace"
        ops.wgrad_tn(a_d, b_d, out.views[0], alpha=alpha, splits=splits)
        exact("second launch", out.check("out")[0], got)
        ws.guard("wgrad workspace")
    ref, slack = _wgrad_ref(a, b, alpha, slabs)
    close_rc("out", got, ref, f32r(ref), WGRAD_TOL)
    elem("out", got, ref, slack, 0.0)


def case_wgrad_group(ops, dev, M=150):
    """One LoRA group: dU of 3 leaves (a = dy[:, 72 l : 72 l + 72], b = t[:, 64 l : 64 l + 64]) and dD (a = g, b = x), distinct alphas,
    the four outputs slices of one fp32 arena; NaN rows after M in every operand."""
    dy, t, gg, x = rnd(M, 216, seed=1, scale=0.5), rnd(M, 192, seed=2, scale=0.5), rnd(M, 192, seed=3, scale=0.5), rnd(M, 72, seed=4, scale=0.5)
    dy_d, t_d, g_d, x_d = inbuf(dy, 232, dev, col0=8), inbuf(t, 208, dev, col0=8), inbuf(gg, 216, dev, col0=16), inbuf(x, 88, dev, col0=8)
    regions = [(1, 73, 3 + 70 * l, 3 + 70 * l + 64) for l in range(3)] + [(80, 272, 5, 77)]
    arena = Arena(274, 216, regions, dev)
    alphas = [0.5, 1.0, -2.0, 0.25]
    probs = [(dy_d[:, 72 * l:72 * l + 72], t_d[:, 64 * l:64 * l + 64], arena.views[l], alphas[l]) for l in range(3)]
    probs.append((g_d, x_d, arena.views[3], alphas[3]))
    with Workspace(ops, dev, 1 << 20) as ws:
        ops.wgrad_tn_group(probs)
        got = arena.check("group")
        ws.guard("wgrad group workspace")
        ops.wgrad_tn_group(probs)
        for i, (o, o2) in enumerate(zip(got, arena.check("group"))):
            exact("group second launch", o2, o)
    pairs = [(dy[:, 72 * l:72 * l + 72], t[:, 64 * l:64 * l + 64]) for l in range(3)] + [(gg, x)]
    for i, ((a, b), al) in enumerate(zip(pairs, alphas)):
        ref, slack = _wgrad_ref(a, b, al, 4)
        close_rc("group out", got[i], ref, f32r(ref), WGRAD_TOL)
        elem("group out", got[i], ref, slack, 0.0)


# ------------------------------------------------------------------------------------------------------------------ small kernels
def case_conv_small_cin(ops, dev, cin, cout):
    """t2v_conv3x3_small_cin on 2 x (9 x 11): the ABI has no strides, so the operands are contiguous rows between NaN / sentinel rows."""
    n_img, h, w = 2, 9, 11
    M = n_img * h * w
    x, wt, b = rnd(M, cin, seed=1), f32r(rnd(cout, 9 * cin, seed=2, scale=(9 * cin) ** -0.5)), f32r(rnd(cout, seed=3))
    out = Out(M, cout, [(0, cout)], dev, pre=4, post=4)
    ops.conv_small(inbuf(x, cin, dev, pre=4, post=4), n_img, h, w, inflat(wt, dev), inflat(b, dev), out.views[0])
    G = gather(x, nt.GEMM_CONV3X3, n_img, h, w)
    ref = G @ wt.t() + b
    got = out.check("out")[0]
    close_rc("out", got, ref, bfr(ref), BF16_TOL)
    elem("out", got, ref, 2.0 * (9 * cin + 1) * EPS24 * (G.abs() @ wt.abs().t()) + 8.0 * EPS24 * b.abs())


def case_dropout(ops, dev, inplace, residual, p=0.1, vec=True):
    """t2v_dropout_bf16: ldx != ldr != ldo, ncols smaller than every stride; in place (out == x) and out of place."""
    rows, ncols, site = 37, 72 if vec else 70, 3
    x = (rnd(rows, ncols, seed=1).abs() + 0.5) * torch.where(rnd(rows, ncols, seed=2) > 0, 1.0, -1.0)
    r = rnd(rows, ncols, seed=3) if residual else None
    step = 8 if vec else 2
    out = Out(rows, ncols + 2 * step, [(step, step + ncols)], dev, init=[x] if inplace else None)
    x_d = out.views[0] if inplace else inbuf(x, ncols + 3 * step, dev, col0=step)
    r_d = None if r is None else inbuf(r, ncols + 4 * step, dev, col0=2 * step)
    seed_d = seed_tensor(dev, 77)
    ops.dropout(x_d, r_d, out.views[0], ncols, p, seed_d, site)
    keep = keep_mask(77, site, rows, ncols, p)
    ref = torch.where(keep, x * inv_keep(p), torch.zeros_like(x)) + (0 if r is None else r)
    got = out.check("out")[0]
    close_rc("out", got, ref, bfr(ref), BF16_TOL)
    same_pattern("dropped pattern", got, r if residual else torch.zeros_like(x), x, keep)


def case_repack(ops, dev, kind, taps):
    """t2v_repack_conv_f32: exact, ldo > the pack row, the fp32 parameter inside a NaN-padded flat."""
    N, C = 24, 40
    wt = torch.randn(N, C, taps, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    if kind == 0:
        ref = wt.permute(0, 2, 1).reshape(N, taps * C)
    else:
        ref = wt.flip(2).permute(1, 2, 0).reshape(C, taps * N)
    out = Out(ref.shape[0], ref.shape[1] + 10, [(2, 2 + ref.shape[1])], dev)
    ops.repack_conv(inflat(wt, dev), out.views[0], kind)
    exact("pack", out.check("pack")[0], ref.to(BF))


def case_experimental(ops, dev, which):
    """The experimental entry points, where the loaded library exports them (the device file lists them as absent-by-design)."""
    if which == "gemm2":
        g = Gemm(dev, M=200, N=160, c0=128, residual=True, seed=71)
        ops.gemm(g.a0_d, g.w_d, g.out.views[0], **g.kw(tile_cfg=51))
        ref, slack, _ = g.reference()
        g.check("out", ref, slack)
    else:   # ffn_fused at C = 64
        C, M = 64, 70
        x = rnd(M, C, seed=1)
        w1, b1 = rnd(8 * C, C, seed=2, scale=C ** -0.5), f32r(rnd(8 * C, seed=3, scale=0.1))
        w2, b2 = rnd(C, 4 * C, seed=4, scale=(4 * C) ** -0.5), f32r(rnd(C, seed=5, scale=0.1))
        gamma, beta = f32r(rnd(C, seed=6, scale=0.2, shift=1.0)), f32r(rnd(C, seed=7, scale=0.1))
        w1p, b1p, w2p, b2p = nt.ffn_pack(w1.float(), b1.float(), w2.float(), b2.float(), gamma.float(), beta.float(), BF)
        out = Out(M, C + 8, [(0, C)], dev)
        ops.ffn_fused(inbuf(x, C + 8, dev), w1p.to(dev), b1p.to(dev), w2p.to(dev), b2p.to(dev), 1e-5, out.views[0])
        hdn = F.layer_norm(x, (C,), gamma, beta, 1e-5) @ w1.t() + b1
        ref = x + (hdn[:, :4 * C] * gelu64(hdn[:, 4 * C:])) @ w2.t() + b2
        close_rc("out", out.check("out")[0], ref, bfr(ref), BWD_TOL)


EXPERIMENTAL_ENTRIES = {"gemm2": "t2v_gemm2_enable", "ffn_fused": "t2v_ffn_fused"}


# ------------------------------------------------------------------------------------------------------------------ refusals
def gemm_refusal_cases(ops, dev):
    """-> [(name, thunk)]: ONE call each that the entry point must refuse before any launch, the sentinel-filled outputs untouched."""
    cases = []
    M, K = 6, 64
    f32v = lambda n, s=0: inflat(f32r(rnd(n, seed=s + 20)), dev)  # noqa: E731
    xb = lambda rows, cols, ld, dt=BF: inbuf(rnd(rows, cols, seed=9), ld, dev, dt)  # noqa: E731

    def mk(name, build):
        def thunk():
            call, outs = build()
            refuses(ops, call, *outs)
        cases.append((name, thunk))

    def gm(entry, **bad):
        """entry: gemm / fuse / plan / conv_halo / conv_halo_supported / linear_pr / linear_pr_supported."""
        def build():
            halo, lpr = entry.startswith("conv_halo"), entry.startswith("linear_pr")
            Kc, Mc = (320, M) if lpr else (K, 32 if halo else M)
            s = dict(lda0=Kc + 8, lda1=72, ldo=0, ldr=0, ld_rowvec=0, ld_ln=0, ld_lora_t=72, ld_lora_u=72, geglu=False)
            s.update(bad)
            N = 128 if s["geglu"] else (320 if "ld_ln" in bad else 64)   # (ln_out: N == 320 with valid arguments, the stride the only fault)
            a0 = _with_stride(xb(Mc, Kc, Kc + 8), s["lda0"])
            kw = dict(M=Mc, N=N, tile_cfg=4, bias=f32v(N))
            if "lda1" in bad:
                kw["a1"] = _with_stride(xb(Mc, 64, 72), s["lda1"])
            if halo:
                kw.update(mode=nt.GEMM_CONV3X3, n_img=1, h=2, wd=16, tile_cfg=0)
            taps = 9 if halo else 1
            c_tot = Kc + (64 if "lda1" in bad else 0)
            wt = xb(N, nt.conv_halo_pack_cols(c_tot) if halo else taps * c_tot, (nt.conv_halo_pack_cols(c_tot) if halo else taps * c_tot) + 8)
            if lpr:
                wt = inflat(rnd(N * Kc, seed=3), dev, BF, pad=8).view(N, Kc)
            n_out = N // 2 if s["geglu"] else N
            out = Out(Mc, N + 8, [(0, n_out)], dev)
            outs = [out]
            if s["geglu"]:
                kw["act"] = nt.ACT_GEGLU
            if "ldr" in bad:
                kw["residual"] = _with_stride(xb(Mc, N, N + 8), s["ldr"])
            if "ld_rowvec" in bad:
                kw.update(rowvec=_with_stride(xb(1, N, N + 4, F32), s["ld_rowvec"]), rowvec_div=Mc)
            if "ld_ln" in bad:
                ln = Out(Mc, N + 8, [(0, N)], dev)
                outs.append(ln)
                kw["ln"] = (f32v(N, 1), f32v(N, 2), 1e-5, _with_stride(ln.views[0], s["ld_ln"]))
            if "ld_lora_t" in bad or "ld_lora_u" in bad:
                kw["lora"] = (_with_stride(xb(Mc, 64, 72), s["ld_lora_t"]), _with_stride(xb(N, 64, 72), s["ld_lora_u"]), N, 1.0)
            o = _with_stride(out.views[0], s["ldo"] or N + 8)
            fn = {"gemm": ops.gemm, "fuse": ops.gemm_fuse_supported, "plan": ops.gemm_plan, "conv_halo": ops.conv_halo,
                  "conv_halo_supported": ops.conv_halo_supported, "linear_pr": ops.linear_pr, "linear_pr_supported": ops.linear_pr_supported}[entry]
            return (lambda: fn(a0, wt, o, **kw)), outs
        return build

    for entry in ("gemm", "fuse", "plan"):
        mk(f"{entry} lda0 < c0", gm(entry, lda0=56))
        mk(f"{entry} lda1 < c1", gm(entry, lda1=56))
        mk(f"{entry} ldo < n_out", gm(entry, ldo=56))
        mk(f"{entry} ldr < n_out", gm(entry, ldr=56))
        mk(f"{entry} ld_rowvec < n_out", gm(entry, ld_rowvec=60))
        mk(f"{entry} ld_lora_t < 64 leaves", gm(entry, ld_lora_t=56))
        mk(f"{entry} ld_lora_u < 64", gm(entry, ld_lora_u=56))
    mk("gemm GEGLU ldo < N / 2", gm("gemm", ldo=56, geglu=True))
    mk("gemm ld_ln_out < N", gm("gemm", ld_ln=312))
    mk("plan ld_ln_out < N", gm("plan", ld_ln=312))
    # kept from before: misaligned base, ldw < K, bad dropout geometry, two fused statistics, ln_in on t2v_gemm

    def old(which):
        def build():
            N, Mo = 64, (32 if which == "rowstat + colstat" else M)
            a0, wt, out = xb(Mo, K, K + 8), xb(N, K, K + 8), Out(Mo, N + 8, [(0, N)], dev)
            kw = dict(M=Mo, N=N, tile_cfg=4)
            if which == "misaligned a0":
                a0 = torch.as_strided(a0, (M, K), (K + 8, 1), a0.storage_offset() + 4)
            elif which == "ldw < K":
                wt = _with_stride(wt, 56)
            elif which == "dropout col0 + N > ncols":
                kw["dropout"] = (0.1, seed_tensor(dev), 1, N, 4)
            elif which == "ln_in":
                kw["ln_in"] = (f32v(K, 1), f32v(K, 2), 1e-5)
            elif which == "rowstat + colstat":   # more than one fused statistic per launch
                rs, cs = Out(Mo, 8, [(0, 4)], dev, F32), Out(1, N * 2 + 8, [(0, N * 2)], dev, F32, pre=1, post=1)
                kw.update(rowstat=rs.views[0], colstat=cs.views[0].reshape(1, N, 2))
                return (lambda: ops.gemm(a0, wt, out.views[0], **kw)), [out, rs, cs]
            return (lambda: ops.gemm(a0, wt, out.views[0], **kw)), [out]
        return build

    for which in ("misaligned a0", "ldw < K", "dropout col0 + N > ncols", "ln_in", "rowstat + colstat"):
        mk(f"gemm {which}", old(which))
    for entry in ("conv_halo", "conv_halo_supported", "linear_pr", "linear_pr_supported"):
        mk(f"{entry} lda0 < c0", gm(entry, lda0=56))
        mk(f"{entry} ldo < n_out", gm(entry, ldo=56))
        mk(f"{entry} ldr < n_out", gm(entry, ldr=56))
        mk(f"{entry} lda1 < c1", gm(entry, lda1=56))
        mk(f"{entry} ld_rowvec < n_out", gm(entry, ld_rowvec=60))

    def wg(group, lda=72, ldb=72, ldo=68):
        def build():
            a, b = _with_stride(xb(M, 64, 72), lda), _with_stride(xb(M, 64, 72), ldb)
            out = Out(64, 68, [(0, 64)], dev, F32)
            o = _with_stride(out.views[0], ldo)
            if group:
                return (lambda: ops.wgrad_tn_group([(a, b, o, 1.0)])), [out]
            return (lambda: ops.wgrad_tn(a, b, o)), [out]
        return build

    for group in (False, True):
        nm = "wgrad_tn_group" if group else "wgrad_tn"
        mk(f"{nm} lda < R", wg(group, lda=56))
        mk(f"{nm} ldb < C", wg(group, ldb=56))
        mk(f"{nm} ldo < C", wg(group, ldo=60))

    def dr(ldx=72, ldr=72, ldo=72):
        def build():
            out = Out(M, 72, [(0, 64)], dev)
            return (lambda: ops.dropout(_with_stride(xb(M, 64, 72), ldx), _with_stride(xb(M, 64, 72), ldr), _with_stride(out.views[0], ldo), 64, 0.1,
                                        seed_tensor(dev), 1)), [out]
        return build

    mk("dropout ldx < ncols", dr(ldx=56))
    mk("dropout ldr < ncols", dr(ldr=56))
    mk("dropout ldo < ncols", dr(ldo=56))

    def rp(kind):
        def build():
            N_, C_, taps = 8, 16, 9
            cols = taps * (C_ if kind == 0 else N_)
            out = Out(N_ if kind == 0 else C_, cols + 8, [(0, cols)], dev)
            wt = inflat(torch.randn(N_, C_, taps), dev)
            return (lambda: ops.repack_conv(wt, _with_stride(out.views[0], cols - 8), kind)), [out]
        return build

    mk("repack_conv kind 0 ldo < taps * C", rp(0))
    mk("repack_conv kind 1 ldo < taps * N", rp(1))
    return cases


# ------------------------------------------------------------------------------------------------------------------ the table
_S1 = dict(M=77, N=96, c0=64, rowvec_div=7, residual=True)
_S2 = dict(M=130, N=72, c0=64, c1=128, rowvec_div=7, residual=True)
_MODES = {"linear": nt.GEMM_LINEAR, "conv3x3": nt.GEMM_CONV3X3, "conv3x3_s2": nt.GEMM_CONV3X3_S2, "conv3x3_up2": nt.GEMM_CONV3X3_UP2,
          "tconv3": nt.GEMM_TCONV3, "conv3x3_s2_pad01": nt.GEMM_CONV3X3_S2_PAD01}


def _mode_shape(name, grid):
    """Grid "5x7": 2 images of 5 x 7 with the virtual concat 64 + 128; grid "6x8": 2 images of 6 x 8, one 64-channel source.  TCONV3:
    2 clips x 4 frames x (3 x 5) in both.  N = 80: ragged against every tile."""
    mode = _MODES[name]
    ch = dict(c0=64, c1=128) if grid == "5x7" else dict(c0=64)
    if mode == nt.GEMM_LINEAR:
        return dict(M=70, N=80, mode=mode, **ch)
    geo = dict(n_img=8, h=3, w=5, frames=4) if mode == nt.GEMM_TCONV3 else dict(n_img=2, h=int(grid[0]), w=int(grid[2]))
    ho, wo = out_grid(mode, geo["n_img"], geo["h"], geo["w"])
    return dict(M=geo["n_img"] * ho * wo, N=80, mode=mode, residual=True, **ch, **geo)


def sweep_cases(ids):
    """The tile / store-path sweep for the given tile ids: 2 shapes x 3 output forms each."""
    c = []
    for cfg in ids:
        for sn, shape in (("77x96", _S1), ("130x72", _S2)):
            for form in ("vec", "scalar", "f32"):
                c.append((f"gemm-cfg{cfg}-{sn}-{form}", case_gemm, dict(cfg=cfg, out=form, seed=cfg, **shape)))
    return c


def gather_cases(ids):
    """The six gather modes with strided A on one id per tile class, on both grids."""
    c = []
    for cfg in ids:
        for mn in _MODES:
            for grid in ("5x7", "6x8"):
                c.append((f"gemm-cfg{cfg}-{mn}-{grid}", case_gemm, dict(cfg=cfg, seed=100 + cfg, **_mode_shape(mn, grid))))
    return c


def other_cases():
    c = []
    for cfg in (4, 18):
        for split in (2, 3, 5):
            c.append((f"gemm-splitk{split}-conv-cfg{cfg}", case_gemm, dict(cfg=cfg, split=split, expect_splits=split, M=80, N=64, c0=128, mode=nt.GEMM_CONV3X3,
                                                                          n_img=2, h=5, w=8, residual=True, rowvec_div=40, seed=split)))
            c.append((f"gemm-splitk{split}-linear-cfg{cfg}", case_gemm, dict(cfg=cfg, split=split, expect_splits=split, out="f32", M=100, N=64, c0=1280,
                                                                            residual=True, seed=split)))
        # the scalar store path cannot split (p.vec4 is part of can_split): the launch falls back to one split, the workspace is untouched
        c.append((f"gemm-splitk3-fallback-cfg{cfg}", case_gemm, dict(cfg=cfg, split=3, expect_splits=1, out="scalar", M=80, N=64, c0=1280, seed=9)))
        c.append((f"gemm-batched-cfg{cfg}", case_gemm_batched, dict(cfg=cfg)))
        c.append((f"gemm-batched-zero-inner-cfg{cfg}", case_gemm_batched, dict(cfg=cfg, zero="inner")))
    for cfg in (4, 11, 12, 22):   # (GEGLU needs 64-wide wave tiles: id 22 falls back to id 4 inside the library)
        c.append((f"gemm-geglu-cfg{cfg}", case_gemm, dict(cfg=cfg, M=150, N=256, c0=128, act=nt.ACT_GEGLU, seed=3)))
    c.append(("gemm-geglu-f32", case_gemm, dict(cfg=4, out="f32", M=150, N=256, c0=128, act=nt.ACT_GEGLU, seed=4)))
    for form in ("vec", "scalar", "f32"):
        c.append((f"gemm-silu-{form}", case_gemm, dict(cfg=5, out=form, M=130, N=96, c0=64, act=nt.ACT_SILU, residual=True, rowvec_div=7, seed=5)))
        c.append((f"gemm-alpha-{form}", case_gemm, dict(cfg=1, out=form, M=77, N=96, c0=128, alpha=0.125, residual=True, seed=6)))
        c.append((f"gemm-M2-{form}", case_gemm, dict(cfg=8, out=form, M=2, N=320, c0=64, residual=True, rowvec_div=1, seed=7)))
        c.append((f"gemm-N4-{form}", case_gemm, dict(cfg=2, out=form, M=150, N=4, c0=64, residual=True, alpha=0.5, seed=8)))
    c.append(("gemm-act-probe", case_act_probe, {}))
    return c


def fused_cases():
    c = []
    for cfg in (4, 7, 23):
        c.append((f"gemm-rowstat-cfg{cfg}", case_rowstat, dict(cfg=cfg)))
        for M in (64, 96):
            c.append((f"gemm-colstat-M{M}-cfg{cfg}", case_colstat, dict(cfg=cfg, M=M)))
        c.append((f"gemm-lnf-cfg{cfg}", case_lnf, dict(cfg=cfg)))
    c.append(("gemm-colstat-silu", case_colstat, dict(cfg=4, M=64, act=nt.ACT_SILU)))
    c.append(("gemm-lnf-geglu", case_lnf, dict(cfg=4, act=nt.ACT_GEGLU)))
    c.append(("gemm-ln_out-M77", case_ln_out, dict(M=77)))
    c.append(("gemm-ln_out-M320", case_ln_out, dict(M=320, K=128)))
    for cfg in (4, 5, 23):   # the fast kernel where the tile has a fused twin (4, 23), the generic one otherwise (5)
        for p in (0.1, 1e-5):
            c.append((f"gemm-dropout-p{p}-cfg{cfg}", case_gemm_dropout, dict(cfg=cfg, p=p)))
            if cfg != 23:
                c.append((f"gemm-dropout-p{p}-cfg{cfg}-generic", case_gemm_dropout, dict(cfg=cfg, p=p, generic=True)))
    c.append(("gemm-dropout-noresidual", case_gemm_dropout, dict(cfg=5, p=0.1, residual=False)))
    # (a wave tile may span two leaves at most: the 160-wide wave tiles of id 23 take one 96-column leaf, not three of 32)
    for cfg, leaves in ((4, 3), (4, 1), (7, 3), (23, 1)):
        for p in (0.0, 0.1):
            c.append((f"gemm-lora-{leaves}leaves-p{p}-cfg{cfg}", case_gemm_lora, dict(cfg=cfg, leaves=leaves, p=p)))
    c.append(("gemm-lora-colstat", case_gemm_lora, dict(cfg=4, leaves=3, p=0.1, colstat=True, M=192)))
    return c


def halo_cases():
    c = []
    for cfg in (40, 41, 42, 43, 44):
        w, h = (16 if cfg == 42 else 32), 10     # (the 16-wide tile takes 16-wide grids only; one or two tile rows per image)
        c.append((f"conv_halo-cfg{cfg}-concat", case_conv_halo, dict(cfg=cfg, h=h, w=w, c0=64, c1=128, N=80, n_img=1)))
        for N in (48, 80, 192):
            c.append((f"conv_halo-cfg{cfg}-N{N}", case_conv_halo, dict(cfg=cfg, h=h, w=w, c0=64, N=N, n_img=2 if N == 80 else 1, residual=N != 192)))
        c.append((f"conv_halo-cfg{cfg}-h12", case_conv_halo, dict(cfg=cfg, h=12, w=w, c0=64, N=80, n_img=1, residual=True)))
        c.append((f"conv_halo-cfg{cfg}-ups", case_conv_halo, dict(cfg=cfg, h=h // 2, w=w // 2, c0=64, N=80, n_img=2, ups=1, residual=True)))
        c.append((f"conv_halo-cfg{cfg}-epilogue", case_conv_halo, dict(cfg=cfg, h=h, w=w, c0=64, N=160, n_img=2, residual=True, rowvec=True,
                                                                      act=nt.ACT_SILU, colstat=True)))
    return c


def lpr_cases():
    c = []
    for K, bm in ((320, 160), (512, 96), (640, 96)):
        for ny in (0, 2, 3):
            c.append((f"linear_pr-K{K}-ny{ny}", case_linear_pr, dict(M=bm + 75 if K == 320 else 96 * 2 + 40, K=K, N=640, ny=ny)))
        c.append((f"linear_pr-K{K}-geglu", case_linear_pr, dict(M=bm + 75, K=K, N=640, act=nt.ACT_GEGLU)))
        c.append((f"linear_pr-K{K}-ln_in", case_linear_pr, dict(M=bm + 40, K=K, N=320, ln_in=True)))
        if K != 512:
            c.append((f"linear_pr-K{K}-residual", case_linear_pr, dict(M=bm + 64, K=K, N=320, residual=True, ny=2)))
            c.append((f"linear_pr-K{K}-gn_coef", case_linear_pr, dict(M=2 * bm, K=K, N=320, gn_rpu=bm)))
    return c


def small_cases():
    c = []
    for M, R, Cc in ((130, 4, 64), (200, 64, 72), (300, 250, 380), (77, 1, 320)):
        for splits in (0, 1, 3):
            c.append((f"wgrad-{M}x{R}x{Cc}-s{splits}", case_wgrad, dict(M=M, R=R, C=Cc, splits=splits, aligned=splits != 3)))
    c.append(("wgrad-200x64x72-s0-misaligned", case_wgrad, dict(M=200, R=64, C=72, splits=0, aligned=False, alpha=-1.5)))
    c.append(("wgrad-group", case_wgrad_group, {}))
    for cin in (4, 8):
        for cout in (64, 320):
            c.append((f"conv_small_cin-{cin}-{cout}", case_conv_small_cin, dict(cin=cin, cout=cout)))
    for inplace in (False, True):
        for residual in (False, True):
            c.append((f"dropout-inplace{int(inplace)}-resid{int(residual)}", case_dropout, dict(inplace=inplace, residual=residual)))
    c.append(("dropout-2-byte-path", case_dropout, dict(inplace=False, residual=True, vec=False)))
    c.append(("dropout-p-below-2^-16", case_dropout, dict(inplace=False, residual=False, p=1e-5)))
    for kind in (0, 1):
        for taps in (9, 3):
            c.append((f"repack_conv-kind{kind}-taps{taps}", case_repack, dict(kind=kind, taps=taps)))
    return c


def experimental_cases():
    return [(f"experimental-{w}", case_experimental, dict(which=w)) for w in EXPERIMENTAL_ENTRIES]


def table(sweep_ids, gather_ids):
    return sweep_cases(sweep_ids) + gather_cases(gather_ids) + other_cases() + fused_cases() + halo_cases() + lpr_cases() + small_cases()


REFUSAL_IDS = [n for n, _ in gemm_refusal_cases(None, None)]   # (the thunks touch ops / dev only when called)


def report_table():
    """REPORT folded per (family, tensor): cases, worst rounding, largest bound, worst observed — the rows of MEASURED."""
    fam = {}
    for case, tensor, meas, bound, err in REPORT:
        key = (case.split("-cfg")[0].split("-")[0] + ("-" + case.split("-")[1] if case.startswith("gemm-") and not case.split("-")[1].startswith("cfg") else ""), tensor)
        n, m, b, e = fam.get(key, (0, 0.0, 0.0, 0.0))
        fam[key] = (n + 1, max(m, meas), max(b, bound), max(e, err))
    return [f"{k[0]:22s} {k[1]:24s} {n:5d}  {m:.1e}   {b:.1e}   {e:.1e}" for k, (n, m, b, e) in sorted(fam.items())]
