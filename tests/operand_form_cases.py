"""Per-entry kernel cases at the ENGINES' operand forms, with poisoned padding — one table, two backends.

Every ``case_xxx(ops, dev, ...)`` builds its operands the way the engines hand them to the C-ABI (column slices of wider buffers:
q | k halves, q | k | v thirds, virtual concats of two row-strided parts, V token-major or as the per-head transpose), calls the
``HipOps``-style wrapper on ``ops`` and checks the result against an fp64 torch reference WRITTEN OUT HERE from the definitions in
include/t2v_hip.h (never tests/emu_ops.py: the new cases must not share its mistakes).  ``tests/test_hostsim_operand_forms.py`` runs
the table on the host SIMT simulator (CPU), ``tests/test_gpu_operand_forms.py`` on the device.

Poison and guards (everything stays inside one allocation per tensor; no case makes an out-of-bounds access):
  * every operand is a view into a larger buffer: row stride > width, spare rows before and after;
  * input bytes the header says are NOT read hold NaN (stride gaps, spare rows, columns >= n, V rows past the sequence, the space
    between the images of a V^T buffer); bytes it says ARE read hold what it demands (V^T padding keys: 1e30, finite; the padding of
    kt / qt / dot: zero);
  * the region a kernel must write is pre-filled with NaN and must come back finite; everything else of an output allocation holds
    a sentinel and is compared BIT FOR BIT afterwards (stride gaps, neighbouring column slices, spare rows, workspace tails).

Metric: per ROW, e_r = ||got_r - ref_r|| / max(||ref_r||, 0.1 rms_row_norm(ref)); the maximum over the rows must stay below the bound.
Kernels that are exact data movement must match bit for bit.  Bound per tensor = max(the project's tolerance for the op family,
2 x the same metric of the fp64 reference rounded to the kernel's documented output / intermediate types) — computed from the reference
alone, at run time, once per case (``REPORT`` collects measured rounding, bound and observed error per tensor; ``report_lines()``
formats it).

Worst row per family and tensor (maximum over the family's cases).  rounding = the metric of the fp64 reference rounded to the
documented output / intermediate types (the reference alone), bound = what the cases assert, then the worst row observed on the host
simulator and on an MI355X:

    family                     tensor       cases  rounding  bound     simulator  MI355X
    attn_spatial_bwd mild      l2             9    2.4e-08   1.0e-04   5.1e-08    5.6e-08
    attn_spatial_bwd mild      dsum           9    2.1e-03   1.2e-02   2.1e-03    2.1e-03
    attn_spatial_bwd mild      dq             9    3.4e-03   1.2e-02   3.4e-03    3.4e-03
    attn_spatial_bwd mild      dk             9    4.0e-03   1.2e-02   4.0e-03    4.0e-03
    attn_spatial_bwd mild      dv             9    3.2e-03   1.2e-02   3.2e-03    3.2e-03
    attn_spatial_bwd peaked    l2             8    3.0e-08   1.0e-04   3.9e-08    7.1e-08
    attn_spatial_bwd peaked    dsum           8    2.1e-03   1.2e-02   2.1e-03    2.1e-03
    attn_spatial_bwd peaked    dq             8    8.0e-03   1.6e-02   8.0e-03    8.0e-03
    attn_spatial_bwd peaked    dk             8    7.9e-03   1.6e-02   7.9e-03    7.9e-03
    attn_spatial_bwd peaked    dv             8    4.5e-03   1.2e-02   4.5e-03    4.5e-03
    attn_spatial               out            2    2.9e-03   8.0e-03   2.7e-03    2.7e-03
    attn_temporal              out            8    3.4e-03   6.8e-03   2.9e-03    2.9e-03
    attn_temporal              probs          4    4.4e-08   1.0e-04   1.9e-07    1.7e-07
    attn_temporal_bwd          dq             8    4.0e-03   7.9e-03   2.2e-03    2.2e-03
    attn_temporal_bwd          dk             8    3.7e-03   7.3e-03   2.3e-03    2.3e-03
    attn_temporal_bwd          dv             8    3.4e-03   6.7e-03   2.1e-03    2.1e-03
    layernorm                  out            6    2.3e-03   4.6e-03   2.3e-03    2.3e-03
    layernorm_bwd              dx             6    1.8e-03   6.0e-03   1.8e-03    1.8e-03
    group_norm                 out           18    2.0e-03   4.0e-03   2.0e-03    2.0e-03
    gn_stats                   stats         18    2.9e-08   1.0e-04   6.2e-08    6.2e-08
    gn_apply                   out           18    2.0e-03   4.0e-03   2.0e-03    2.0e-03
    gn_bwd / gn_bwd2           dx            18    1.9e-03   6.0e-03   1.9e-03    1.9e-03
    softmax_rows               p              3    2.3e-03   4.6e-03   2.3e-03    2.3e-03
    softmax_bwd_rows           ds             3    2.9e-03   6.0e-03   2.9e-03    2.9e-03
    geglu_fwd                  out            2    2.6e-03   5.1e-03   2.6e-03    2.6e-03
    geglu_bwd                  dh             2    2.8e-03   6.0e-03   2.8e-03    2.8e-03
    add                        out            1    2.3e-03   4.6e-03   2.3e-03    2.3e-03
    sumpool2x2                 out            1    2.3e-03   4.6e-03   2.3e-03    2.3e-03
    norm_affine_grad           dbeta          3    3.0e-08   1.0e-04   8.9e-08    8.9e-08
    norm_affine_grad           dgamma         2    2.6e-08   1.0e-04   8.3e-08    8.5e-08
    transpose, transpose_pad, scatter2x, ncfhw_to_tokens, tokens_to_ncfhw, cast, gather, im2col: bit for bit on both backends

(a bf16 result whose only error is its final rounding sits AT the rounding figure: one rounding of an n-element row gives about
2^-9 / sqrt(3) * (a few worst-case rows) ~ 2e-3 .. 4e-3, which is why the bound is twice the measured figure where that exceeds the
project's whole-tensor tolerance.)  The raw t2v_attn_spatial_bwd call with seq_q = 130, seq_kv = 77 is right on both backends and stays
a positive case.
"""
import math

import torch
import torch.nn.functional as F

from t2v_turbo_amd import native as nt

NAN = float("nan")
SENT = -7.0          # sentinel of the must-not-write regions (finite, bf16-exact)
BF16_TOL, BWD_TOL, ATTN_TOL, ATTN_BWD_TOL, STAT_TOL = 4e-3, 6e-3, 8e-3, 1.2e-2, 1e-4
REPORT = []          # (case, tensor, reference-rounding worst row, bound, observed worst row)
_CUR = [""]

BF, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------------------ helpers
def rnd(*shape, seed, scale=1.0, shift=0.0):
    """Seeded normal values, rounded to bf16 (what the kernel receives), as fp64."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift).to(BF).double()


def bfr(t):
    return t.to(BF).double()


def f32r(t):
    return t.to(F32).double()


def _raw(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def inbuf(data, ld, dev, dtype=BF, col0=0, pre=2, post=2, fill=NAN):
    """``data`` [M, C] as a view (rows [pre, pre + M), columns [col0, col0 + C)) of a [pre + M + post, ld] buffer of ``fill``."""
    M, C = data.shape
    assert ld >= col0 + C
    full = torch.full((pre + M + post, ld), fill, dtype=dtype)
    full[pre:pre + M, col0:col0 + C] = data.to(dtype)
    return full.to(dev)[pre:pre + M, col0:col0 + C]


def inflat(data, dev, dtype=F32, pad=16):
    """Contiguous ``data`` inside a flat buffer with ``pad`` NaN elements before and after (pad * itemsize a multiple of 16)."""
    full = torch.full((data.numel() + 2 * pad,), NAN, dtype=dtype) if dtype.is_floating_point else torch.full((data.numel() + 2 * pad,), -1, dtype=dtype)
    full[pad:pad + data.numel()] = data.reshape(-1).to(dtype)
    return full.to(dev)[pad:pad + data.numel()].view(data.shape)


class Out:
    """An output allocation [pre + M + post, ld]: the column ranges ``cols`` of rows [pre, pre + M) are must-write regions (NaN, or
    ``init`` for in-place / accumulating kernels), every other element a sentinel that has to survive bit for bit."""

    def __init__(self, M, ld, cols, dev, dtype=BF, pre=2, post=2, init=None):
        full = torch.full((pre + M + post, ld), SENT, dtype=dtype)
        self.mask = torch.zeros(pre + M + post, ld, dtype=torch.bool)
        self.rows, self.cols = slice(pre, pre + M), cols
        for i, (c0, c1) in enumerate(cols):
            full[self.rows, c0:c1] = NAN if init is None or init[i] is None else init[i].to(dtype)
            self.mask[self.rows, c0:c1] = True
        self.snap = full.clone()
        self.full = full.to(dev)
        self.views = [self.full[self.rows, c0:c1] for c0, c1 in cols]

    def guard(self, what):
        got = self.full.cpu()
        bad = (_raw(got) != _raw(self.snap)) & ~self.mask
        assert not bool(bad.any()), f"{what}: wrote outside its region, first at (row, col) {bad.nonzero()[0].tolist()} of the allocation"
        return got

    def check(self, what):
        got = self.guard(what)
        outs = [got[self.rows, c0:c1] for c0, c1 in self.cols]
        for i, o in enumerate(outs):
            fin = torch.isfinite(o.double())
            assert bool(fin.all()), f"{what}[{i}]: non-finite / unwritten at (row, col) {(~fin).nonzero()[0].tolist()}"
        return outs

    def untouched(self):
        return torch.equal(_raw(self.full.cpu()), _raw(self.snap))


def row_err(got, ref):
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    rn = ref.norm(dim=1)
    floor = 0.1 * float(rn.pow(2).mean().sqrt())
    return float(((got - ref).norm(dim=1) / rn.clamp_min(max(floor, 1e-300))).max())


def close(name, got, ref, ref_rounded, tol):
    meas = row_err(ref_rounded, ref)
    bound = max(tol, 2.0 * meas)
    err = row_err(got, ref)
    REPORT.append((_CUR[0], name, meas, bound, err))
    assert err < bound, f"{name}: worst row {err:.3e} >= bound {bound:.3e} (tolerance {tol:.1e}, reference rounding {meas:.3e})"


def exact(name, got, ref):
    """Bit-for-bit: ``ref`` already has the output dtype."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, name
    bad = _raw(got.contiguous()) != _raw(ref.contiguous())
    REPORT.append((_CUR[0], name, 0.0, 0.0, float(bad.any())))
    assert not bool(bad.any()), f"{name}: differs, first at {bad.nonzero()[0].tolist()}"


def refuses(ops, fn, *outs):
    """``fn()`` must raise NativeError (an error code from the entry point, before any launch) and leave every output untouched."""
    try:
        fn()
    except nt.NativeError:
        pass
    else:
        raise AssertionError("the entry point accepted a bad argument")
    for o in outs:
        assert o.untouched(), "a refused call wrote to its output"


def _dev(t, dev, dtype=F32):
    return t.to(dtype).to(dev)


# ------------------------------------------------------------------------------------------------------------------ spatial attention
def _tposed(t, n_img, seq, ld, dev, tail=NAN):
    """t [n_img * seq, cols] -> per image [cols][ld]: columns [0, seq) = t^T, [seq, roundup(seq, 64)) = 0 (read: must be zero),
    [roundup, ld) = ``tail`` (not read)."""
    cols, sp = t.shape[1], (seq + 63) // 64 * 64
    out = torch.full((n_img * cols, ld), tail, dtype=torch.float64)
    out[:, :sp] = 0.0
    for i in range(n_img):
        out[i * cols:(i + 1) * cols, :seq] = t[i * seq:(i + 1) * seq].t()
    return inbuf(out, ld, dev)


def _attn_inputs(n_img, heads, seq_q, seq_kv, dist):
    inner = heads * 64
    sc = 0.8 if dist == "mild" else 2.0
    q, k = rnd(n_img * seq_q, inner, seed=1, scale=sc), rnd(n_img * seq_kv, inner, seed=2, scale=sc)
    v, do = rnd(n_img * seq_kv, inner, seed=3), rnd(n_img * seq_q, inner, seed=4)
    if dist == "peaked":
        # channel 0 of every head: keys 0, the LAST key (in the final, partial tile) 16, and every query the value that makes that key's
        # dot product the largest of its row by 2 .. 4 (0.25 .. 0.5 in the exponent): the running maximum moves in the final tile.  The
        # last query of every image gets + 160 (20 in the exponent): its softmax is one-hot to bf16 precision, its dS ~ 0.
        for img in range(n_img):
            rq, rk = slice(img * seq_q, (img + 1) * seq_q), slice(img * seq_kv, (img + 1) * seq_kv)
            for hd in range(heads):
                c0 = hd * 64
                k[rk, c0] = 0.0
                k[(img + 1) * seq_kv - 1, c0:c0 + 64] = 0.0
                k[(img + 1) * seq_kv - 1, c0] = 16.0
                other = (q[rq, c0 + 1:c0 + 64] @ k[rk, c0 + 1:c0 + 64].t())[:, :seq_kv - 1] if seq_kv > 1 else torch.zeros(seq_q, 1, dtype=torch.float64)
                want = other.max(dim=1).values.clamp_min(0.0) + 3.0
                want[-1] += 160.0
                q[rq, c0] = bfr(want / 16.0)     # bf16 spacing of want / 16 <= 1/16 for want < 256: the margin stays within 3 +- 1
                assert bool(((q[rq, c0] * 16.0) > other.max(dim=1).values + 1.0).all())
    return q, k, v, do


def _attn_ref(q, k, v, do, n_img, heads, seq_q, seq_kv, scale):
    """fp64 definition and the same with the documented bf16 intermediates (P, dS, D from the bf16 O)."""
    inner = heads * 64
    o = torch.zeros(n_img * seq_q, inner, dtype=torch.float64)
    g = [torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)]
    gr = [torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)]
    l2, ds = torch.zeros(n_img * heads, seq_q, dtype=torch.float64), torch.zeros(n_img * heads, seq_q, dtype=torch.float64)
    ds_r, probs = torch.zeros_like(ds), {}
    for img in range(n_img):
        rq, rk = slice(img * seq_q, (img + 1) * seq_q), slice(img * seq_kv, (img + 1) * seq_kv)
        for hd in range(heads):
            c = slice(hd * 64, (hd + 1) * 64)
            Q, K, V, dO = q[rq, c], k[rk, c], v[rk, c], do[rq, c]
            S = Q @ K.t() * scale
            P = S.softmax(dim=1)
            o[rq, c] = P @ V
            dP = dO @ V.t()
            D = (P * dP).sum(dim=1, keepdim=True)
            dS = P * (dP - D)
            g[0][rq, c], g[1][rk, c], g[2][rk, c] = dS @ K * scale, dS.t() @ Q * scale, P.t() @ dO
            l2[img * heads + hd] = torch.logsumexp(S, dim=1) / math.log(2.0)
            ds[img * heads + hd] = D[:, 0]
            Dr = (dO * bfr(o[rq, c])).sum(dim=1, keepdim=True)
            dSr = bfr(P * (dP - Dr))
            gr[0][rq, c], gr[1][rk, c], gr[2][rk, c] = bfr(dSr @ K * scale), bfr(dSr.t() @ Q * scale), bfr(bfr(P).t() @ dO)
            ds_r[img * heads + hd] = Dr[:, 0]
            probs[(img, hd)] = P
    return bfr(o), g, gr, l2, ds, ds_r


def case_attn_spatial_bwd(ops, dev, seq, v_layout, dist, seq_kv=None, refuse=False):
    """t2v_attn_spatial_bwd: q | k halves of one [M, 2 inner] buffer, dq | dk halves of another, dv at ld = inner + 8, V token-major or
    per head, ld_kt = sp, ld_qt = sp + 64, ld_stat = sp + 8.  ``seq_kv``: the raw entry with seq_q != seq_kv (the wrapper passes seq
    twice); ``refuse``: that call must be refused."""
    n_img, heads, scale = 2, 2, 0.125
    inner, seq_q, raw = heads * 64, seq, seq_kv is not None
    seq_kv = seq if seq_kv is None else seq_kv
    Mq, Mk = n_img * seq_q, n_img * seq_kv
    q, k, v, do = _attn_inputs(n_img, heads, seq_q, seq_kv, dist)
    o, g, gr, l2_ref, ds_ref, ds_r = _attn_ref(q, k, v, do, n_img, heads, seq_q, seq_kv, scale)
    spq, spk = (seq_q + 63) // 64 * 64, (seq_kv + 63) // 64 * 64
    qk = torch.full((max(Mq, Mk), 2 * inner), NAN, dtype=torch.float64)
    qk[:Mq, :inner], qk[:Mk, inner:] = q, k
    qk_d = inbuf(qk, 2 * inner, dev)
    q_d, k_d = qk_d[:Mq, :inner], qk_d[:Mk, inner:]
    if v_layout == "tok":
        v_d = inbuf(v, inner + 8, dev)
        vis, vhs = seq_kv * (inner + 8), 64
    else:   # per (image, head): [padded keys][64]; the padding rows are not read (keys past seq_kv come from the library's zero page)
        vb = torch.full((n_img * heads * spk, 64), NAN, dtype=torch.float64)
        for img in range(n_img):
            for hd in range(heads):
                vb[(img * heads + hd) * spk:(img * heads + hd) * spk + seq_kv] = v[img * seq_kv:(img + 1) * seq_kv, hd * 64:(hd + 1) * 64]
        v_d = inbuf(vb, 64, dev)
        vis, vhs = heads * spk * 64, spk * 64
    kt_d = _tposed(k, n_img, seq_kv, spk, dev)
    qt_d, dot_d = _tposed(q, n_img, seq_q, spq + 64, dev), _tposed(do, n_img, seq_q, spq + 64, dev)
    do_d, o_d = inbuf(do, inner + 8, dev), inbuf(o, inner + 8, dev)
    ld_stat = spq + 8
    l2_o, ds_o = Out(n_img * heads, ld_stat, [(0, seq_q)], dev, F32), Out(n_img * heads, ld_stat, [(0, seq_q)], dev, F32)
    gqk = Out(max(Mq, Mk), 2 * inner, [(0, inner), (inner, 2 * inner)], dev)
    if Mq != Mk:   # the shorter half's extra rows must survive too
        gqk = _qk_out(Mq, Mk, inner, dev)
    gv = Out(Mk, inner + 8, [(0, inner)], dev)
    dq_d, dk_d, dv_d = gqk.views[0][:Mq], gqk.views[1][:Mk], gv.views[0]

    def call():
        if not raw:
            ops.attn_spatial_bwd(q_d, k_d, v_d, vis, vhs, kt_d, qt_d, dot_d, do_d, o_d, l2_o.views[0], ds_o.views[0], dq_d, dk_d, dv_d,
                                 n_img, seq, heads, scale)
        else:
            p = lambda t: t.data_ptr()  # noqa: E731
            ops._call("t2v_attn_spatial_bwd", p(q_d), 2 * inner, p(k_d), 2 * inner, p(v_d), v_d.stride(0), vis, vhs, p(kt_d), spk, p(qt_d),
                      p(dot_d), spq + 64, p(do_d), inner + 8, p(o_d), inner + 8, p(l2_o.views[0]), p(ds_o.views[0]), ld_stat, p(dq_d),
                      2 * inner, p(dk_d), 2 * inner, p(dv_d), inner + 8, n_img, seq_q, seq_kv, heads, scale)

    if refuse:
        return refuses(ops, call, gqk, gv, l2_o, ds_o)
    call()
    got_qk, (got_v,) = gqk.check("dq|dk"), gv.check("dv")
    (l2_g,), (ds_g,) = l2_o.check("l2"), ds_o.check("dsum")
    close("l2", l2_g, l2_ref, f32r(l2_ref), STAT_TOL)
    close("dsum", ds_g, ds_ref, f32r(ds_r), ATTN_BWD_TOL)
    for name, a, b, c in zip(("dq", "dk", "dv"), (got_qk[0][:Mq], got_qk[1][:Mk], got_v), g, gr):
        close(name, a, b, c, ATTN_BWD_TOL)


def _qk_out(Mq, Mk, inner, dev):
    """dq | dk halves with different row counts: the must-write region of each half ends at its own row count."""
    o = Out(max(Mq, Mk), 2 * inner, [(0, inner), (inner, 2 * inner)], dev)
    full = o.full.cpu()
    for M, c0 in ((Mq, 0), (Mk, inner)):
        full[2 + M:2 + max(Mq, Mk), c0:c0 + inner] = SENT
        o.mask[2 + M:2 + max(Mq, Mk), c0:c0 + inner] = False
    o.snap = full.clone()
    o.full = full.to(dev)
    o.views = [o.full[o.rows, c0:c1] for c0, c1 in o.cols]
    return o


def case_attn_spatial(ops, dev, n_img, seq_q, seq_kv, heads, kv_div):
    """t2v_attn_spatial: q | k halves of [M, 2 inner], out at ldo = inner + 4, V^T with ld_vt = sp + 8, padding keys 1e30 (read,
    finite), and a vt_img_stride larger than heads * 64 * ld_vt with NaN between the images."""
    inner, scale, n_kv = heads * 64, 0.125, n_img // kv_div
    Mq, Mk = n_img * seq_q, n_kv * seq_kv
    q, k, v = rnd(Mq, inner, seed=1, scale=0.8), rnd(Mk, inner, seed=2, scale=0.8), rnd(Mk, inner, seed=3)
    qk = torch.full((max(Mq, Mk), 2 * inner), NAN, dtype=torch.float64)
    qk[:Mq, :inner], qk[:Mk, inner:] = q, k
    qk_d = inbuf(qk, 2 * inner, dev)
    sp = (seq_kv + 63) // 64 * 64
    ld_vt, stride = sp + 8, heads * 64 * (sp + 8) + 64
    vt = torch.full((n_kv * stride + 16,), NAN, dtype=BF)
    ref, ref_r = torch.zeros(Mq, inner, dtype=torch.float64), torch.zeros(Mq, inner, dtype=torch.float64)
    for ikv in range(n_kv):
        blk = vt[ikv * stride:ikv * stride + heads * 64 * ld_vt].view(heads * 64, ld_vt)
        blk[:, :seq_kv] = v[ikv * seq_kv:(ikv + 1) * seq_kv].t().to(BF)
        blk[:, seq_kv:sp] = 1e30
    for img in range(n_img):
        ikv = img // kv_div
        for hd in range(heads):
            c, rq, rk = slice(hd * 64, hd * 64 + 64), slice(img * seq_q, (img + 1) * seq_q), slice(ikv * seq_kv, (ikv + 1) * seq_kv)
            P = (q[rq, c] @ k[rk, c].t() * scale).softmax(dim=1)
            ref[rq, c], ref_r[rq, c] = P @ v[rk, c], bfr(bfr(P) @ v[rk, c])
    out = Out(Mq, inner + 4, [(0, inner)], dev)
    ops.attn_spatial(qk_d[:Mq, :inner], qk_d[:Mk, inner:], vt.to(dev), ld_vt, out.views[0], n_img, seq_q, seq_kv, heads, kv_div, scale,
                     vt_img_stride=stride)
    close("out", out.check("out")[0], ref, ref_r, ATTN_TOL)


# ------------------------------------------------------------------------------------------------------------------ temporal attention
def _seqs(t, clips, frames, hw, heads):
    return t.reshape(clips, frames, hw, heads, 64).permute(0, 2, 3, 1, 4).reshape(-1, frames, 64)


def _rows(t, clips, frames, hw, heads):
    return t.reshape(clips, hw, heads, frames, 64).permute(0, 3, 1, 2, 4).reshape(-1, heads * 64)


def case_attn_temporal(ops, dev, frames, hw, with_probs):
    clips, heads, scale = 2, 2, 0.125
    inner, M = heads * 64, clips * frames * hw
    qkv = rnd(M, 3 * inner, seed=1, scale=0.7)
    Q, K, V = (_seqs(qkv[:, i * inner:(i + 1) * inner], clips, frames, hw, heads) for i in range(3))
    P = (Q @ K.transpose(1, 2) * scale).softmax(dim=2)
    ref = _rows(P @ V, clips, frames, hw, heads)
    ref_r = bfr(_rows(bfr(P) @ V, clips, frames, hw, heads))
    qkv_d = inbuf(qkv, 3 * inner, dev)
    out = Out(M, inner + 8, [(0, inner)], dev)
    n_p = clips * hw * heads * frames * frames
    pr = Out(1, n_p + 8, [(0, n_p)], dev, F32, pre=1, post=1) if with_probs else None
    ops.attn_temporal(qkv_d[:, :inner], qkv_d[:, inner:2 * inner], qkv_d[:, 2 * inner:], out.views[0], clips, frames, hw, heads, scale,
                      probs=None if pr is None else pr.views[0])
    close("out", out.check("out")[0], ref, ref_r, BF16_TOL)
    if pr is not None:
        close("probs", pr.check("probs")[0].reshape(-1, frames), P.reshape(-1, frames), f32r(P).reshape(-1, frames), STAT_TOL)


def case_attn_temporal_bwd(ops, dev, frames, hw, with_dprobs, refuse=False):
    clips, heads, scale = 2, 2, 0.125
    inner, M = heads * 64, clips * frames * hw
    qkv, do = rnd(M, 3 * inner, seed=1, scale=0.7), rnd(M, inner, seed=2)
    dpr = torch.randn(clips * hw * heads, frames, frames, generator=torch.Generator().manual_seed(3)).double() if with_dprobs else None
    Q, K, V = (_seqs(qkv[:, i * inner:(i + 1) * inner], clips, frames, hw, heads) for i in range(3))
    dO = _seqs(do, clips, frames, hw, heads)
    P = (Q @ K.transpose(1, 2) * scale).softmax(dim=2)
    dP = dO @ V.transpose(1, 2) + (0 if dpr is None else dpr)
    dS = P * (dP - (P * dP).sum(dim=2, keepdim=True))
    dSr, Pr = bfr(dS), bfr(P)
    rw = lambda t: _rows(t, clips, frames, hw, heads)  # noqa: E731
    ref = [rw(dS @ K * scale), rw(dS.transpose(1, 2) @ Q * scale), rw(P.transpose(1, 2) @ dO)]
    ref_r = [bfr(rw(dSr @ K * scale)), bfr(rw(dSr.transpose(1, 2) @ Q * scale)), bfr(rw(Pr.transpose(1, 2) @ dO))]
    qkv_d, do_d = inbuf(qkv, 3 * inner, dev), inbuf(do, inner + 8, dev)
    dpr_d = None if dpr is None else inflat(dpr, dev)
    g = Out(M, 3 * inner + 8, [(0, inner), (inner, 2 * inner), (2 * inner, 3 * inner)], dev)

    def call():
        ops.attn_temporal_bwd(qkv_d[:, :inner], qkv_d[:, inner:2 * inner], qkv_d[:, 2 * inner:], do_d, dpr_d, *g.views, clips, frames, hw,
                              heads, scale)

    if refuse:
        return refuses(ops, call, g)
    call()
    for name, a, b, c in zip(("dq", "dk", "dv"), g.check("dq|dk|dv"), ref, ref_r):
        close(name, a, b, c, BWD_TOL)


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_inputs(M, C, shifted):
    x = rnd(M, C, seed=1, scale=0.5, shift=30.0) if shifted else rnd(M, C, seed=1)
    return x, f32r(rnd(C, seed=2, scale=0.2, shift=1.0)), f32r(rnd(C, seed=3, scale=0.1))


def case_layernorm(ops, dev, M, C, shifted=False):
    x, gamma, beta = _ln_inputs(M, C, shifted)
    ref = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    out = Out(M, C + 8, [(0, C)], dev)
    ops.layernorm(inbuf(x, C + 8, dev), _dev(gamma, dev), _dev(beta, dev), 1e-5, out.views[0])
    close("out", out.check("out")[0], ref, bfr(ref), BF16_TOL)


def case_layernorm_bwd(ops, dev, M, C, shifted=False, resid=True):
    x, gamma, _ = _ln_inputs(M, C, shifted)
    dy, r = rnd(M, C, seed=4), rnd(M, C, seed=5)
    mean = x.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + 1e-5)
    xh, g = (x - mean) * rstd, dy * gamma
    ref = rstd * (g - g.mean(dim=1, keepdim=True) - xh * (g * xh).mean(dim=1, keepdim=True)) + (r if resid else 0)
    dx = Out(M, C + 8, [(0, C)], dev)
    ops.layernorm_bwd(inbuf(x, C + 8, dev), _dev(gamma, dev), 1e-5, inbuf(dy, C + 8, dev), inbuf(r, C + 8, dev) if resid else None, dx.views[0])
    close("dx", dx.check("dx")[0], ref, bfr(ref), BWD_TOL)


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def _gn_inputs(c0, c1, units, rows):
    C, M = c0 + c1, units * rows
    x = rnd(M, C, seed=1)
    for u in range(units):   # every unit its own mean and spread: the row after a unit boundary must be normalised with ITS unit's statistics
        x[u * rows:(u + 1) * rows] = bfr(x[u * rows:(u + 1) * rows] * (1.0 + 0.5 * u) + 3.0 * u)
    return x, f32r(rnd(C, seed=5, scale=0.2, shift=1.0)), f32r(rnd(C, seed=6, scale=0.1))


def _gn_stats_ref(x, units, rows, G, eps):
    C = x.shape[1]
    xg = x.reshape(units, rows, G, C // G).permute(0, 2, 1, 3).reshape(units, G, -1)
    return xg.mean(dim=2), 1.0 / torch.sqrt(xg.var(dim=2, unbiased=False) + eps)


def _parts(x, c0, c1, dev):
    return inbuf(x[:, :c0], c0 + 8, dev), (inbuf(x[:, c0:], c1 + 16, dev, col0=8) if c1 else None)


def _ws(n, dev):
    return Out(1, n + 16, [(0, n)], dev, F32, pre=1, post=1, init=[torch.zeros(1, n)])


def case_group_norm(ops, dev, c0, c1, rows, silu):
    """t2v_group_norm, t2v_gn_stats and t2v_gn_apply over a virtual concat of two row-strided parts; units = 2 with different means."""
    units, G, eps = 2, 32, 1e-5
    C, M = c0 + c1, units * rows
    x, gamma, beta = _gn_inputs(c0, c1, units, rows)
    mean, rstd = _gn_stats_ref(x, units, rows, G, eps)
    rep = lambda t: t.repeat_interleave(C // G, dim=1)[:, None, :]  # noqa: E731
    y = ((x.reshape(units, rows, C) - rep(mean)) * rep(rstd) * gamma + beta).reshape(M, C)
    ref = F.silu(y) if silu else y
    x0, x1 = _parts(x, c0, c1, dev)
    g_d, b_d = _dev(gamma, dev), _dev(beta, dev)
    ws = _ws(ops.group_norm_ws_floats(units, rows, G, C), dev)
    out = Out(M, C + 8, [(0, C)], dev)
    ops.group_norm(x0, x1, units, rows, eps, g_d, b_d, silu, ws.views[0], out.views[0], G)
    ws.guard("group_norm ws")
    close("group_norm", out.check("group_norm out")[0], ref, bfr(ref), BF16_TOL)
    ws = _ws(ops.gn_ws_floats(units, rows, G), dev)
    st_c = Out(1, units * 2 * G + 8, [(0, units * 2 * G)], dev, F32, pre=1, post=1)   # (the ABI's stats are contiguous [units][groups][2])
    ops.gn_stats(x0, x1, units, rows, eps, ws.views[0], st_c.views[0], G)
    ws.guard("gn_stats ws")
    st_ref = torch.stack([mean, rstd], dim=2).reshape(units, 2 * G)
    st_got = st_c.check("stats")[0].reshape(units, 2 * G)
    close("gn_stats", st_got, st_ref, f32r(st_ref), STAT_TOL)
    out2 = Out(M, C + 8, [(0, C)], dev)
    ops.gn_apply(x0, x1, units, rows, _dev(st_ref, dev).contiguous(), g_d, b_d, silu, out2.views[0], G)
    close("gn_apply", out2.check("gn_apply out")[0], ref, bfr(ref), BF16_TOL)


def case_gn_bwd(ops, dev, c0, c1, rows, silu):
    """t2v_gn_bwd (one part, C <= 2048) / t2v_gn_bwd2 (virtual concat) with strided dy, resid and dx."""
    units, G, eps = 2, 32, 1e-5
    C, M, cpg = c0 + c1, units * rows, (c0 + c1) // 32
    x, gamma, beta = _gn_inputs(c0, c1, units, rows)
    dy, r = rnd(M, C, seed=3), rnd(M, C, seed=4)
    mean, rstd = _gn_stats_ref(x, units, rows, G, eps)
    mean, rstd = f32r(mean), f32r(rstd)   # (the kernel receives the fp32 statistics of the forward)
    rep = lambda t: t.repeat_interleave(cpg, dim=1)[:, None, :]  # noqa: E731
    xh = (x.reshape(units, rows, C) - rep(mean)) * rep(rstd)
    g = dy.reshape(units, rows, C)
    if silu:
        u = xh * gamma + beta
        sig = torch.sigmoid(u)
        g = g * sig * (1 + u * (1 - sig))
    g = g * gamma
    gg, xg = g.reshape(units, rows, G, cpg), xh.reshape(units, rows, G, cpg)
    m1, m2 = gg.mean(dim=(1, 3), keepdim=True), (gg * xg).mean(dim=(1, 3), keepdim=True)
    ref = (rep(rstd).reshape(units, 1, G, cpg) * (gg - m1 - xg * m2)).reshape(M, C) + r
    x0, x1 = _parts(x, c0, c1, dev)
    ws = _ws(ops.gn_bwd_ws_floats(units, rows, G), dev)
    dx = Out(M, C + 8, [(0, C)], dev)
    st = _dev(torch.stack([mean, rstd], dim=2).reshape(units, 2 * G), dev).contiguous()
    ops.gn_bwd(x0, units, rows, st, _dev(gamma, dev), _dev(beta, dev), silu, inbuf(dy, C + 8, dev), inbuf(r, C + 16, dev, col0=8), ws.views[0],
               dx.views[0], G, x1=x1)
    ws.guard("gn_bwd ws")
    close("dx", dx.check("dx")[0], ref, bfr(ref), BWD_TOL)


# ------------------------------------------------------------------------------------------------------------------ softmax
def _logits(rows, n):
    s = rnd(rows, n, seed=1, scale=4.0)
    s[0, min(1, n - 1)] = bfr(s[0, min(1, n - 1)] + 80.0)
    return s


def case_softmax_rows(ops, dev, rows, n, n_pad, ld):
    """In place: columns [0, n) normalised, [n, n_pad) set to exactly 0 (their input is NaN: read, never used), [n_pad, ld) guarded."""
    s = _logits(rows, n)
    init = torch.full((rows, n_pad), NAN, dtype=torch.float64)
    init[:, :n] = s
    buf = Out(rows, ld, [(0, n_pad)], dev, init=[init])
    ops.softmax_rows(buf.views[0], rows, n, n_pad, ld)
    got = buf.check("softmax")[0]
    assert n == n_pad or float(got[:, n:].double().abs().max()) == 0.0
    ref = s.softmax(dim=1)
    close("p", got[:, :n], ref, bfr(ref), BF16_TOL)


def case_softmax_bwd_rows(ops, dev, rows, n, n_pad, ld):
    p = bfr(_logits(rows, n).softmax(dim=1))
    dp = rnd(rows, n, seed=2)
    ref = p * (dp - (p * dp).sum(dim=1, keepdim=True))
    init = torch.full((rows, n_pad), NAN, dtype=torch.float64)
    init[:, :n] = dp
    buf = Out(rows, ld, [(0, n_pad)], dev, init=[init])
    ops.softmax_bwd_rows(inbuf(p, ld, dev), buf.views[0], rows, n, n_pad, ld)
    got = buf.check("softmax_bwd")[0]
    assert n == n_pad or float(got[:, n:].double().abs().max()) == 0.0
    close("ds", got[:, :n], ref, bfr(ref), BWD_TOL)


# ------------------------------------------------------------------------------------------------------------------ GEGLU
def _geglu_inputs(M, inner):
    h = rnd(M, 2 * inner, seed=1).reshape(M, inner // 32, 2, 32)
    special = torch.tensor([4.5, -4.5, 6.0, -6.0, 20.0, -20.0, 0.0], dtype=torch.float64)
    h[0, 0, 1, :7] = special                     # gates: the polynomial's clamp (forward), the exact pdf (backward)
    h[M - 1, inner // 32 - 1, 1, 32 - 7:] = special
    return h.reshape(M, 2 * inner)


def case_geglu_fwd(ops, dev, M, inner):
    h = _geglu_inputs(M, inner)
    g = h.reshape(M, -1, 2, 32)
    ref = (g[:, :, 0] * F.gelu(g[:, :, 1])).reshape(M, inner)
    out = Out(M, inner + 8, [(0, inner)], dev)
    ops.geglu_fwd(inbuf(h, 2 * inner + 8, dev), out.views[0])
    close("out", out.check("out")[0], ref, bfr(ref), BF16_TOL)


def case_geglu_bwd(ops, dev, M, inner):
    h, dy = _geglu_inputs(M, inner), rnd(M, inner, seed=2)
    g = h.reshape(M, -1, 2, 32)
    v, gate, d = g[:, :, 0], g[:, :, 1], dy.reshape(M, -1, 32)
    cdf = 0.5 * (1.0 + torch.erf(gate * math.sqrt(0.5)))
    pdf = torch.exp(-0.5 * gate * gate) / math.sqrt(2.0 * math.pi)
    ref = torch.stack([d * gate * cdf, d * v * (cdf + gate * pdf)], dim=2).reshape(M, 2 * inner)
    dh = Out(M, 2 * inner + 8, [(0, 2 * inner)], dev)
    ops.geglu_bwd(inbuf(h, 2 * inner + 8, dev), inbuf(dy, inner + 8, dev), dh.views[0])
    close("dh", dh.check("dh")[0], ref, bfr(ref), BWD_TOL)


# ------------------------------------------------------------------------------------------------------------------ data movement
def case_add(ops, dev, M=37, C=72):
    a, b = rnd(M, C, seed=1), rnd(M, C, seed=2)
    out = Out(M, C + 8, [(0, C)], dev)
    ops.add(inbuf(a, C + 8, dev), inbuf(b, C + 16, dev, col0=8), out.views[0])
    close("out", out.check("out")[0], a + b, bfr(a + b), BF16_TOL)


def _batched(data, ld, gap, dev):
    """data [batch, R, C] -> flat buffer, batch b at b * (R * ld + gap), rows at stride ld; NaN elsewhere.  -> (view of batch 0, stride)."""
    batch, R, C = data.shape
    stride = R * ld + gap
    full = torch.full((16 + batch * stride,), NAN, dtype=BF)
    for b in range(batch):
        full[8 + b * stride:8 + b * stride + R * ld].view(R, ld)[:, :C] = data[b].to(BF)
    return torch.as_strided(full.to(dev), (R, C), (ld, 1), 8), stride


class _BatchedOut(Out):
    def __init__(self, batch, R, C, ld, gap, dev):
        stride = R * ld + gap
        full = torch.full((1, 16 + batch * stride), SENT, dtype=BF)
        self.mask = torch.zeros_like(full, dtype=torch.bool)
        for b in range(batch):
            self.mask[0, 8 + b * stride:8 + b * stride + R * ld].view(R, ld)[:, :C] = True
        full[self.mask] = NAN
        self.snap, self.full, self.stride = full.clone(), full.to(dev), stride
        self.view0 = torch.as_strided(self.full, (R, C), (ld, 1), 8)
        self.geom = (batch, R, C, ld, stride)

    def result(self, what):
        got = self.guard(what)
        batch, R, C, ld, stride = self.geom
        out = torch.stack([got[0, 8 + b * stride:8 + b * stride + R * ld].view(R, ld)[:, :C] for b in range(batch)])
        assert bool(torch.isfinite(out.double()).all()), f"{what}: unwritten"
        return out


def case_transpose(ops, dev, rows, cols, batch, pad):
    """t2v_transpose_bf16 / t2v_transpose_pad_bf16 with row strides > widths and batch strides with gaps; exact, zero padding exact."""
    src = rnd(batch, rows, cols, seed=1)
    ld_in = cols + 8
    rp = (rows + 63) // 64 * 64 if pad else rows
    ld_out = rp + 8
    s_d, in_stride = _batched(src, ld_in, 24, dev)
    out = _BatchedOut(batch, cols, rp, ld_out, 40, dev)
    (ops.transpose_pad if pad else ops.transpose)(s_d, rows, cols, out.view0, batch=batch, in_stride=in_stride, out_stride=out.stride)
    ref = torch.zeros(batch, cols, rp, dtype=torch.float64)
    ref[:, :, :rows] = src.transpose(1, 2)
    exact("out", out.result("transpose"), ref.to(BF))


def case_sumpool_scatter(ops, dev):
    n, h, w, C = 2, 3, 5, 16
    src = rnd(n * 2 * h * 2 * w, C, seed=1)
    out = Out(n * h * w, C, [(0, C)], dev)
    ops.sumpool2x2(inbuf(src, C, dev), n, h, w, out.views[0])
    ref = src.reshape(n, h, 2, w, 2, C).sum(dim=(2, 4)).reshape(-1, C)
    close("sumpool", out.check("sumpool")[0], ref, bfr(ref), BF16_TOL)
    for H, W in ((2 * h, 2 * w), (2 * h - 1, 2 * w - 1)):
        s = rnd(n * h * w, C, seed=2)
        o = Out(n * H * W, C, [(0, C)], dev)
        ops.scatter2x(inbuf(s, C, dev), n, h, w, H, W, o.views[0])
        z = torch.zeros(n, H, W, C, dtype=torch.float64)
        z[:, 0:2 * h:2, 0:2 * w:2] = s.reshape(n, h, w, C)[:, :(H + 1) // 2, :(W + 1) // 2]
        exact(f"scatter2x {H}x{W}", o.check("scatter2x")[0], z.reshape(-1, C).to(BF))


def case_layout_cast(ops, dev):
    b, c, f, h, w = 2, 4, 3, 2, 5
    M = b * f * h * w
    x = rnd(b, c, f, h, w, seed=1)
    for dt in (F32, BF, torch.float16):
        xs = x.to(dt)   # (bf16-exact values: every dtype holds them exactly)
        out = Out(M, c + 4, [(0, c)], dev)
        ops.ncfhw_to_tokens(inflat(xs, dev, dt), out.views[0])
        ref = x.permute(0, 2, 3, 4, 1).reshape(M, c).to(BF)
        exact(f"ncfhw_to_tokens {dt}", out.check("tokens")[0], ref)
        for tok_dt in (BF, F32):
            o5 = Out(1, b * c * f * h * w + 8, [(0, b * c * f * h * w)], dev, dt, pre=1, post=1)
            ops.tokens_to_ncfhw(inbuf(ref.double(), c + 4, dev, tok_dt), o5.views[0].view(b, c, f, h, w))
            exact(f"tokens_to_ncfhw {tok_dt}->{dt}", o5.check("ncfhw")[0].reshape(b, c, f, h, w), xs)
    n = 1003
    v = torch.randn(n, generator=torch.Generator().manual_seed(2))
    for src, dst in ((F32, BF), (BF, F32), (F32, torch.float16)):
        o = Out(1, n + 13, [(0, n)], dev, dst, pre=1, post=1)
        s = v.to(src)
        ops.cast(inflat(s, dev, src), o.views[0].reshape(-1))
        exact(f"cast {src}->{dst}", o.check("cast")[0].reshape(-1), s.to(dst))


def case_gather(ops, dev, n, out_dtype, acc):
    """alpha = 1: exact.  Negative indices write 0 (accumulate = 0) or leave the old value bit for bit (accumulate = 1)."""
    gen = torch.Generator().manual_seed(1)
    src = torch.randn(5000, generator=gen)
    idx = torch.randint(-1, 5000, (n,), generator=gen, dtype=torch.int32)
    idx[0] = -1
    if n > 1:
        idx[n - 1], idx[n // 2] = -1, 4999
    base = torch.randn(n, generator=gen).to(out_dtype)
    o = Out(1, n + 11, [(0, n)], dev, out_dtype, pre=1, post=1, init=[base.reshape(1, n)])
    ops.gather(inflat(src, dev), inflat(idx, dev, torch.int32), o.views[0].reshape(-1), alpha=1.0, accumulate=acc)
    j = idx.long()
    val = src[j.clamp_min(0)]
    ref = torch.where(j >= 0, (base.float() + val).to(out_dtype), base) if acc else torch.where(j >= 0, val, torch.zeros(())).to(out_dtype)
    exact("out", o.check("gather")[0].reshape(-1), ref)


# ------------------------------------------------------------------------------------------------------------------ full fine-tuning
def case_im2col(ops, dev, mode):
    n_img, h, w, frames, c0, c1 = 4, 5, 8, 2, 8, 16
    C, taps = c0 + c1, (3 if mode == nt.GEMM_TCONV3 else 9)
    x = rnd(n_img * h * w, C, seed=1)
    if mode == nt.GEMM_TCONV3:
        x5 = F.pad(x.reshape(n_img // frames, frames, h * w, C), (0, 0, 0, 0, 1, 1))
        ref = torch.stack([x5[:, t:t + frames] for t in range(3)], dim=3).reshape(-1, 3 * C)
    else:
        x4 = x.reshape(n_img, h, w, C).permute(0, 3, 1, 2)
        u = {nt.GEMM_CONV3X3: lambda: F.unfold(x4, 3, padding=1), nt.GEMM_CONV3X3_S2: lambda: F.unfold(x4, 3, padding=1, stride=2),
             nt.GEMM_CONV3X3_S2_PAD01: lambda: F.unfold(F.pad(x4, (0, 1, 0, 1)), 3, stride=2),
             nt.GEMM_CONV3X3_UP2: lambda: F.unfold(F.interpolate(x4, scale_factor=2, mode="nearest"), 3, padding=1)}[mode]()
        ref = u.reshape(n_img, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)
    rows = ops.im2col_rows(mode, n_img, h, w)
    assert rows == ref.shape[0]
    x0, x1 = _parts(x, c0, c1, dev)
    out = Out(rows, taps * C + 8, [(0, taps * C)], dev)
    ops.im2col(x0, x1, mode, n_img, h, w, frames, out.views[0])
    exact("xcol", out.check("xcol")[0], ref.to(BF))


def case_norm_affine_grad(ops, dev, kind):
    units, rows, G, c0, c1, silu = 2, 21, 32, (40 if kind != 2 else 96), (24 if kind != 2 else 0), kind == 0
    C, M = c0 + c1, units * rows
    sum_rows = rows if kind == 2 else M
    x, gamma, beta = _gn_inputs(c0, c1, units, rows)
    dy = rnd(M, C, seed=3)
    g, xh, kw = dy, None, {}
    if kind == 0:
        mean, rstd = _gn_stats_ref(x, units, rows, G, 1e-5)
        mean, rstd = f32r(mean), f32r(rstd)
        rep = lambda t: t.repeat_interleave(C // G, dim=1)[:, None, :]  # noqa: E731
        xh = ((x.reshape(units, rows, C) - rep(mean)) * rep(rstd)).reshape(M, C)
        kw = dict(rows_per_unit=rows, groups=G, stats=_dev(torch.stack([mean, rstd], dim=2).reshape(units, 2 * G), dev).contiguous(),
                  gamma=_dev(gamma, dev), beta=_dev(beta, dev))
    elif kind == 1:
        xh = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + 1e-5)
        kw = dict(eps=1e-5)
    if silu:
        z = xh * gamma + beta
        sig = torch.sigmoid(z)
        g = g * sig * (1 + z * (1 - sig))
    n_out = M // sum_rows
    x0, x1 = _parts(x, c0, c1, dev) if kind != 2 else (None, None)
    ws = _ws(max(ops.norm_affine_grad_ws_floats(M, sum_rows, C), 1), dev)
    dg = Out(n_out, C + 4, [(0, C)], dev, F32) if kind != 2 else None
    db = Out(n_out, C + 12, [(4, C + 4)], dev, F32)
    ops.norm_affine_grad(x0, x1, inbuf(dy, C + 8, dev), kind=kind, sum_rows=sum_rows, ws=ws.views[0], dgamma=None if dg is None else dg.views[0],
                         dbeta=db.views[0], silu=silu, **kw)
    ws.guard("norm_affine_grad ws")
    ref = g.reshape(n_out, sum_rows, C).sum(dim=1)
    close("dbeta", db.check("dbeta")[0], ref, f32r(ref), STAT_TOL)
    if dg is not None:
        ref = (g * xh).reshape(n_out, sum_rows, C).sum(dim=1)
        close("dgamma", dg.check("dgamma")[0], ref, f32r(ref), STAT_TOL)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _x(M, C, ld, dev, col0=0):
    return inbuf(rnd(M, C, seed=9), ld, dev, col0=col0)


def _with_stride(t, ld):
    """The same base pointer with a (bad) row stride: only ever handed to an entry point that must refuse it before launching."""
    return torch.as_strided(t, t.shape, (ld, 1), t.storage_offset())


def refusal_cases(ops, dev):
    """-> [(name, thunk)]: every thunk makes ONE call that the entry point must refuse (checked against the T2V_REQUIRE lines: each
    refusal happens before any launch) and asserts that the sentinel-filled output is untouched."""
    M, C = 6, 64
    f32 = lambda n, s=0: _dev(rnd(n, seed=s + 20), dev)  # noqa: E731
    cases = []

    def mk(name, build):
        def thunk():
            call, outs = build()
            refuses(ops, call, *outs)
        cases.append((name, thunk))

    def ln(ldx, ldo):
        def build():
            out = Out(M, 80, [(0, 64)], dev)
            return (lambda: ops.layernorm(_with_stride(_x(M, 64, 72, dev), ldx), f32(64), f32(64, 1), 1e-5, _with_stride(out.views[0], ldo))), [out]
        return build

    def _wide(Cc):
        return _x(2, Cc, Cc + 8, dev)

    mk("layernorm ldx % 8", ln(68, 80))
    mk("layernorm ldo % 8", ln(72, 76))
    mk("layernorm ldx < C", ln(56, 80))
    mk("layernorm ldo < C", ln(72, 56))

    def lnb(ldx=72, ldy=72, ldr=72, ldo=80, Cc=64):
        def build():
            out = Out(M, 80, [(0, 64)], dev)
            if Cc == 64:
                x, dy, r, dx = _x(M, 64, 72, dev), _x(M, 64, 72, dev), _x(M, 64, 72, dev), out.views[0]
            else:
                big = Out(2, Cc + 8, [(0, Cc)], dev)
                x, dy, r, dx, out = _wide(Cc), _wide(Cc), _wide(Cc), big.views[0], big
                return (lambda: ops.layernorm_bwd(x, f32(Cc), 1e-5, dy, r, dx)), [out]
            return (lambda: ops.layernorm_bwd(_with_stride(x, ldx), f32(Cc), 1e-5, _with_stride(dy, ldy), _with_stride(r, ldr),
                                              _with_stride(dx, ldo))), [out]
        return build

    mk("layernorm_bwd ldy % 8", lnb(ldy=68))
    mk("layernorm_bwd ldx < C", lnb(ldx=56))
    mk("layernorm_bwd ldr < C", lnb(ldr=56))
    mk("layernorm_bwd ldo < C", lnb(ldo=56))
    mk("layernorm_bwd C = 2056", lnb(Cc=2056))

    def gn(which, ld0=72, ld1=72, ldo=136, ldy=136):
        def build():
            units, rows, G = 2, 3, 32
            x0, x1 = _with_stride(_x(M, 64, 72, dev), ld0 if which != "gn_bwd" else 72), _with_stride(_x(M, 64, 72, dev), ld1)
            out = Out(M, 136, [(0, 128)], dev)
            o = _with_stride(out.views[0], ldo)
            ws, st = _dev(torch.zeros(4096), dev), _dev(torch.ones(units, 2 * G), dev)
            g_, b_ = f32(128), f32(128, 1)
            if which == "group_norm":
                return (lambda: ops.group_norm(x0, x1, units, rows, 1e-5, g_, b_, True, ws, o, G)), [out]
            if which == "gn_apply":
                return (lambda: ops.gn_apply(x0, x1, units, rows, st, g_, b_, True, o, G)), [out]
            if which == "gn_stats":
                so = Out(1, units * 2 * G + 8, [(0, units * 2 * G)], dev, F32, pre=1, post=1)
                return (lambda: ops.gn_stats(x0, x1, units, rows, 1e-5, ws, so.views[0], G)), [so]
            dy = _with_stride(_x(M, 128, 136, dev), ldy)
            if which == "gn_bwd2":
                return (lambda: ops.gn_bwd(x0, units, rows, st, g_, b_, True, dy, None, ws, o, G, x1=x1)), [out]
            xs = _with_stride(_x(M, 128, 136, dev), ld0 if ld0 != 72 else 136)
            return (lambda: ops.gn_bwd(xs, units, rows, st, g_, b_, True, dy, None, ws, o, G)), [out]
        return build

    for which in ("group_norm", "gn_apply", "gn_stats", "gn_bwd2"):
        mk(f"{which} ld0 % 8", gn(which, ld0=68))
        mk(f"{which} ld1 < c1", gn(which, ld1=56))
    for which in ("group_norm", "gn_apply", "gn_bwd2", "gn_bwd"):
        mk(f"{which} ldo < C", gn(which, ldo=120))
    mk("gn_bwd ldx < C", gn("gn_bwd", ld0=120))
    mk("gn_bwd ldy < C", gn("gn_bwd", ldy=120))
    mk("gn_bwd2 ldy % 8", gn("gn_bwd2", ldy=132))

    def sm(bwd, n_pad, ld):
        def build():
            buf = Out(3, 72, [(0, 64)], dev)
            if bwd:
                return (lambda: ops.softmax_bwd_rows(_x(3, 64, 72, dev), buf.views[0], 3, 40, n_pad, ld)), [buf]
            return (lambda: ops.softmax_rows(buf.views[0], 3, 40, n_pad, ld)), [buf]
        return build

    for bwd in (False, True):
        nm = "softmax_bwd_rows" if bwd else "softmax_rows"
        mk(f"{nm} n_pad > ld", sm(bwd, 80, 72))
        mk(f"{nm} ld % 8", sm(bwd, 64, 68))
        mk(f"{nm} n_pad % 8", sm(bwd, 60, 72))

    def geglu(bwd, ldh=72, ldo=40, ldy=40):
        def build():
            h = _with_stride(_x(M, 64, 72, dev), ldh)
            if bwd:
                out = Out(M, 72, [(0, 64)], dev)
                return (lambda: ops.geglu_bwd(h, _with_stride(_x(M, 32, 40, dev), ldy), _with_stride(out.views[0], ldh))), [out]
            out = Out(M, 40, [(0, 32)], dev)
            return (lambda: ops.geglu_fwd(h, _with_stride(out.views[0], ldo))), [out]
        return build

    mk("geglu_fwd ldh % 8", geglu(False, ldh=68))
    mk("geglu_fwd ldh < 2 inner", geglu(False, ldh=56))
    mk("geglu_fwd ldo < inner", geglu(False, ldo=24))
    mk("geglu_bwd ldd < 2 inner", geglu(True, ldh=56))
    mk("geglu_bwd ldy < inner", geglu(True, ldy=24))
    mk("geglu_bwd ldy % 8", geglu(True, ldy=36))

    def addc(lda=72, ldo=72):
        def build():
            out = Out(M, 72, [(0, 64)], dev)
            return (lambda: ops.add(_with_stride(_x(M, 64, 72, dev), lda), _x(M, 64, 72, dev), _with_stride(out.views[0], ldo))), [out]
        return build

    mk("add lda % 8", addc(lda=68))
    mk("add lda < C", addc(lda=56))
    mk("add ldo < C", addc(ldo=56))

    def tp(pad, ld_in=72, ld_out=72, rows=6):
        def build():
            out = Out(64, 72, [(0, 64)], dev)
            fn = ops.transpose_pad if pad else ops.transpose
            return (lambda: fn(_with_stride(_x(6, 64, 72, dev), ld_in), rows, 64, _with_stride(out.views[0], ld_out))), [out]
        return build

    mk("transpose ld_in < cols", tp(False, ld_in=56))
    mk("transpose ld_out < rows", tp(False, ld_out=4))
    mk("transpose_pad ld_in % 8", tp(True, ld_in=68))
    mk("transpose_pad ld_out < roundup(rows, 64)", tp(True, ld_out=56))
    mk("transpose_pad ld_in < cols", tp(True, ld_in=56))

    def attn_t(bwd, frames=4, ldq=384, ldo=136, ldg=392):
        def build():
            clips, hw, heads, inner = 1, 2, 2, 128
            Mt = clips * 4 * hw
            qkv = _with_stride(_x(Mt, 128, 384, dev), ldq)
            if not bwd:
                out = Out(Mt, 136, [(0, 128)], dev)
                return (lambda: ops.attn_temporal(qkv, qkv, qkv, _with_stride(out.views[0], ldo), clips, frames, hw, heads, 0.125)), [out]
            g = Out(Mt, 392, [(0, 128), (128, 256), (256, 384)], dev)
            gv = [_with_stride(v, ldg) for v in g.views]
            return (lambda: ops.attn_temporal_bwd(qkv, qkv, qkv, _with_stride(_x(Mt, 128, 136, dev), ldo), None, *gv, clips, frames, hw, heads, 0.125)), [g]
        return build

    mk("attn_temporal ldq % 8", attn_t(False, ldq=388))
    mk("attn_temporal ldq < inner", attn_t(False, ldq=120))
    mk("attn_temporal ldo < inner", attn_t(False, ldo=120))
    mk("attn_temporal_bwd frames = 17", attn_t(True, frames=17))
    mk("attn_temporal_bwd ldq % 8", attn_t(True, ldq=388))
    mk("attn_temporal_bwd dq stride % 4", attn_t(True, ldg=390))
    mk("attn_temporal_bwd dq stride < inner", attn_t(True, ldg=120))
    mk("attn_temporal_bwd ldo < inner", attn_t(True, ldo=120))

    def attn_s(ldq=256, ld_vt=64, ldo=132, stride=0):
        def build():
            n_img, seq, heads = 1, 40, 2
            qk = _x(seq, 256, 256, dev)
            vt = _dev(torch.zeros(128 * 64 + 64), dev, BF)
            out = Out(seq, 132, [(0, 128)], dev)
            return (lambda: ops.attn_spatial(_with_stride(qk[:, :128], ldq), qk[:, 128:], vt, ld_vt, _with_stride(out.views[0], ldo), n_img, seq, seq,
                                             heads, 1, 0.125, vt_img_stride=stride)), [out]
        return build

    mk("attn_spatial ldq % 8", attn_s(ldq=260))
    mk("attn_spatial ldq < inner", attn_s(ldq=120))
    mk("attn_spatial ldo % 4", attn_s(ldo=130))
    mk("attn_spatial ldo < inner", attn_s(ldo=124))
    mk("attn_spatial ld_vt < padded seq", attn_s(ld_vt=56))
    mk("attn_spatial vt_img_stride % 8", attn_s(stride=128 * 64 + 4))

    def attn_sb(**bad):
        def build():
            n_img, seq, heads, inner, sp = 1, 40, 2, 128, 64
            a = dict(ldq=256, ld_kt=64, ld_qt=128, ld_stat=72, lddq=256, lddv=136, ldv=136, ldo=136)
            a.update(bad)
            qk, v, do, o = _x(seq, 256, 256, dev), _x(seq, 128, 136, dev), _x(seq, 128, 136, dev), _x(seq, 128, 136, dev)
            kt, qt, dot = (_dev(torch.zeros(128, 128), dev, BF) for _ in range(3))
            l2, ds = Out(heads, 72, [(0, seq)], dev, F32), Out(heads, 72, [(0, seq)], dev, F32)
            g, gv = Out(seq, 256, [(0, 128), (128, 256)], dev), Out(seq, 136, [(0, 128)], dev)
            p = lambda t: t.data_ptr()  # noqa: E731
            return (lambda: ops._call("t2v_attn_spatial_bwd", p(qk), a["ldq"], p(qk[:, 128:]), 256, p(v), a["ldv"], seq * 136, 64, p(kt), a["ld_kt"],
                                      p(qt), p(dot), a["ld_qt"], p(do), a["ldo"], p(o), 136, p(l2.views[0]), p(ds.views[0]), a["ld_stat"],
                                      p(g.views[0]), a["lddq"], p(g.views[1]), 256, p(gv.views[0]), a["lddv"], n_img, seq, seq, heads, 0.125)), [g, gv, l2, ds]
        return build

    mk("attn_spatial_bwd ldq % 8", attn_sb(ldq=260))
    mk("attn_spatial_bwd ldq < inner", attn_sb(ldq=120))
    mk("attn_spatial_bwd ld_kt < padded seq", attn_sb(ld_kt=56))
    mk("attn_spatial_bwd ld_qt < padded seq", attn_sb(ld_qt=56))
    mk("attn_spatial_bwd ld_stat < seq", attn_sb(ld_stat=32))
    mk("attn_spatial_bwd lddq % 4", attn_sb(lddq=258))
    mk("attn_spatial_bwd lddv < inner", attn_sb(lddv=120))
    mk("attn_spatial_bwd ldo < inner", attn_sb(ldo=120))

    def im2col(ld0=16, ldo=9 * 24 + 8):
        def build():
            n_img, h, w = 1, 2, 2
            x0, x1 = _with_stride(_x(4, 8, 16, dev), ld0), _x(4, 16, 24, dev)
            out = Out(4, 9 * 24 + 8, [(0, 9 * 24)], dev)
            return (lambda: ops.im2col(x0, x1, nt.GEMM_CONV3X3, n_img, h, w, 0, _with_stride(out.views[0], ldo))), [out]
        return build

    mk("im2col ld0 % 8", im2col(ld0=12))
    mk("im2col ld0 < c0", im2col(ld0=0))
    mk("im2col ldo < taps * C", im2col(ldo=9 * 24 - 8))

    def nag(ldy=72, ld0=72, ld_db=68):
        def build():
            db, ws = Out(1, 68, [(0, 64)], dev, F32), _dev(torch.zeros(4096), dev)
            dg = Out(1, 68, [(0, 64)], dev, F32)
            return (lambda: ops.norm_affine_grad(_with_stride(_x(M, 64, 72, dev), ld0), None, _with_stride(_x(M, 64, 72, dev), ldy), kind=1, sum_rows=M,
                                                 ws=ws, dgamma=dg.views[0], dbeta=_with_stride(db.views[0], ld_db), eps=1e-5)), [db, dg]
        return build

    mk("norm_affine_grad ldy % 8", nag(ldy=68))
    mk("norm_affine_grad ldy < C", nag(ldy=56))
    mk("norm_affine_grad ld0 < c0", nag(ld0=56))
    mk("norm_affine_grad ld_dbeta < C", nag(ld_db=32))
    return cases


# ------------------------------------------------------------------------------------------------------------------ the table
def _cases():
    c = []
    for seq in (7, 40, 64, 130):
        for lay in ("tok", "head"):
            for dist in ("mild", "peaked"):
                c.append((f"attn_spatial_bwd-{seq}-{lay}-{dist}", case_attn_spatial_bwd, dict(seq=seq, v_layout=lay, dist=dist)))
    c.append(("attn_spatial_bwd-q130-kv77-raw", case_attn_spatial_bwd, dict(seq=130, v_layout="tok", dist="mild", seq_kv=77)))
    for shp in ((2, 40, 40, 2, 1), (4, 130, 77, 2, 2)):
        c.append(("attn_spatial-" + "-".join(map(str, shp)), case_attn_spatial, dict(zip(("n_img", "seq_q", "seq_kv", "heads", "kv_div"), shp))))
    for frames, hw in ((1, 9), (5, 33), (16, 1), (16, 40)):
        for flag in (False, True):
            c.append((f"attn_temporal-{frames}-{hw}-probs{int(flag)}", case_attn_temporal, dict(frames=frames, hw=hw, with_probs=flag)))
            c.append((f"attn_temporal_bwd-{frames}-{hw}-dprobs{int(flag)}", case_attn_temporal_bwd, dict(frames=frames, hw=hw, with_dprobs=flag)))
    for M, C in ((1, 8), (5, 64), (37, 320), (9, 2048), (7, 4096)):
        c.append((f"layernorm-{M}-{C}", case_layernorm, dict(M=M, C=C)))
        if C <= 2048:
            c.append((f"layernorm_bwd-{M}-{C}", case_layernorm_bwd, dict(M=M, C=C)))
    c.append(("layernorm-mean30", case_layernorm, dict(M=5, C=320, shifted=True)))
    c.append(("layernorm_bwd-mean30", case_layernorm_bwd, dict(M=5, C=320, shifted=True)))
    c.append(("layernorm_bwd-noresid", case_layernorm_bwd, dict(M=5, C=64, resid=False)))
    for c0, c1 in ((320, 0), (168, 152), (1280, 640)):
        for rows in (1, 40, 77):
            for silu in (False, True):
                c.append((f"group_norm-{c0}+{c1}-{rows}-silu{int(silu)}", case_group_norm, dict(c0=c0, c1=c1, rows=rows, silu=silu)))
                c.append((f"gn_bwd-{c0}+{c1}-{rows}-silu{int(silu)}", case_gn_bwd, dict(c0=c0, c1=c1, rows=rows, silu=silu)))
    for shp in ((3, 40, 64, 72), (5, 77, 128, 136), (4, 2560, 2560, 2568)):
        kw = dict(zip(("rows", "n", "n_pad", "ld"), shp))
        c.append(("softmax_rows-" + "-".join(map(str, shp)), case_softmax_rows, kw))
        c.append(("softmax_bwd_rows-" + "-".join(map(str, shp)), case_softmax_bwd_rows, kw))
    for M, inner in ((1, 32), (70, 96)):
        c.append((f"geglu_fwd-{M}-{inner}", case_geglu_fwd, dict(M=M, inner=inner)))
        c.append((f"geglu_bwd-{M}-{inner}", case_geglu_bwd, dict(M=M, inner=inner)))
    c.append(("add", case_add, {}))
    for rows in (1, 63, 64, 65):
        c.append((f"transpose_pad-{rows}", case_transpose, dict(rows=rows, cols=72, batch=2, pad=True)))
    c.append(("transpose-70x100x3", case_transpose, dict(rows=70, cols=100, batch=3, pad=False)))
    c.append(("sumpool_scatter", case_sumpool_scatter, {}))
    c.append(("layout_cast", case_layout_cast, {}))
    for n in (1, 4097):
        for dt in (F32, BF):
            for acc in (False, True):
                c.append((f"gather-{n}-{'f32' if dt == F32 else 'bf16'}-acc{int(acc)}", case_gather, dict(n=n, out_dtype=dt, acc=acc)))
    for mode in (nt.GEMM_CONV3X3, nt.GEMM_CONV3X3_S2, nt.GEMM_CONV3X3_S2_PAD01, nt.GEMM_CONV3X3_UP2, nt.GEMM_TCONV3):
        c.append((f"im2col-mode{mode}", case_im2col, dict(mode=mode)))
    for kind in (0, 1, 2):
        c.append((f"norm_affine_grad-kind{kind}", case_norm_affine_grad, dict(kind=kind)))
    return c


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
REFUSAL_IDS = [n for n, _ in refusal_cases(None, None)]   # (the thunks touch ops / dev only when called)


def run(ops, dev, name, fn, kw):
    _CUR[0] = name
    fn(ops, dev, **kw)


def report_lines():
    return [f"{c:44s} {t:22s} rounding {m:.2e}  bound {b:.2e}  observed {e:.2e}" for c, t, m, b, e in REPORT]


def run_refusal(ops, dev, name, table=None):
    """``table``: another module's refusal table of the same form (tests/gemm_form_cases.py)."""
    dict((table or refusal_cases)(ops, dev))[name]()
