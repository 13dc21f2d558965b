"""GroupNorm from the producers' COLUMN STATISTICS — t2v_group_norm_cs, t2v_gn_stats_cs, t2v_gn_coef_cs, t2v_gn_coef_cs_supported — by
statistics form, with poisoned padding: one table, two backends (tests/test_hostsim_norm_cs.py: the host SIMT simulator,
tests/test_gpu_norm_cs.py: the device).  Helpers, poison / guard discipline, metric and bound rule are those of
tests/operand_form_cases.py (imported, not copied).

Operands.  ``cs`` [rows / 32][c][2] per part = (sum, sum of squares) of the bf16 tensor per 32-row slab, formed in fp64 and rounded to fp32:
what the kernel receives.  Every array is a view into a NaN-framed flat buffer, 16-byte aligned or offset by two floats (8-byte aligned:
the partial-sums form) — by one float only where the call must be refused.  The tensor parts are row-strided views with NaN gaps and spare
rows, the output has stride gaps and spare rows, ``stats`` / ``coef`` sit in sentinel-framed flat buffers, the workspace is
t2v_group_norm_cs_ws_floats floats followed by a sentinel tail.  The statistics-only cases draw slab sums directly (a slab mean and a slab
variance per channel): they need no tensor, so many slabs cost nothing.

Reference.  The header's definition in fp64 FROM THE fp32 cs ENTRIES (and the bf16 tensor): mean = S / n, var = max(Q / n - mean^2, 0),
rstd = 1 / sqrt(var + eps), y = (x - mean) rstd gamma + beta (then SiLU), coef[u][0][c] = rstd gamma, coef[u][1][c] = beta - mean rstd gamma.
Rounded model: bf16 of the reference for the tensor; for stats / coef the same definition on per-channel slab sums accumulated in fp32 in
slab order, rounded to fp32.  Bound = max(tolerance, 2 x the metric of the rounded model): BF16_TOL for the tensor, STAT_TOL for
stats / coef, from the reference alone at run time.

Forms (conditions read off gn_csd_threads / t2v_group_norm_cs; each case asserts t2v_gn_coef_cs_supported's answer so that a change of the
selection rule cannot move it off its branch unnoticed):
  direct, 256 threads        C = 320, 2 slabs; (328, 56): group 27 (channels 324 .. 335) straddles the parts; 400 slabs: the 8-in-flight trip + tail
  direct, 1 024 threads      (1280, 1280) x 1 600 rows, one unit (50 slabs, 6 lanes at 256 threads -> 9 loads); groups = 2: C = 512 x 17 slabs
                             (9 loads at 256 threads), C = 640 / 1 024 x 2 slabs (more than 256 channels per group: the coefficients of
                             channels >= 256 of a group were never written before gn_csd_threads took 1 024 threads there)
  partial sums               cs offset by two floats (3 slabs: 1 per block; 402 slabs: 6 per block = the 4-in-flight trip + tail); odd
                             channels per group (C = 96: 3, (96, 64): 5); C = 2 688 > 80 groups (tensor form only: its stats / coef calls
                             run direct); 801 slabs of C = 2 560 (33 per thread at 1 024 threads); C = 256 x 4 100 slabs (16-byte pieces of
                             16.8 MB of statistics)
one input with its mean far from zero (shift 8, spread 0.5) per form; a second call must give the same bits (one case per form).

Worst row per tensor (maximum over the cases), as in tests/operand_form_cases.py: rounding = the metric of the rounded model against the
fp64 reference, bound = what the cases assert, then the worst row observed on the host simulator and on an MI355X:

    family                     tensor             cases  rounding  bound     simulator  MI355X
    gn_stats_cs                stats               17    4.9e-06   1.0e-04   1.0e-06    1.0e-06
    gn_coef_cs                 coef                10    2.3e-05   1.0e-04   4.8e-06    4.8e-06
    group_norm_cs              out                  9    2.4e-03   4.7e-03   2.4e-03    2.4e-03
    the second call of the determinism cases (stats, coef, out): bit for bit on both backends

Every case runs on both backends (the largest, 4.1 M elements, takes the simulator about a second).
"""
import math

import torch
import torch.nn.functional as F

from tests.operand_form_cases import (BF16_TOL, NAN, REPORT, STAT_TOL, F32, Out, _CUR, _dev, _parts, _with_stride, _ws, bfr, close, exact, f32r,
                                      refuses, rnd)

G32, EPS = 32, 1e-5
EPS64 = float(torch.tensor(EPS, dtype=F32))   # (the entry points take eps as a float)


# ------------------------------------------------------------------------------------------------------------------ operands
def _csbuf(cs, dev, off=0):
    """``cs`` (fp32, contiguous) inside a NaN-framed flat buffer, ``off`` floats past a 16-byte boundary."""
    if cs is None:
        return None
    n, pad = cs.numel(), 16 + off
    full = torch.full((n + 2 * pad,), NAN, dtype=F32)
    full[pad:pad + n] = cs.reshape(-1)
    v = full.to(dev)[pad:pad + n].view(cs.shape)
    assert v.data_ptr() % 16 == 4 * off % 16
    return v


def _cs_of(x, c0):
    """x fp64 [M, C] (bf16 values) -> fp32 (cs0 [M / 32, c0, 2], cs1 [M / 32, C - c0, 2] or None)."""
    M, C = x.shape
    s = x.reshape(M // 32, 32, C)
    cs = torch.stack([s.sum(dim=1), (s * s).sum(dim=1)], dim=2).to(F32)
    return cs[:, :c0].contiguous(), (cs[:, c0:].contiguous() if c0 < C else None)


def _cs_synth(units, slabs, C, seed, shift=0.0):
    """Slab sums of a tensor nobody builds: per (unit, channel) a mean and a spread (different per unit), per slab a sample mean and a
    sample variance around them.  -> fp32 [units * slabs, C, 2]."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    u = torch.arange(units, dtype=torch.float64)[:, None, None]
    mu = 0.3 * r(units, 1, C) + shift + 3.0 * u
    sd = (1.0 + 0.5 * u) * (0.5 + torch.rand(units, 1, C, generator=g, dtype=torch.float64)) * (0.5 if shift else 1.0)
    m = mu + sd * r(units, slabs, C) / math.sqrt(32.0)
    v = sd * sd * (1.0 + 0.25 * r(units, slabs, C)).abs()
    return torch.stack([32.0 * m, 32.0 * (v + m * m)], dim=3).reshape(units * slabs, C, 2).to(F32)


def _inputs(c0, c1, units, rows, shifted):
    C, M = c0 + c1, units * rows
    x = rnd(M, C, seed=1, scale=0.5, shift=8.0) if shifted else rnd(M, C, seed=1)
    for u in range(units):   # every unit its own mean and spread: the row after a unit boundary must be normalised with ITS unit's statistics
        x[u * rows:(u + 1) * rows] = bfr(x[u * rows:(u + 1) * rows] + 1.0 * u) if shifted else bfr(x[u * rows:(u + 1) * rows] * (1.0 + 0.5 * u) + 3.0 * u)
    return x, f32r(rnd(C, seed=5, scale=0.2, shift=1.0)), f32r(rnd(C, seed=6, scale=0.1))


# ------------------------------------------------------------------------------------------------------------------ reference
def _finish(t, units, G, rows):
    """t fp64 [units, C, 2] per-channel sums -> (mean, rstd) fp64 [units, G]: the header's definition."""
    C = t.shape[1]
    g = t.reshape(units, G, C // G, 2).sum(dim=2)
    n = float(rows * (C // G))
    mean = g[..., 0] / n
    var = (g[..., 1] / n - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + EPS64)


def _stats_ref(cs, units, G, rows):
    """cs fp32 [units * slabs, C, 2] (the parts side by side) -> ((mean, rstd) in fp64, the same from per-channel sums accumulated in
    fp32 in slab order)."""
    C = cs.shape[1]
    c = cs.reshape(units, -1, C, 2)
    acc = torch.zeros(units, C, 2, dtype=F32)
    for s in range(c.shape[1]):
        acc = acc + c[:, s]
    return _finish(c.double().sum(dim=1), units, G, rows), _finish(acc.double(), units, G, rows)


def _coef_of(mean, rstd, gamma, beta, C):
    """-> fp64 [units, 2, C]"""
    rep = lambda t: t.repeat_interleave(C // mean.shape[1], dim=1)  # noqa: E731
    a = rep(rstd) * gamma
    return torch.stack([a, beta - rep(mean) * a], dim=1)


def _flat_out(n, dev):
    return Out(1, n + 8, [(0, n)], dev, F32, pre=1, post=1)


def _check_stats_coef(ops, dev, cs0_d, cs1_d, c0, c1, units, rows, G, cs_full, gamma, beta, sup, twice):
    """t2v_gn_stats_cs and, where the direct form takes the shape, t2v_gn_coef_cs on the same statistics."""
    C = c0 + c1
    (mean, rstd), (mean_r, rstd_r) = _stats_ref(cs_full, units, G, rows)
    st_ref, st_rr = torch.stack([mean, rstd], dim=2).reshape(units, 2 * G), torch.stack([mean_r, rstd_r], dim=2).reshape(units, 2 * G)
    runs = []
    for _ in range(2 if twice else 1):
        ws = _ws(ops.group_norm_cs_ws_floats(units, rows, G), dev)
        st = _flat_out(units * 2 * G, dev)
        ops.gn_stats_cs(cs0_d, cs1_d, c0, c1, units, rows, EPS, ws.views[0], st.views[0], G)
        ws.guard("gn_stats_cs ws")
        runs.append(st.check("stats")[0].reshape(units, 2 * G))
    close("stats", runs[0], st_ref, f32r(st_rr), STAT_TOL)
    if twice:
        exact("stats again", runs[1], runs[0])
    if not sup:
        return mean, rstd
    g_d, b_d = _dev(gamma, dev), _dev(beta, dev)
    runs = []
    for _ in range(2 if twice else 1):
        co = _flat_out(units * 2 * C, dev)
        ops.gn_coef_cs(cs0_d, cs1_d, c0, c1, units, rows, EPS, g_d, b_d, co.views[0], G)
        runs.append(co.check("coef")[0].reshape(units * 2, C))
    close("coef", runs[0], _coef_of(mean, rstd, gamma, beta, C).reshape(units * 2, C),
          f32r(_coef_of(mean_r, rstd_r, gamma, beta, C)).reshape(units * 2, C), STAT_TOL)
    if twice:
        exact("coef again", runs[1], runs[0])
    return mean, rstd


# ------------------------------------------------------------------------------------------------------------------ cases
def case_tensor(ops, dev, c0, c1, rows, silu, form, units=2, cs_off=0, shifted=False, twice=False, sup=None):
    """t2v_group_norm_cs, then t2v_gn_stats_cs and t2v_gn_coef_cs (where supported) on the same cs.  ``form``: the statistics form
    t2v_group_norm_cs takes (direct needs the supported answer AND 2 C <= the workspace floats per unit), ``sup``: the answer of
    t2v_gn_coef_cs_supported where it differs from that."""
    G, C, M = G32, c0 + c1, units * rows
    sup = (form == "direct") if sup is None else sup
    x, gamma, beta = _inputs(c0, c1, units, rows, shifted)
    cs0, cs1 = _cs_of(x, c0)
    cs0_d, cs1_d = _csbuf(cs0, dev, cs_off), _csbuf(cs1, dev, cs_off)
    assert ops.gn_coef_cs_supported(cs0_d, cs1_d, c0, c1, units, rows, G) == sup, "the case left its statistics form"
    assert (sup and C <= G * 80) == (form == "direct")
    cs_full = cs0 if cs1 is None else torch.cat([cs0, cs1], dim=1)
    mean, rstd = _check_stats_coef(ops, dev, cs0_d, cs1_d, c0, c1, units, rows, G, cs_full, gamma, beta, sup, twice)
    coef = _coef_of(mean, rstd, gamma, beta, C)
    y = (x.reshape(units, rows, C) * coef[:, 0][:, None, :] + coef[:, 1][:, None, :]).reshape(M, C)
    ref = F.silu(y) if silu else y
    x0, x1 = _parts(x, c0, c1, dev)
    g_d, b_d = _dev(gamma, dev), _dev(beta, dev)
    runs = []
    for _ in range(2 if twice else 1):
        ws = _ws(ops.group_norm_cs_ws_floats(units, rows, G), dev)
        out = Out(M, C + 8, [(0, C)], dev)
        ops.group_norm_cs(cs0_d, cs1_d, x0, x1, units, rows, EPS, g_d, b_d, silu, ws.views[0], out.views[0], G)
        ws.guard("group_norm_cs ws")
        runs.append(out.check("group_norm_cs out")[0])
    close("out", runs[0], ref, bfr(ref), BF16_TOL)
    if twice:
        exact("out again", runs[1], runs[0])


def case_stats(ops, dev, C, slabs, form, groups=G32, units=2, cs_off=0, shifted=False, twice=False):
    """t2v_gn_stats_cs and (direct form) t2v_gn_coef_cs on drawn slab sums: no tensor."""
    rows = slabs * 32
    cs = _cs_synth(units, slabs, C, seed=3, shift=8.0 if shifted else 0.0)
    cs_d = _csbuf(cs, dev, cs_off)
    sup = form == "direct"
    assert ops.gn_coef_cs_supported(cs_d, None, C, 0, units, rows, groups) == sup, "the case left its statistics form"
    gamma, beta = f32r(rnd(C, seed=5, scale=0.2, shift=1.0)), f32r(rnd(C, seed=6, scale=0.1))
    _check_stats_coef(ops, dev, cs_d, None, C, 0, units, rows, groups, cs, gamma, beta, sup, twice)


# ------------------------------------------------------------------------------------------------------------------ refusals
def refusal_cases(ops, dev):
    """-> [(name, thunk)]: ONE call each that the entry point must refuse before any launch, every output sentinel-filled and untouched
    afterwards.  Every allocation is large enough for the call as if it had been accepted."""
    cases = []

    def mk(name, build):
        def thunk():
            call, outs = build()
            refuses(ops, call, *outs)
        cases.append((name, thunk))

    def operands(c0, c1, units, rows, cs_rows, cs_off=0):
        x, gamma, beta = _inputs(c0, c1, units, cs_rows, False)
        cs0, cs1 = _cs_of(x, c0)
        x0, x1 = _parts(x[:units * rows], c0, c1, dev)
        return _csbuf(cs0, dev, cs_off), _csbuf(cs1, dev, cs_off), x0, x1, _dev(gamma, dev), _dev(beta, dev)

    def gn(c0=64, c1=0, units=2, rows=32, cs_rows=None, cs_off=0, no_cs1=False, ldo=None):
        def build():
            C = c0 + c1
            cs0, cs1, x0, x1, g_d, b_d = operands(c0, c1, units, rows, cs_rows or rows, cs_off)
            ws = _ws(ops.group_norm_cs_ws_floats(units, rows, G32), dev)
            out = Out(units * rows, C + 8, [(0, C)], dev)
            o = out.views[0] if ldo is None else _with_stride(out.views[0], ldo)
            return (lambda: ops.group_norm_cs(cs0, None if no_cs1 else cs1, x0, x1, units, rows, EPS, g_d, b_d, True, ws.views[0], o, G32)), [out, ws]
        return build

    def stats(C=64, units=2, rows=32, cs_rows=None, cs_off=0, coef=False):
        def build():
            cs0, _, _, _, g_d, b_d = operands(C, 0, units, rows, cs_rows or rows, cs_off)
            ws = _ws(ops.group_norm_cs_ws_floats(units, rows, G32), dev)
            if coef:
                co = _flat_out(units * 2 * C, dev)
                return (lambda: ops.gn_coef_cs(cs0, None, C, 0, units, rows, EPS, g_d, b_d, co.views[0], G32)), [co]
            st = _flat_out(units * 2 * G32, dev)
            return (lambda: ops.gn_stats_cs(cs0, None, C, 0, units, rows, EPS, ws.views[0], st.views[0], G32)), [st, ws]
        return build

    mk("group_norm_cs rows_per_unit % 32", gn(rows=40, cs_rows=64))
    mk("gn_stats_cs rows_per_unit % 32", stats(rows=40, cs_rows=64))
    mk("gn_coef_cs rows_per_unit % 32", stats(rows=40, cs_rows=64, coef=True))
    mk("group_norm_cs cs0 4-byte aligned", gn(cs_off=1))
    mk("gn_stats_cs cs0 4-byte aligned", stats(cs_off=1))
    mk("gn_coef_cs cs0 4-byte aligned", stats(cs_off=1, coef=True))
    mk("group_norm_cs c1 without cs1", gn(c0=64, c1=64, no_cs1=True))

    def coef_unsupported():
        call, outs = stats(C=96, rows=96, coef=True)()
        cs0 = operands(96, 0, 2, 96, 96)[0]
        assert not ops.gn_coef_cs_supported(cs0, None, 96, 0, 2, 96, G32)
        return call, outs
    mk("gn_coef_cs where _supported answers 0", coef_unsupported)
    mk("gn_stats_cs C > 4096", stats(C=4128, units=1))
    mk("group_norm_cs ldo < C", gn(c0=64, c1=64, ldo=120))
    return cases


# ------------------------------------------------------------------------------------------------------------------ the table
def _cases():
    c = []
    t = lambda name, **kw: c.append(("tensor-" + name, case_tensor, kw))  # noqa: E731
    s = lambda name, **kw: c.append(("stats-" + name, case_stats, kw))  # noqa: E731
    t("320-64-direct256", c0=320, c1=0, rows=64, silu=True, form="direct", twice=True)
    t("328+56-96-direct256-straddle", c0=328, c1=56, rows=96, silu=False, form="direct")
    t("1280+1280-1600-direct1024", c0=1280, c1=1280, rows=1600, silu=True, form="direct", units=1)
    t("320-96-partial-cs8", c0=320, c1=0, rows=96, silu=True, form="partial", cs_off=2, twice=True)
    t("96-96-partial-cpg3", c0=96, c1=0, rows=96, silu=False, form="partial")
    t("96+64-96-partial-cpg5", c0=96, c1=64, rows=96, silu=True, form="partial")
    t("2688-64-partial-wide", c0=2688, c1=0, rows=64, silu=False, form="partial", sup=True)
    t("320-64-direct256-mean8", c0=320, c1=0, rows=64, silu=False, form="direct", shifted=True)
    t("96-96-partial-mean8", c0=96, c1=0, rows=96, silu=True, form="partial", shifted=True)
    s("320-400slabs-direct256-trip8", C=320, slabs=400, form="direct")
    s("512-17slabs-g2-direct1024", C=512, slabs=17, form="direct", groups=2, twice=True)
    s("320-402slabs-partial-cs8-trip4", C=320, slabs=402, form="partial", cs_off=2)
    s("2560-801slabs-partial", C=2560, slabs=801, form="partial")
    s("256-4100slabs-partial-8MB", C=256, slabs=4100, form="partial")
    s("640-2slabs-g2-direct1024-cpg320", C=640, slabs=2, form="direct", groups=2)
    s("1024-2slabs-g2-direct1024-cpg512", C=1024, slabs=2, form="direct", groups=2)
    s("320-400slabs-direct256-mean8", C=320, slabs=400, form="direct", shifted=True)
    return c


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
REFUSAL_IDS = [n for n, _ in refusal_cases(None, None)]   # (the thunks touch ops / dev only when called)


def run(ops, dev, name, fn, kw):
    _CUR[0] = name
    fn(ops, dev, **kw)


def run_refusal(ops, dev, name):
    dict(refusal_cases(ops, dev))[name]()


def report_lines():
    return [f"{c:44s} {t:22s} rounding {m:.2e}  bound {b:.2e}  observed {e:.2e}" for c, t, m, b, e in REPORT]
