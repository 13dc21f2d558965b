"""The FLAT step kernels against their definitions — t2v_adamw_step, t2v_ema_update, t2v_sumsq (the oracles of t2v_adamw_multi /
t2v_adamw8_step, t2v_ema_multi and t2v_sumsq_multi), t2v_quant8_blockwise / t2v_dequant8_blockwise, and the scheduler family t2v_lcm_step,
t2v_lincomb3, t2v_silu, t2v_timestep_embedding[_f32]: one table, two backends (tests/test_hostsim_step_kernels.py: the host SIMT simulator,
tests/test_gpu_step_kernels.py: the device).  Helpers, poison / guard discipline and the ``close`` bound rule are those of
tests/operand_form_cases.py (imported, not copied).

Every buffer is a sentinel- or NaN-framed flat allocation (``inflat`` for inputs, an ``Out`` of one row for outputs and in / out buffers):
must-write regions start as NaN (0xFF for code bytes) and must come back finite, in / out buffers start from their values, frames are
compared bit for bit afterwards, inputs are never written (``grad`` is checked for it).  Sizes: 1, 3, 4, 5, 255, 256, 257, 1023, 1025 and per
kernel one that takes a second block / the grid-stride loop; views 0, 1 or 3 elements past a 16-byte boundary where the entry point
allows it, and one refusal where it does not.

References (never tests/emu_ops.py, never a path that can call the kernel under test):
  adamw_step    torch.optim.AdamW's arithmetic in fp64 on the fp32-rounded scalars, bc1 / sqrt(bc2) formed in fp32 as the entry point forms
                them; p, m, v within RTOL, ATOL = 1e-6, 1e-7 (tests/adamw_cases.py, tests/optim8_util.py) per element
  ema_update    t * rate + s * (1 - rate) in numpy float32, every product and the sum rounded on its own: BIT FOR BIT (the kernel's
                contraction-off expression); and fp64 within RTOL, ATOL
  sumsq         the fp64 sum, STAT_TOL; exactly min(ceil(n / 256), 1024) workspace floats written; a second call gives the same bits
  quant8        optim.quantize_blockwise / dequantize_blockwise on CPU tensors (the definition): absmax bit for bit, codes differ by at most
                1 on at most 1e-3 n + 1 elements, padding bytes = the code of 0, dequant bit for bit
  lcm_step, lincomb3   the header's lines in fp64; ``close`` with the fp32-rounded reference as model and 1e-6
  silu          fp64, bf16-rounded model, BF16_TOL
  timestep_embedding[_f32]   per ELEMENT |err| <= 2^-9 [bf16 output] + 4e-6 |a| + 2e-6, a = the argument of sin / cos: the fp32 chain
                logf * i / half -> expf -> * t carries at most about 2e-6 relative error into a (three roundings of a value up to 9.2, then a
                2-ulp expf), 2^-9 is half a bf16 ulp below 1, the factor 2 is margin for the device's sincosf

Worst row per family (maximum over the family's cases); rounding = the metric of the rounded model against the fp64 reference, bound = what
the cases assert, then the worst observed on the host simulator and on an MI355X (adamw / ema fp64 / timestep_embedding: the largest
|err| / allowance over the elements, bound 1):

    family                     tensor             cases  rounding  bound     simulator  MI355X
    adamw_step                 p                   20    0.0e+00   1.0e+00   1.2e-01    6.4e-02
    adamw_step                 m                   20    0.0e+00   1.0e+00   4.3e-02    4.3e-02
    adamw_step                 v                   20    0.0e+00   1.0e+00   1.8e-02    1.8e-02
    ema_update                 target fp64         18    0.0e+00   1.0e+00   9.6e-02    9.6e-02
    sumsq                      sumsq               12    4.0e-08   1.0e-04   1.1e-07    1.1e-07
    quant8                     codes               26    0.0e+00   2.1e+03   0.0e+00    0.0e+00
    lcm_step                   denoised            12    3.0e-08   1.0e-06   5.0e-08    4.6e-08
    lcm_step                   prev                12    3.0e-08   1.0e-06   6.6e-08    6.1e-08
    lincomb3                   out                 18    3.6e-08   1.0e-06   5.2e-08    5.2e-08
    silu                       out                  3    1.5e-03   4.0e-03   1.5e-03    1.5e-03
    timestep_embedding         embedding bf16       4    0.0e+00   1.0e+00   1.0e+00    1.0e+00
    timestep_embedding         embedding f32        4    0.0e+00   1.0e+00   1.0e-01    1.0e-01
    (quant8 codes: the number of codes that differ from the definition's, bound = the largest allowance 1e-3 n + 1; the bf16 embedding sits at
    its allowance because half a bf16 ulp IS the allowance: the fp32 row shows what the arithmetic alone uses of it)
    adamw_step grad, ema_update target (numpy float32), sumsq's second call, quant8 absmax and dequant, lcm_step prev == denoised without
    noise: bit for bit on both backends

Every case runs on both backends (``quant8-2097413-*``, 8 193 quantisation blocks for the grid-stride loop of the 2 048-workgroup
persistent grid, takes the simulator about a second).
"""
import numpy as np
import torch
import torch.nn.functional as F

from t2v_turbo_amd.optim import QBLOCK, dequantize_blockwise, make_code_books, quantize_blockwise
from tests.operand_form_cases import BF, BF16_TOL, F32, REPORT, STAT_TOL, Out, _CUR, bfr, close, exact, f32r, inflat, refuses, rnd

RTOL, ATOL = 1e-6, 1e-7        # fp32 rounding: the constants of tests/adamw_cases.py and tests/optim8_util.py
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1025)


# ------------------------------------------------------------------------------------------------------------------ helpers
def f32(v):
    return float(np.float32(v))


def randf(n, seed, scale=1.0):
    """Seeded normal values rounded to fp32, as fp64."""
    return f32r(torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale)


def fin(data, dev, dtype=F32, off=0):
    """Input: ``data`` in a NaN-framed flat buffer, ``off`` elements past a 16-byte boundary."""
    v = inflat(data, dev, dtype, pad=16 + off)
    assert v.data_ptr() % 16 == off * v.element_size() % 16
    return v


class Flat(Out):
    """One-row ``Out``: ``n`` elements ``off`` elements past a 16-byte boundary, 16 + elements of sentinel on either side; ``init`` for an
    in / out buffer (else NaN: must be written)."""

    def __init__(self, n, dev, dtype=F32, off=0, init=None, tail=0):
        super().__init__(1, n + tail + 32 + off, [(16 + off, 16 + off + n)], dev, dtype, pre=0, post=0, init=None if init is None else [init.reshape(1, n)])
        self.v = self.views[0].reshape(-1)
        assert self.v.data_ptr() == self.views[0].data_ptr() and self.v.data_ptr() % 16 == off * self.v.element_size() % 16

    def get(self, what):
        return self.check(what)[0].reshape(-1)


class ByteOut:
    """``Out`` for code bytes: ``n`` must-write bytes (0xFF) framed by 16 bytes of 77 on either side, compared afterwards."""

    def __init__(self, n, dev):
        full = torch.full((n + 32,), 77, dtype=torch.uint8)
        full[16:16 + n] = 255
        self.snap, self.full, self.n = full.clone(), full.to(dev), n
        self.v = self.full[16:16 + n]

    def get(self, what):
        got = self.full.cpu()
        assert torch.equal(got[:16], self.snap[:16]) and torch.equal(got[16 + self.n:], self.snap[16 + self.n:]), f"{what}: wrote outside its region"
        return got[16:16 + self.n]

    def untouched(self):
        return torch.equal(self.full.cpu(), self.snap)


def allclose(name, got, ref):
    """Per element |got - ref| <= ATOL + RTOL |ref| (fp64 reference); REPORT: the largest error / allowance."""
    ratio = float(((got.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max())
    REPORT.append((_CUR[0], name, 0.0, 1.0, ratio))
    assert ratio <= 1.0, f"{name}: error {ratio:.3f} x the allowance of rtol {RTOL}, atol {ATOL}"


def as_row(t):
    return t.reshape(1, -1)


# ------------------------------------------------------------------------------------------------------------------ optimizer / EMA
def case_adamw(ops, dev, n, wd):
    lr, b1, b2, eps, step, gs = 1e-2, 0.9, 0.999, 1e-8, 4, 0.37
    p, g, m = randf(n, 1), randf(n, 2, 0.1), randf(n, 3, 0.05)
    v = f32r(randf(n, 4, 0.01).abs() + 1e-6)
    P, G, M, V = (Flat(n, dev, init=t) for t in (p, g, m, v))
    ops.adamw_step(P.v, G.v, M.v, V.v, lr, b1, b2, eps, wd, step, grad_scale=gs)
    one = np.float32(1)
    bc1 = float(one - np.power(np.float32(b1), np.float32(step)))
    bc2_sqrt = float(np.sqrt(one - np.power(np.float32(b2), np.float32(step))))
    gr = g * f32(gs)
    m_ref = f32(b1) * m + (1.0 - f32(b1)) * gr
    v_ref = f32(b2) * v + (1.0 - f32(b2)) * gr * gr
    p_ref = p * (1.0 - f32(lr) * f32(wd)) - (f32(lr) / bc1) * m_ref / (v_ref.sqrt() / bc2_sqrt + f32(eps))
    exact("grad", G.get("grad"), g.to(F32))
    for name, o, ref in (("p", P, p_ref), ("m", M, m_ref), ("v", V, v_ref)):
        allclose(name, o.get(name), ref)


def case_ema(ops, dev, n, t_off, s_off):
    rate = np.float32(0.95)
    t, s = randf(n, 1), randf(n, 2)
    T = Flat(n, dev, off=t_off, init=t)
    ops.ema_update(T.v, fin(s, dev, off=s_off), float(rate))
    got = T.get("target")
    tn, sn = t.to(F32).numpy(), s.to(F32).numpy()
    want = tn * rate + sn * (np.float32(1) - rate)   # float32 throughout: two rounded products, one rounded sum
    assert want.dtype == np.float32
    exact("target", got, torch.from_numpy(want))
    allclose("target fp64", got, t * float(rate) + s * (1.0 - float(rate)))


def case_sumsq(ops, dev, n, off):
    x = randf(n, 1, 0.05)   # (small values: one stray workspace float or sentinel would move the sum by far more than the bound)
    blocks = min((n + 255) // 256, 1024)
    x_d = fin(x, dev, off=off)
    runs = []
    for _ in range(2):
        ws, out = Flat(blocks, dev, tail=1024 - blocks), Flat(1, dev, tail=3)
        ops.sumsq(x_d, ws.v, out.v)
        ws.get("sumsq ws")          # exactly ``blocks`` floats written (all finite), the rest of the 1024 and the frame untouched
        runs.append(out.get("sumsq out"))
    ref = (x * x).sum().reshape(1, 1)
    close("sumsq", as_row(runs[0]), ref, f32r(ref), STAT_TOL)
    exact("sumsq again", runs[1], runs[0])


def case_quant8(ops, dev, n, book, off):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * torch.rand(n, generator=gen).mul(8).sub(6).exp()
    if n >= 2 * QBLOCK:
        x[QBLOCK:2 * QBLOCK] = 0.0   # an all-zero block: absmax 0, the code of 0
    code = make_code_books()[book]
    x = x if float(code[0]) < 0 else x.abs()
    nb = (n + QBLOCK - 1) // QBLOCK
    want_c, want_a = quantize_blockwise(x, code)   # CPU tensors: the definition
    assert not want_c.is_cuda
    codes, absmax = ByteOut(nb * QBLOCK, dev), Flat(nb, dev)
    code_d = fin(code, dev)
    ops.quant8(fin(x, dev, off=off), code_d, codes.v, absmax.v)
    got_c, got_a = codes.get("codes"), absmax.get("absmax")
    exact("absmax", got_a, want_a)
    d = (got_c.int() - want_c.int()).abs()
    REPORT.append((_CUR[0], "codes", 0.0, 1e-3 * n + 1, float(d.sum())))
    assert int(d.max()) <= 1 and int(d.sum()) <= 1e-3 * n + 1, f"codes: {int(d.sum())} differ, by up to {int(d.max())}"
    zero_code = int(quantize_blockwise(torch.zeros(1), code)[0][0])
    assert bool((got_c[n:] == zero_code).all()), "padding bytes of the last block must hold the code of 0"
    if n >= 2 * QBLOCK:
        assert float(got_a[1]) == 0.0 and bool((got_c[QBLOCK:2 * QBLOCK] == zero_code).all())
    out = Flat(n, dev, off=off)
    ops.dequant8(codes.v, absmax.v, code_d, out.v)
    exact("dequant", out.get("dequant"), dequantize_blockwise(got_c, got_a, code, n))


# ------------------------------------------------------------------------------------------------------------------ scheduler family
LCM = dict(sa_t=0.6, sb_t=0.8, c_skip=0.3, c_out=0.7, sa_p=0.9, sb_p=0.43589)


def case_lcm_step(ops, dev, n, eps_bf16, with_noise, sa_t=None):
    k = {a: f32(b) for a, b in LCM.items()}
    x, noise = randf(n, 1), randf(n, 3)
    eps = bfr(randf(n, 2)) if eps_bf16 else randf(n, 2)
    prev, den = Flat(n, dev, off=3), Flat(n, dev)
    x_d, e_d = fin(x, dev, off=1), fin(eps, dev, BF if eps_bf16 else F32)
    n_d = fin(noise, dev) if with_noise else None

    def call():
        ops.lcm_step(x_d, e_d, n_d, k["sa_t"] if sa_t is None else sa_t, k["sb_t"], k["c_skip"], k["c_out"], k["sa_p"], k["sb_p"], prev.v, den.v)

    if sa_t is not None:
        return refuses(ops, call, prev, den)
    call()
    x0 = (x - k["sb_t"] * eps) / k["sa_t"]
    den_ref = k["c_out"] * x0 + k["c_skip"] * x
    prev_ref = k["sa_p"] * den_ref + k["sb_p"] * noise if with_noise else den_ref
    got_p, got_d = prev.get("prev"), den.get("denoised")
    close("denoised", as_row(got_d), as_row(den_ref), f32r(as_row(den_ref)), 1e-6)
    close("prev", as_row(got_p), as_row(prev_ref), f32r(as_row(prev_ref)), 1e-6)
    if not with_noise:
        exact("prev == denoised", got_p, got_d)


def case_lincomb3(ops, dev, nb, inner, terms, refuse=None):
    n = nb * inner
    x, y, z = randf(n, 1), randf(n, 2), randf(n, 3)
    ca = [f32(0.5 + 0.03 * b) for b in range(nb)]   # a distinct triple per batch row: a wrong i / inner shows
    cb = [f32(-1.0 + 0.05 * b) for b in range(nb)] if terms >= 2 else None
    cc = [f32(0.25 - 0.02 * b) for b in range(nb)] if terms >= 3 else None
    out = Flat(n, dev, off=1)
    x_d, y_d, z_d = fin(x, dev), (fin(y, dev, off=3) if terms >= 2 else None), (fin(z, dev) if terms >= 3 else None)
    if refuse == "no cb":
        return refuses(ops, lambda: ops.lincomb3(x_d, fin(y, dev), None, ca, None, None, out.v), out)
    if refuse is not None:
        return refuses(ops, lambda: ops.lincomb3(x_d, y_d, z_d, ca, cb, cc, out.v), out)
    ops.lincomb3(x_d, y_d, z_d, ca, cb, cc, out.v)
    col = lambda c: torch.tensor(c, dtype=torch.float64)[:, None]  # noqa: E731
    ref = col(ca) * x.reshape(nb, inner)
    if terms >= 2:
        ref = ref + col(cb) * y.reshape(nb, inner)
    if terms >= 3:
        ref = ref + col(cc) * z.reshape(nb, inner)
    close("out", as_row(out.get("out")), as_row(ref), f32r(as_row(ref)), 1e-6)


def case_silu(ops, dev, n):
    x = rnd(n, seed=1, scale=3.0)
    out = Flat(n, dev, BF, off=1)
    ops.silu(fin(x, dev, BF), out.v)
    ref = F.silu(x)
    close("out", as_row(out.get("out")), as_row(ref), bfr(as_row(ref)), BF16_TOL)


def case_timestep_embedding(ops, dev, dim, guidance, out_f32):
    half = dim // 2
    i = torch.arange(half, dtype=torch.float64)
    if guidance:   # sin || cos of 1000 w, divisor half - 1
        t = torch.tensor([7.5, 12.25, 0.0], dtype=F32)
        a = t.double()[:, None] * 1000.0 * torch.exp(-i * np.log(10000.0) / (half - 1))
        ref = torch.cat([a.sin(), a.cos()], dim=1)
    else:          # cos || sin of t, divisor half
        t = torch.tensor([999, 0, 519, 1], dtype=torch.int64)
        a = t.double()[:, None] * torch.exp(-np.log(10000.0) * i / half)
        ref = torch.cat([a.cos(), a.sin()], dim=1)
    n = t.numel()
    out = Flat(n * dim, dev, F32 if out_f32 else BF)
    (ops.timestep_embedding_f32 if out_f32 else ops.timestep_embedding)(fin(t, dev, t.dtype), dim, guidance, out.views[0])
    got = out.get("embedding").double().reshape(n, dim)
    allow = (0.0 if out_f32 else 2.0 ** -9) + 4e-6 * torch.cat([a, a], dim=1).abs() + 2e-6
    ratio = float(((got - ref).abs() / allow).max())
    REPORT.append((_CUR[0], "embedding f32" if out_f32 else "embedding bf16", 0.0, 1.0, ratio))
    assert ratio <= 1.0, f"embedding: error {ratio:.3f} x the per-element allowance"


# ------------------------------------------------------------------------------------------------------------------ refusals
def refusal_cases(ops, dev):
    """-> [(name, thunk)]: ONE call each that the entry point must refuse before any launch; every buffer is large enough for the call as
    if it had been accepted, and every output must be untouched afterwards."""
    cases = []

    def adamw(bad=None, step=4):
        def thunk():
            n = 8
            bufs = [Flat(n, dev, off=1 if i == bad else 0, init=randf(n, i + 1).abs() + 0.1) for i in range(4)]
            refuses(ops, lambda: ops.adamw_step(*(b.v for b in bufs), 1e-2, 0.9, 0.999, 1e-8, 0.0, step), *bufs)
        return thunk

    for i, nm in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):
        cases.append((f"adamw_step {nm} 4 bytes off alignment", adamw(bad=i)))
    cases.append(("adamw_step step = 0", adamw(step=0)))
    cases.append(("lcm_step sa_t = 0", lambda: case_lcm_step(ops, dev, 8, False, True, sa_t=0.0)))
    cases.append(("lincomb3 nb = 65", lambda: case_lincomb3(ops, dev, 65, 2, 3, refuse="nb")))
    cases.append(("lincomb3 y without cb", lambda: case_lincomb3(ops, dev, 2, 8, 1, refuse="no cb")))
    return cases


# ------------------------------------------------------------------------------------------------------------------ the table
def _cases():
    c = []
    for n in SIZES + (3 * 1024 + 2,):     # 3 * 1024 + 2: the tail branch i < n < i + 4 in the last of four blocks
        for wd in (0.0, 0.1):
            c.append((f"adamw_step-{n}-wd{wd}", case_adamw, dict(n=n, wd=wd)))
    for n in SIZES:                       # (257 and up: a second block)
        c.append((f"ema_update-{n}-target+4", case_ema, dict(n=n, t_off=1, s_off=0)))
        c.append((f"ema_update-{n}-source+4", case_ema, dict(n=n, t_off=0, s_off=1)))
    for n in (1, 255, 257, 256 * 1024 + 77):   # the last: 1 025 blocks' worth on the 1 024-block grid-stride loop
        for off in (0, 1, 3):
            c.append((f"sumsq-{n}-off{off}", case_sumsq, dict(n=n, off=off)))
    for n in (1, 255, 256, 257, 1000, 4097):
        for book in (0, 1):
            for off in (0, 1):
                c.append((f"quant8-{n}-book{book}-off{off}", case_quant8, dict(n=n, book=book, off=off)))
    for book, off in ((0, 0), (1, 1)):
        c.append((f"quant8-{8193 * 256 + 5}-book{book}-off{off}", case_quant8, dict(n=8193 * 256 + 5, book=book, off=off)))
    for n in (1, 257, 64 * 37):
        for eps_bf16 in (False, True):
            for with_noise in (False, True):
                c.append((f"lcm_step-{n}-eps{'bf16' if eps_bf16 else 'f32'}-noise{int(with_noise)}", case_lcm_step,
                          dict(n=n, eps_bf16=eps_bf16, with_noise=with_noise)))
    for nb in (1, 2, 64):
        for inner in (1, 37):
            for terms in (1, 2, 3):
                c.append((f"lincomb3-{nb}x{inner}-terms{terms}", case_lincomb3, dict(nb=nb, inner=inner, terms=terms)))
    for n in (1, 255, 1000):
        c.append((f"silu-{n}", case_silu, dict(n=n)))
    for dim in (320, 256):
        for guidance in (False, True):
            for out_f32 in (False, True):
                c.append((f"timestep_embedding-{dim}-{'guidance' if guidance else 'time'}-{'f32' if out_f32 else 'bf16'}", case_timestep_embedding,
                          dict(dim=dim, guidance=guidance, out_f32=out_f32)))
    return c


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
REFUSAL_IDS = [n for n, _ in refusal_cases(None, None)]   # (the thunks touch ops / dev only when called)


def run(ops, dev, name, fn, kw):
    _CUR[0] = name
    fn(ops, dev, **kw)


def run_refusal(ops, dev, name):
    dict(refusal_cases(ops, dev))[name]()
