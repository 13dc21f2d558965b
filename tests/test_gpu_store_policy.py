"""-m gpu: what one launch stores, the next launch reads — with the output stores' cache policy (csrc/common.h, T2V_WT_MASK).

Every chain below is run three ways on the ops' stream: eagerly, as ONE captured hipGraph replayed three times with the input changed
between the replays (a line left over from the previous replay would show), and stage by stage on the torch emulation
(tests/emu_ops.py) from the device's own stage inputs.  The replay must equal the eager run BIT FOR BIT, padding included; the
emulation must agree within the tolerance tests/test_gpu_kernels.py uses for that entry point (rel-L2 4e-3 for bf16 outputs, 8e-3 for
t2v_attn_spatial whose P is rounded to bf16; column statistics against the sums of the stored outputs, rtol 1e-4 / atol 2e-3).

Shapes: the smallest that still take every switched store path — the fast staged epilogue with residual and column statistics, the
generic epilogue of a split-K reduce over fp32 partial slabs, TCONV3, GroupNorm apply from column statistics, LayerNorm, the
panel-resident Linear on one full and one partial panel (plain, in place over its residual, GEGLU), both attention kernels, one
conv_halo tile row with statistics.  Every 2-D operand is a view with a row stride larger than its width; the padding of the outputs
holds a sentinel that must come back untouched, their bodies NaN that must come back finite.

Measured on an MI355X: the six tests take 2.3 s together; rel-L2 against the emulation 1.6e-3 .. 2.0e-3 at every stage (the rounding
of the bf16 output), every replay bit-equal to its eager chain."""
import pytest
import torch

from tests.emu_ops import EmuOps
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

BF16_TOL = 4e-3
SENT = 3.0
PAD = 8


def _rt(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).bfloat16().float()


class Buf:
    """[rows, cols] view at row stride cols + PAD of one allocation; ``f32``: an fp32 tensor, else an activation (bf16 on the device)."""

    def __init__(self, rows, cols, data=None, f32=False, pad=PAD):
        self.rows, self.cols, self.f32, self.is_out = rows, cols, f32, data is None
        full = torch.full((rows, cols + pad), SENT if data is None else float("nan"))
        full[:, :cols] = float("nan") if data is None else data
        self.init = full
        self.dev = full.cuda().to(torch.float32 if f32 else torch.bfloat16)

    def reset(self, data=None):
        if data is not None:
            self.init[:, :self.cols] = data
        self.dev.copy_(self.init)

    def view(self, full=None):
        return (self.dev if full is None else full)[:, :self.cols]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Chain:
    """bufs: name -> Buf; flat: name -> contiguous fp32 / pack tensors on the device; stages: (name, fn(ops, T), [(output, tolerance)]);
    inputs(r): name -> data of replay r."""

    def __init__(self, bufs, flat, stages, inputs, restore=()):
        self.bufs, self.flat, self.stages, self.inputs, self.restore = bufs, flat, stages, inputs, restore

    def tensors(self, fulls=None, cpu=False):
        T = {n: b.view(None if fulls is None else fulls[n]) for n, b in self.bufs.items()}
        T.update({n: (t.float().cpu() if cpu else t) for n, t in self.flat.items()})
        return T

    def prepare(self, r):
        data = self.inputs(r)
        for n, b in self.bufs.items():
            if b.is_out or n in data or n in self.restore:
                b.reset(data.get(n))

    def issue(self, ops):
        T = self.tensors()
        for _, fn, _ in self.stages:
            fn(ops, T)

    def snapshot(self):
        torch.cuda.synchronize()
        return {n: b.dev.clone() for n, b in self.bufs.items()}

    def eager_against_emulation(self, hip, emu):
        for name, fn, outs in self.stages:
            pre = self.snapshot()
            fn(hip, self.tensors())
            torch.cuda.synchronize()
            Te = self.tensors({n: t.float().cpu() for n, t in pre.items()}, cpu=True)
            fn(emu, Te)
            for out, tol in outs:
                got = self.bufs[out].view().float().cpu()
                assert torch.isfinite(got).all(), f"{name}: {out} left unwritten / non-finite"
                if tol == "colstat":   # of the bf16 values the kernel itself stored (tests/test_gpu_kernels.py::_halo_case)
                    src, M, N = outs[0][0], self.bufs[outs[0][0]].rows, self.bufs[outs[0][0]].cols
                    y = self.bufs[src].view().float().cpu().reshape(M // 32, 32, N)
                    want = torch.stack([y.sum(dim=1), (y * y).sum(dim=1)], dim=2).reshape(1, -1)
                    assert torch.allclose(got, want, rtol=1e-4, atol=2e-3), (name, float((got - want).abs().max()))
                else:
                    err = rel_l2(got, Te[out])
                    print(f"{name}: {out} rel-L2 vs emulation {err:.2e} (bound {tol:.0e})")
                    assert err < tol, (name, out, err)

    def check_padding(self, snap, what):
        for n, b in self.bufs.items():
            if b.is_out or n in self.restore:
                pad = snap[n][:, b.cols:].float()
                assert bool((pad == SENT).all()), f"{what}: padding of {n} overwritten"


def _run(hip, emu, chain):
    chain.prepare(0)
    chain.eager_against_emulation(hip, emu)     # (also the warm-up every capture needs: lazily allocated workspaces exist now)
    chain.check_padding(chain.snapshot(), "eager")
    g = torch.cuda.CUDAGraph()
    chain.prepare(0)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        chain.issue(hip)
    for r in range(3):
        chain.prepare(r)
        chain.issue(hip)
        eager = chain.snapshot()
        chain.prepare(r)
        g.replay()
        replay = chain.snapshot()
        chain.check_padding(replay, f"replay {r}")
        for n in chain.bufs:
            assert torch.equal(_bits(eager[n]), _bits(replay[n])), f"replay {r}: {n} differs from the eager chain"
        if r:
            chain.prepare(r)
            chain.eager_against_emulation(hip, emu)


@pytest.fixture(scope="module")
def backends():
    from t2v_turbo_amd.native import HipOps
    hip = HipOps()
    hip.init()
    return hip, EmuOps()


def _f32(t):
    return t.cuda().float().contiguous()


def test_gemm_groupnorm_tconv_chain(backends):
    """t2v_gemm (fast staged epilogue, residual, column statistics) -> t2v_group_norm_cs (SiLU) -> t2v_gemm TCONV3, frames = 2."""
    from t2v_turbo_amd import native as nt
    hip, emu = backends
    M, C = 192, 320
    bufs = {"x": Buf(M, C, _rt(M, C, seed=1)), "w1": Buf(C, C, _rt(C, C, seed=2, scale=C ** -0.5)), "res": Buf(M, C, _rt(M, C, seed=3)),
            "y1": Buf(M, C), "cs": Buf(1, M // 32 * C * 2, f32=True), "y2": Buf(M, C),
            "w2": Buf(C, 3 * C, _rt(C, 3 * C, seed=4, scale=(3 * C) ** -0.5)), "y3": Buf(M, C)}
    flat = {"b1": _f32(_rt(C, seed=5)), "gamma": _f32(_rt(C, seed=6) * 0.1 + 1.0), "beta": _f32(_rt(C, seed=7) * 0.1), "b2": _f32(_rt(C, seed=8)),
            "ws": torch.zeros(max(hip.group_norm_cs_ws_floats(1, M, 32), 8), device="cuda")}

    def s1(ops, T):
        ops.gemm(T["x"], T["w1"], T["y1"], M=M, N=C, bias=T["b1"], residual=T["res"], colstat=T["cs"].reshape(M // 32, C, 2))

    def s2(ops, T):
        ops.group_norm_cs(T["cs"].reshape(M // 32, C, 2), None, T["y1"], None, 1, M, 1e-5, T["gamma"], T["beta"], True, T["ws"], T["y2"])

    def s3(ops, T):
        ops.gemm(T["y2"], T["w2"], T["y3"], M=M, N=C, mode=nt.GEMM_TCONV3, n_img=2, h=8, wd=12, frames=2, bias=T["b2"])

    assert hip.gemm_fuse_supported(bufs["x"].view(), bufs["w1"].view(), bufs["y1"].view(), M=M, N=C, bias=flat["b1"], residual=bufs["res"].view(),
                                   colstat=bufs["cs"].view().reshape(M // 32, C, 2))
    chain = Chain(bufs, flat, [("gemm", s1, [("y1", BF16_TOL), ("cs", "colstat")]), ("group_norm_cs", s2, [("y2", BF16_TOL)]),
                               ("tconv3", s3, [("y3", BF16_TOL)])],
                  lambda r: {"x": _rt(M, C, seed=10 + r, scale=1.0 + r)})
    _run(hip, emu, chain)


def test_linear_pr_layernorm_chain(backends):
    """t2v_linear_pr over one full and one partial 160-row panel with a residual -> the same in place over its residual -> t2v_layernorm
    -> t2v_linear_pr GEGLU at N = 128."""
    from t2v_turbo_amd import native as nt
    hip, emu = backends
    M, K, N = 160 + 96, 320, 320
    wts = [_rt(n, K, seed=20 + i, scale=K ** -0.5) for i, n in enumerate((N, N, 128))]
    res0 = _rt(M, N, seed=24)
    bufs = {"a": Buf(M, K, _rt(M, K, seed=25)), "res": Buf(M, N, _rt(M, N, seed=26)), "o1": Buf(M, N), "io": Buf(M, N, res0),
            "o3": Buf(M, N), "o4": Buf(M, 64)}
    for b in (bufs["io"],):   # an input that is also written: sentinel padding, as the outputs
        b.init[:, b.cols:] = SENT
    flat = {f"wp{i}": nt.pack_linear_pr(w.bfloat16()).cuda() for i, w in enumerate(wts)}
    flat.update({f"b{i}": _f32(_rt(n, seed=30 + i)) for i, n in enumerate((N, N, 128))})
    flat.update(gamma=_f32(_rt(N, seed=34) * 0.1 + 1.0), beta=_f32(_rt(N, seed=35) * 0.1))

    def s1(ops, T):
        ops.linear_pr(T["a"], T["wp0"], T["o1"], M=M, N=N, bias=T["b0"], residual=T["res"])

    def s2(ops, T):
        ops.linear_pr(T["o1"], T["wp1"], T["io"], M=M, N=N, bias=T["b1"], residual=T["io"])

    def s3(ops, T):
        ops.layernorm(T["io"], T["gamma"], T["beta"], 1e-5, T["o3"])

    def s4(ops, T):
        ops.linear_pr(T["o3"], T["wp2"], T["o4"], M=M, N=128, bias=T["b2"], act=nt.ACT_GEGLU)

    T = Chain(bufs, flat, [], None).tensors()
    assert hip.linear_pr_supported(T["a"], T["wp0"], T["o1"], M=M, N=N, bias=T["b0"], residual=T["res"]) == 1
    assert hip.linear_pr_supported(T["o1"], T["wp1"], T["io"], M=M, N=N, bias=T["b1"], residual=T["io"]) == 1
    assert hip.linear_pr_supported(T["o3"], T["wp2"], T["o4"], M=M, N=128, bias=T["b2"], act=nt.ACT_GEGLU) == 1
    chain = Chain(bufs, flat, [("linear_pr", s1, [("o1", BF16_TOL)]), ("linear_pr in place", s2, [("io", BF16_TOL)]),
                               ("layernorm", s3, [("o3", BF16_TOL)]), ("linear_pr geglu", s4, [("o4", BF16_TOL)])],
                  lambda r: {"a": _rt(M, K, seed=40 + r, scale=1.0 + 0.5 * r)}, restore=("io",))
    _run(hip, emu, chain)


def test_split_k_then_layernorm(backends):
    """A split-K t2v_gemm (fp32 partial slabs, reduce kernel) and a consumer of its output."""
    hip, emu = backends
    M, N, K = 64, 128, 2304
    bufs = {"x": Buf(M, K, _rt(M, K, seed=50)), "w": Buf(N, K, _rt(N, K, seed=51, scale=K ** -0.5)), "y": Buf(M, N), "z": Buf(M, N)}
    flat = {"b": _f32(_rt(N, seed=52)), "gamma": _f32(_rt(N, seed=53) * 0.1 + 1.0), "beta": _f32(_rt(N, seed=54) * 0.1)}
    _, splits = hip.gemm_plan(bufs["x"].view(), bufs["w"].view(), bufs["y"].view(), M=M, N=N, bias=flat["b"], split_k=4)
    assert splits == 4, f"the launch does not split K four ways: {splits}"

    def s1(ops, T):
        ops.gemm(T["x"], T["w"], T["y"], M=M, N=N, bias=T["b"], split_k=4)

    def s2(ops, T):
        ops.layernorm(T["y"], T["gamma"], T["beta"], 1e-5, T["z"])

    chain = Chain(bufs, flat, [("split-K gemm", s1, [("y", BF16_TOL)]), ("layernorm", s2, [("z", BF16_TOL)])],
                  lambda r: {"x": _rt(M, K, seed=55 + r, scale=1.0 + r)})
    _run(hip, emu, chain)


def test_attn_temporal(backends):
    hip, emu = backends
    hw, F, heads = 3, 16, 5
    M, inner = hw * F, heads * 64
    bufs = {"qkv": Buf(M, 3 * inner, _rt(M, 3 * inner, seed=60)), "o": Buf(M, inner)}

    def s1(ops, T):
        q = T["qkv"]
        ops.attn_temporal(q[:, :inner], q[:, inner:2 * inner], q[:, 2 * inner:], T["o"], 1, F, hw, heads, 0.125)

    chain = Chain(bufs, {}, [("attn_temporal", s1, [("o", BF16_TOL)])], lambda r: {"qkv": _rt(M, 3 * inner, seed=61 + r, scale=1.0 + 0.5 * r)})
    _run(hip, emu, chain)


def test_attn_spatial(backends):
    hip, emu = backends
    sq, skv, heads = 64, 77, 2
    inner, kp = heads * 64, 128
    vt = _rt(inner, kp, seed=72)
    vt[:, skv:] = 1e30   # padding keys: probability exactly 0
    bufs = {"q": Buf(sq, inner, _rt(sq, inner, seed=70)), "k": Buf(skv, inner, _rt(skv, inner, seed=71)), "o": Buf(sq, inner)}
    flat = {"vt": vt.cuda().bfloat16().contiguous()}

    def s1(ops, T):
        ops.attn_spatial(T["q"], T["k"], T["vt"], kp, T["o"], 1, sq, skv, heads, 1, 0.125)

    chain = Chain(bufs, flat, [("attn_spatial", s1, [("o", 8e-3)])], lambda r: {"q": _rt(sq, inner, seed=73 + r, scale=1.0 + 0.5 * r)})
    _run(hip, emu, chain)


def test_conv_halo(backends):
    """One t2v_conv_halo launch at a small geometry the kernel takes (one 5-row x 32-column tile row per image), residual and column
    statistics."""
    from t2v_turbo_amd import native as nt
    hip, emu = backends
    h, w, c0, N = 5, 32, 64, 80
    M = h * w
    pack = nt.pack_conv_slab(_rt(N, 9 * c0, seed=80, scale=(9 * c0) ** -0.5))
    bufs = {"x": Buf(M, c0, _rt(M, c0, seed=81)), "res": Buf(M, N, _rt(M, N, seed=82)), "y": Buf(M, N), "cs": Buf(1, M // 32 * N * 2, f32=True)}
    flat = {"wp": pack.cuda().bfloat16().contiguous(), "b": _f32(_rt(N, seed=83))}

    def kw(T):
        return dict(M=M, N=N, mode=nt.GEMM_CONV3X3, n_img=1, h=h, wd=w, bias=T["b"], residual=T["res"], colstat=T["cs"].reshape(M // 32, N, 2))

    def s1(ops, T):
        ops.conv_halo(T["x"], T["wp"], T["y"], **kw(T))

    T = Chain(bufs, flat, [], None).tensors()
    assert hip.conv_halo_supported(T["x"], T["wp"], T["y"], **kw(T)) == 1, "the halo kernel does not take the case"
    chain = Chain(bufs, flat, [("conv_halo", s1, [("y", BF16_TOL), ("cs", "colstat")])], lambda r: {"x": _rt(M, c0, seed=84 + r, scale=1.0 + r)})
    _run(hip, emu, chain)
