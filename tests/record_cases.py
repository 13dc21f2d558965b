"""Shared cases of the record-producer kernels (csrc/train.hip: ``t2v_cd_add_noise``, ``t2v_ddim_reverse_step``, ``t2v_pack_f16_multi``)
for the host-simulator and the device tests: the geometries, schedule and bounds of tests/cd_head_cases.py.

Yardsticks: ``preprocess.add_noise_torch`` / ``preprocess.ddim_reverse_step_torch`` in float64 on the same rounded inputs (and the same
twins in fp32 for the allowance of ``check_elementwise``); for the pack ``src.cpu().to(torch.float16)``, bit for bit — the conversion is
fully defined, so equality is the bound.  A state the kernel must not touch (a finished clip, ``prev`` of a clip whose turn it is not)
is compared bit for bit with what was there.  Two runs give the same bits; outputs are NaN-prefilled and carved out of an ``Arena``."""
import ctypes as C
import functools

import torch

from t2v_turbo_amd import native as nt
from t2v_turbo_amd import preprocess as pp
from tests import cd_head_cases as cc

GEOMS, DTYPES = cc.GEOMS, cc.DTYPES
STEP_RATIO = 20          # 1000 // 50: at i = 0 (t = 19) the previous timestep clamps to 0

ADD_NOISE_PARAMS = [(g, d, lp) for g in GEOMS for d in DTYPES for lp in ("bf16", "fp16")]
# (geometry, step i): with index [7] / [0, 24, 49] / [24, 25] — i < idx, i == idx, i > idx, idx == 0, and i = 0 where t_p clamps
REVERSE_STEPS = [("tail", 3), ("tail", 7), ("tail", 8), ("misaligned", 0), ("misaligned", 24), ("misaligned", 49), ("workgroups", 24),
                 ("workgroups", 25)]
REVERSE_PARAMS = [(g, i, e, p) for g, i in REVERSE_STEPS for e in ("bf16", "fp32") for p in (True, False)]


def same_bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8).cpu(), b.contiguous().reshape(-1).view(torch.uint8).cpu())


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def _sched(ops, dev, index):
    acp, solver = cc.schedule()
    tabs = (acp.to(dev), solver.ddim_timesteps.to(dev), solver.ddim_alpha_cumprods_prev.float().to(dev), index.to(dev))
    return ops.cd_sched(*tabs, 0, 1.0), tabs


# ------------------------------------------------------------------------------------------------------------------- add_noise
@functools.lru_cache(maxsize=None)
def add_noise_case(geom, in_dtype):
    shape, index, _ = GEOMS[geom]
    g = torch.Generator().manual_seed(3000 + sorted(GEOMS).index(geom))
    x = torch.randn(shape, generator=g).to(DTYPES[in_dtype])
    noise = torch.randn(shape, generator=g).to(torch.float32 if in_dtype == "fp32" else DTYPES[in_dtype])
    case = dict(x=x, noise=noise, index=torch.tensor(index), shape=shape)
    acp, solver = cc.schedule()
    case["ref64"] = pp.add_noise_torch(solver, acp, case["index"], x.double(), noise.double())
    case["twin32"] = pp.add_noise_torch(solver, acp, case["index"], x.float(), noise.float())
    return case


def run_add_noise(ops, dev, case, lp_dtype, misalign=False, noise=None):
    """One t2v_cd_add_noise -> (z fp32, z_lp), outputs in a guarded arena."""
    arena = cc.Arena(dev)
    sched, tabs = _sched(ops, dev, case["index"])
    noise = case["noise"] if noise is None else noise
    x = arena.put(case["x"], case["x"].element_size() if misalign else 0)
    nz = arena.put(noise, noise.element_size() if misalign else 0)
    z = arena.take(case["shape"], torch.float32, misalign=4 if misalign else 0)
    z_lp = None if lp_dtype is None else arena.take(case["shape"], lp_dtype, misalign=2 if misalign else 0)
    ops.cd_add_noise(sched, x, nz, z, z_lp)
    _sync(dev)
    arena.check()
    return z.clone(), None if z_lp is None else z_lp.clone()


def check_add_noise(case, z, z_lp, tag=""):
    cc.check_elementwise(f"z_t{tag}", z, case["ref64"], case["twin32"])
    if z_lp is not None:
        cc.check_elementwise(f"z_t copy{tag}", z_lp, case["ref64"], case["twin32"])


# ------------------------------------------------------------------------------------------------------------------- reverse step
@functools.lru_cache(maxsize=None)
def reverse_case(geom, i, eps_dtype, index=None, step_ratio=STEP_RATIO):
    shape, gindex, _ = GEOMS[geom]
    g = torch.Generator().manual_seed(4000 + sorted(GEOMS).index(geom))
    x = torch.randn(shape, generator=g)
    eps = torch.randn(shape, generator=g).to(DTYPES[eps_dtype])
    case = dict(x=x, eps=eps, index=torch.tensor(gindex if index is None else list(index)), shape=shape, i=i, step_ratio=step_ratio)
    acp, solver = cc.schedule()
    for name, cdt in (("ref64", torch.float64), ("twin32", torch.float32)):
        case[name], _ = pp.ddim_reverse_step_torch(solver, acp, case["index"], i, x.to(cdt), eps.to(cdt), None, step_ratio)
    return case


def run_reverse(ops, dev, case, with_prev, lp_dtype=torch.bfloat16, misalign=False):
    """One t2v_ddim_reverse_step on a copy of the case's state -> (x, prev, x_lp)."""
    arena = cc.Arena(dev)
    sched, tabs = _sched(ops, dev, case["index"])
    x = arena.put(case["x"], 4 if misalign else 0)
    eps = arena.put(case["eps"], case["eps"].element_size() if misalign else 0)
    prev = arena.take(case["shape"], torch.float32, misalign=4 if misalign else 0) if with_prev else None
    x_lp = None if lp_dtype is None else arena.take(case["shape"], lp_dtype, misalign=2 if misalign else 0)
    ops.ddim_reverse_step(sched, case["i"], case["step_ratio"], x, eps, prev, x_lp)
    _sync(dev)
    arena.check()
    return x.clone(), None if prev is None else prev.clone(), None if x_lp is None else x_lp.clone()


def check_reverse(case, x, prev, x_lp, tag=""):
    i, n_ddim = case["i"], cc.NUM_DDIM
    idx = case["index"].clamp(0, n_ddim - 1)
    cc.check_elementwise(f"x after step {i}{tag}", x, case["ref64"], case["twin32"])
    if x_lp is not None:
        cc.check_elementwise(f"x copy after step {i}{tag}", x_lp, case["ref64"], case["twin32"])
    for b in range(case["shape"][0]):
        if i > int(idx[b]):
            assert same_bits(x[b], case["x"][b]), f"clip {b} is finished at step {i}: its state must not move"
        if prev is not None:
            if i == int(idx[b]):
                assert same_bits(prev[b], case["x"][b]), f"clip {b}: prev is the state before step {i}"
            else:
                assert bool(torch.isnan(prev[b]).all()), f"clip {b}: prev written at step {i} != index {int(idx[b])}"


# ------------------------------------------------------------------------------------------------------------------- pack
SPECIALS = [70000.0, -70000.0, 1e-7, 6e-8, float("nan"), -0.0, 0.0, 65520.0, -65520.0, 65504.0, 65519.996, 1.0 + 2.0 ** -11,
            1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, float("inf"),
            -float("inf"), 1e-40, 2048.0 + 1.0, 2048.0 + 3.0]
NAN_AT = 4
# seven sources of odd sizes: consecutive destination offsets are 2-byte, not 16-byte aligned; (size, dtype, source off a 16-byte boundary)
PACK_SOURCES = [(37, "fp32", False), (181, "bf16", True), (10561, "fp32", True), (29, "fp16", False), (2049, "bf16", False),
                (333, "fp32", False), (231, "bf16", True)]


@functools.lru_cache(maxsize=None)
def pack_case():
    g = torch.Generator().manual_seed(5000)
    srcs = []
    for n, dt, _ in PACK_SOURCES:
        t = torch.randn(n, generator=g) * 3.0
        k = min(n, len(SPECIALS))
        t[:k] = torch.tensor(SPECIALS[:k])
        t = t.to(DTYPES[dt])
        if dt != "fp32" and k > NAN_AT:          # the quiet NaN without a payload, by its bits (what a conversion makes of a payload is not defined)
            t.view(torch.int16)[NAN_AT] = {"bf16": 0x7FC0, "fp16": 0x7E00}[dt]
        srcs.append(t)
    return srcs


def run_pack(ops, dev, srcs=None, gap=3, first_off=1):
    """One t2v_pack_f16_multi of the seven sources, ``gap`` untouched elements between two entries -> (dst, [(off, n)])."""
    srcs = pack_case() if srcs is None else srcs
    arena = cc.Arena(dev)
    dsrcs = [arena.put(s, s.element_size() if mis else 0) for s, (_, _, mis) in zip(srcs, PACK_SOURCES)]
    spans, off = [], first_off
    for s in srcs:
        spans.append((off, s.numel()))
        off += s.numel() + gap
    dst = arena.take((off,), torch.float16)
    ops.pack_f16_multi([(s, o) for s, (o, _) in zip(dsrcs, spans)], dst)
    _sync(dev)
    arena.check()
    return dst.clone(), spans


def check_pack(dst, spans, srcs=None):
    srcs = pack_case() if srcs is None else srcs
    dst = dst.cpu()
    written = torch.zeros(dst.numel(), dtype=torch.bool)
    for s, (off, n) in zip(srcs, spans):
        want = s.cpu().to(torch.float16)
        got = dst[off:off + n]
        bad = torch.nonzero(got.view(torch.int16) != want.view(torch.int16)).reshape(-1)
        assert bad.numel() == 0, (off, n, s.dtype, [(int(j), float(s[j]), float(got[j]), float(want[j])) for j in bad[:5]])
        written[off:off + n] = True
    assert bool(torch.isnan(dst[~written]).all()), "an element between two entries was written"


def run_pack_rows(ops, dev, B=3, sizes=(37, 181, 2049), dts=("fp32", "bf16", "fp32")):
    """The clip-by-clip layout of the producer: every source is [B, n_k], row r goes to r * rec + off_k of a [B, rec + 1] buffer."""
    g = torch.Generator().manual_seed(5001)
    arena = cc.Arena(dev)
    srcs = [(torch.randn(B, n, generator=g) * 3.0).to(DTYPES[d]) for n, d in zip(sizes, dts)]
    rec = sum(sizes) + 1          # (one element per record that nobody writes)
    dst = arena.take((B, rec), torch.float16)
    entries, off = [], 0
    for s in srcs:
        entries.append((arena.put(s), off, B, rec))
        off += s.shape[1]
    ops.pack_f16_multi(entries, dst)
    _sync(dev)
    arena.check()
    want = torch.cat([s.to(torch.float16) for s in srcs], dim=1)
    assert same_bits(dst[:, :rec - 1], want) and bool(torch.isnan(dst[:, rec - 1]).all())
    return dst.clone()


# ------------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(ops, dev):
    """Every refusal path of the three entry points returns its code and writes nothing."""
    EINVAL, ESHAPE = -1, -2
    sched, tabs = _sched(ops, dev, torch.tensor([3, 4]))
    B, per = 2, 40
    x = torch.randn(B, per, device=dev)
    nan = float("nan")
    z, prev = torch.full((B, per), nan, device=dev), torch.full((B, per), nan, device=dev)
    lp = torch.full((B, per), nan, device=dev, dtype=torch.bfloat16)
    dst = torch.full((B * per,), nan, device=dev, dtype=torch.float16)
    lib, p, S = ops.lib, (lambda t: None if t is None else t.data_ptr()), C.byref(sched)

    def add_noise(s=S, x_=x, dt_x=nt.F32, dt_n=nt.F32, z_=z, lp_=lp, dt_lp=nt.BF16, B_=B, per_=per):
        return lib.t2v_cd_add_noise(s, p(x_), dt_x, p(x), dt_n, p(z_), p(lp_), dt_lp, B_, per_, None)

    def reverse(s=S, i=1, ratio=20, x_=z, eps=x, dt_eps=nt.F32, lp_=lp, dt_lp=nt.BF16, B_=B, per_=per):
        return lib.t2v_ddim_reverse_step(s, i, ratio, p(x_), p(eps), dt_eps, p(prev), p(lp_), dt_lp, B_, per_, None)

    for call in (add_noise, reverse):
        assert call(s=None) == EINVAL and call(B_=0) == EINVAL and call(per_=0) == EINVAL and call(per_=-5) == EINVAL
        assert call(B_=nt.CD_MAX_CLIPS + 1) == ESHAPE
        broken = nt.CdSched.from_buffer_copy(sched)
        broken.ddim_timesteps = None
        assert call(s=C.byref(broken)) == EINVAL
        broken = nt.CdSched.from_buffer_copy(sched)
        broken.n_ddim = 0
        assert call(s=C.byref(broken)) == EINVAL
        assert call(dt_lp=nt.F32) == ESHAPE and call(dt_lp=9) == ESHAPE
    assert add_noise(x_=None) == EINVAL and add_noise(z_=None) == EINVAL
    assert add_noise(dt_x=3) == ESHAPE and add_noise(dt_n=-1) == ESHAPE
    assert reverse(x_=None) == EINVAL and reverse(eps=None) == EINVAL
    assert reverse(i=-1) == EINVAL and reverse(i=cc.NUM_DDIM) == EINVAL and reverse(ratio=-1) == EINVAL
    assert reverse(dt_eps=nt.F16) == ESHAPE and reverse(dt_eps=5) == ESHAPE

    def pack(entries, n=None, dst_=dst, numel=None):
        arr = (nt.PackEntry * nt.PACK_MAX)()
        for d, (src, cnt, rows, off, stride, dt) in zip(arr, entries):
            d.src, d.n, d.rows, d.dst_off, d.dst_stride, d.dt = src, cnt, rows, off, stride, dt
        return lib.t2v_pack_f16_multi(C.cast(arr, C.c_void_p), len(entries) if n is None else n, p(dst_),
                                      dst.numel() if numel is None else numel, None)

    ok = (p(x), per, 1, 0, 0, nt.F32)
    assert lib.t2v_pack_f16_multi(None, 1, p(dst), dst.numel(), None) == EINVAL
    assert pack([ok], dst_=None) == EINVAL and pack([ok], n=0) == EINVAL and pack([ok], n=nt.PACK_MAX + 1) == EINVAL
    assert pack([ok], numel=0) == EINVAL
    assert pack([(None, per, 1, 0, 0, nt.F32)]) == EINVAL and pack([(p(x), 0, 1, 0, 0, nt.F32)]) == EINVAL
    assert pack([(p(x), per, 0, 0, 0, nt.F32)]) == EINVAL and pack([(p(x), per, 1, -1, 0, nt.F32)]) == EINVAL
    assert pack([(p(x), per, 1, 0, 0, 3)]) == ESHAPE and pack([(p(x) + 2, per, 1, 0, 0, nt.F32)]) == ESHAPE
    assert pack([(p(x), per, 1, dst.numel() - per + 1, 0, nt.F32)]) == ESHAPE               # one element past the end
    assert pack([(p(x), per, 2, 0, per - 1, nt.F32)]) == ESHAPE                              # rows overlap
    assert pack([(p(x), per, 2, 1, per, nt.F32)]) == ESHAPE                                  # the last row ends past the end
    assert pack([ok, (p(x), dst.numel() + 1, 1, 0, 0, nt.F32)]) == ESHAPE                    # the second entry is refused: no launch
    _sync(dev)
    for t in (z, prev, lp, dst):
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"
    assert add_noise() == 0 and add_noise(lp_=None, dt_lp=-1) == 0
    z.copy_(x)
    assert reverse() == 0 and reverse(lp_=None, dt_lp=-1) == 0
    assert pack([(p(x), per, 2, 0, per, nt.F32)]) == 0
    _sync(dev)
    assert not any(bool(torch.isnan(t).any()) for t in (z, lp, dst)) and bool(torch.isnan(prev).all())
