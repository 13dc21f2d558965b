"""Shared cases of the motion-prior sampler's kernels (csrc/train.hip: ``t2v_mp_guided_step``; csrc/elementwise.hip: ``t2v_video_to_u8``) for
the host-simulator and the device tests: the geometries, schedule, arena and bounds of tests/cd_head_cases.py.

Head.  Yardstick: ``motion_prior.mp_guided_step_torch`` in float64 on the same rounded inputs, and the same twin in fp32 for the allowance
of ``check_elementwise`` (the project's bound: 4 x the fp32 twin's own error, at least one fp32 ulp of max |ref|; half an ulp of the
output format on top for an output that is rounded to bf16 / fp16).  ``x``, ``x_lp``, ``pred_x0`` and the two x0 slots of ``rec`` are
checked that way; the three copied slots of ``rec`` (and the x0 slots of a cached entry) equal ``.to(torch.float16)`` bit for bit;
the score slot is zeros without a score.  Two runs give the same bits; outputs are NaN-prefilled and carved out of an ``Arena``.

uint8.  The conversion is fully defined, so equality is the bound: ``((v.float().clamp(-1, 1) + 1.0) / 2.0 * 255).to(torch.uint8)``
channels last, NaN -> 0."""
import ctypes as C
import functools

import torch

from t2v_turbo_amd import motion_prior as mp
from t2v_turbo_amd import native as nt
from tests import cd_head_cases as cc

GEOMS, DTYPES = cc.GEOMS, cc.DTYPES
STEPS = (0, 24, 49)
W = 7.5
_OUTS = ("lpr", "", "l", "p", "r", "lp", "pr", "lr")          # which of x_lp / pred_x0 / rec a case asks for
_LP = ("bf16", "fp16")
_PD = ("fp32", "bf16", "fp16")


def _head_params():
    out, k = [], 0
    for g in GEOMS:
        for i in STEPS:
            for d in DTYPES:
                for with_score in (True, False):
                    for with_x0 in (False, True):
                        out.append((g, i, d, with_score, with_x0, _OUTS[k % len(_OUTS)], _LP[k % 2], _PD[k % 3]))
                        k += 1
    return out


# (geometry, step, dtype of cond / uncond / score / given x0, with score, with given x0, outputs, x_lp dtype, pred_x0 dtype)
HEAD_PARAMS = _head_params()


def same_bits(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8).cpu(), b.contiguous().reshape(-1).view(torch.uint8).cpu())


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def _sched(ops, dev):
    acp, solver = cc.schedule()
    tabs = (acp.to(dev), solver.ddim_timesteps.to(dev), solver.ddim_alpha_cumprods_prev.float().to(dev))
    return ops.cd_sched(*tabs, None, 0, 1.0), tabs          # (index NULL: the step comes by value)


# ------------------------------------------------------------------------------------------------------------------- head
@functools.lru_cache(maxsize=None)
def head_case(geom, i, dtype, with_score, with_x0):
    shape = GEOMS[geom][0]
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(6000 + sorted(GEOMS).index(geom))
    x = torch.randn(shape, generator=g)
    cond = torch.randn(shape, generator=g).to(dt)
    uncond = (cond.float() + 0.3 * torch.randn(shape, generator=g)).to(dt)
    score = (0.2 * torch.randn(shape, generator=g)).to(dt) if with_score else None
    x0c = (2.0 * torch.randn(shape, generator=g)).to(dt) if with_x0 else None
    x0u = (x0c.float() + 0.3 * torch.randn(shape, generator=g)).to(dt) if with_x0 else None
    case = dict(x=x, cond=cond, uncond=uncond, score=score, x0c=x0c, x0u=x0u, i=i, shape=shape)
    acp, solver = cc.schedule()

    def twin(cdt):
        f = lambda t: None if t is None else t.to(cdt)   # noqa: E731
        return mp.mp_guided_step_torch(solver, acp, i, W, f(x), f(cond), f(uncond), f(score), f(x0c), f(x0u))
    case["ref64"], case["twin32"] = twin(torch.float64), twin(torch.float32)
    return case


def run_head(ops, dev, case, outs="lpr", lp_dtype=torch.bfloat16, p_dtype=torch.float32, misalign=False):
    """One t2v_mp_guided_step on a copy of the case's state -> dict(x, x_lp, pred_x0, rec), outputs in a guarded arena."""
    arena = cc.Arena(dev)
    sched, tabs = _sched(ops, dev)
    es = lambda t: t.element_size() if misalign else 0   # noqa: E731
    put = lambda t: None if t is None else arena.put(t, es(t))   # noqa: E731
    x = put(case["x"])
    cond, uncond, score, x0c, x0u = (put(case[k]) for k in ("cond", "uncond", "score", "x0c", "x0u"))
    shape = case["shape"]
    x_lp = arena.take(shape, lp_dtype, misalign=2 if misalign else 0) if "l" in outs else None
    pred = arena.take(shape, p_dtype, misalign=torch.empty((), dtype=p_dtype).element_size() if misalign else 0) if "p" in outs else None
    rec = arena.take((shape[0], 5) + tuple(shape[1:]), torch.float16, misalign=2 if misalign else 0) if "r" in outs else None
    ops.mp_guided_step(sched, case["i"], W, x, cond, uncond, x0c, x0u, score, x_lp, pred, rec)
    _sync(dev)
    arena.check()
    return {k: None if v is None else v.clone() for k, v in dict(x=x, x_lp=x_lp, pred_x0=pred, rec=rec).items()}


def check_head(case, got, tag=""):
    ref, twin = case["ref64"], case["twin32"]
    cc.check_elementwise(f"x after step {case['i']}{tag}", got["x"], ref["x"], twin["x"])
    if got["x_lp"] is not None:
        cc.check_elementwise(f"x copy{tag}", got["x_lp"], ref["x"], twin["x"])
    if got["pred_x0"] is not None:
        cc.check_elementwise(f"pred_x0{tag}", got["pred_x0"], ref["pred_x0"], twin["pred_x0"])
    rec = got["rec"]
    if rec is not None:
        rec = rec.cpu()
        for slot, key, given in ((0, "x0_cond", case["x0c"]), (1, "x0_uncond", case["x0u"])):
            if given is None:
                cc.check_elementwise(f"rec {key}{tag}", rec[:, slot], ref[key], twin[key])
            else:
                assert same_bits(rec[:, slot], given.to(torch.float16)), f"rec {key}{tag}: a cached entry is stored as given"
        assert same_bits(rec[:, 2], case["cond"].to(torch.float16)), f"rec cond_pred_noise{tag}"
        assert same_bits(rec[:, 3], case["uncond"].to(torch.float16)), f"rec uncond_pred_noise{tag}"
        want = torch.zeros(case["shape"], dtype=torch.float16) if case["score"] is None else case["score"].to(torch.float16)
        assert same_bits(rec[:, 4], want), f"rec score{tag}"


def check_head_refusals(ops, dev):
    """Every refusal path of t2v_mp_guided_step returns its code and writes nothing."""
    EINVAL, ESHAPE = -1, -2
    sched, tabs = _sched(ops, dev)
    B, per = 2, 40
    nan = float("nan")
    c = torch.randn(B, per, device=dev)
    x = torch.full((B, per), nan, device=dev)
    lp = torch.full((B, per), nan, device=dev, dtype=torch.bfloat16)
    pred = torch.full((B, per), nan, device=dev)
    rec = torch.full((B, 5, per), nan, device=dev, dtype=torch.float16)
    lib, p, S = ops.lib, (lambda t: None if t is None else t.data_ptr()), C.byref(sched)

    def step(s=S, i=1, x_=x, cond=c, uncond=c, dt_eps=nt.F32, x0c=None, x0u=None, dt_x0=-1, score=c, dt_s=nt.F32, lp_=lp, dt_lp=nt.BF16,
             pred_=pred, dt_p=nt.F32, B_=B, per_=per):
        return lib.t2v_mp_guided_step(s, i, W, p(x_), p(cond), p(uncond), dt_eps, p(x0c), p(x0u), dt_x0, p(score), dt_s, p(lp_), dt_lp,
                                      p(pred_), dt_p, p(rec), B_, per_, None)

    assert step(s=None) == EINVAL and step(B_=0) == EINVAL and step(per_=0) == EINVAL and step(per_=-5) == EINVAL
    assert step(x_=None) == EINVAL and step(cond=None) == EINVAL and step(uncond=None) == EINVAL
    assert step(x0c=c, dt_x0=nt.F32) == EINVAL and step(x0u=c, dt_x0=nt.F32) == EINVAL          # exactly one of the two
    assert step(i=-1) == EINVAL and step(i=cc.NUM_DDIM) == EINVAL
    for name in ("alphas_cumprod", "ddim_timesteps", "ddim_alpha_cumprods_prev"):
        broken = nt.CdSched.from_buffer_copy(sched)
        setattr(broken, name, None)
        assert step(s=C.byref(broken)) == EINVAL, name
    broken = nt.CdSched.from_buffer_copy(sched)
    broken.n_ddim = 0
    assert step(s=C.byref(broken)) == EINVAL
    assert step(B_=nt.CD_MAX_CLIPS + 1) == ESHAPE
    assert step(dt_eps=3) == ESHAPE and step(dt_eps=-1) == ESHAPE and step(dt_s=7) == ESHAPE and step(dt_p=3) == ESHAPE
    assert step(x0c=c, x0u=c, dt_x0=5) == ESHAPE
    assert step(dt_lp=nt.F32) == ESHAPE and step(dt_lp=9) == ESHAPE
    _sync(dev)
    for t in (x, lp, pred, rec):
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"
    x.copy_(c)
    assert sched.index is None and step() == 0 and step(score=None, dt_s=-1, lp_=None, dt_lp=-1, pred_=None, dt_p=-1) == 0
    assert step(x0c=c, x0u=c, dt_x0=nt.F32) == 0
    _sync(dev)
    assert not any(bool(torch.isnan(t).any()) for t in (x, lp, pred, rec))


# ------------------------------------------------------------------------------------------------------------------- uint8
PATTERN_SHAPE = (1, 3, 1, 131, 167)          # 65 631 elements >= 65 536, H * W = 21 877 is odd


def u8_expected(video):
    """The torch expression of the header on CPU values, channels last; NaN -> 0."""
    v = video.cpu().float()
    nan = torch.isnan(v)
    out = ((torch.where(nan, torch.full_like(v, -1.0), v).clamp(-1, 1) + 1.0) / 2.0 * 255).to(torch.uint8)
    assert not bool(out[nan].any())
    return out.permute(0, 2, 3, 4, 1).contiguous()


@functools.lru_cache(maxsize=None)
def u8_patterns(dtype):
    """Every 16-bit pattern of bf16 / fp16 once, padded with zeros, as PATTERN_SHAPE."""
    n = 1
    for d in PATTERN_SHAPE:
        n *= d
    bits = torch.zeros(n, dtype=torch.int32)
    bits[:65536] = torch.arange(65536, dtype=torch.int32)
    v = bits.to(torch.int16).view(DTYPES[dtype]).reshape(PATTERN_SHAPE)
    assert int(torch.isnan(v.float()).sum()) == {"bf16": 254, "fp16": 2046}[dtype]
    return v


@functools.lru_cache(maxsize=None)
def u8_boundaries():
    """fp32 values k / 127.5 - 1 and their two fp32 neighbours, k = 0 .. 255: where the truncation steps from k - 1 to k."""
    k = torch.arange(256, dtype=torch.float64)
    v = (k / 127.5 - 1.0).float()
    lo, hi = torch.nextafter(v, torch.full_like(v, -2.0)), torch.nextafter(v, torch.full_like(v, 2.0))
    return torch.stack([lo, v, hi]).reshape(1, 3, 1, 16, 16).contiguous()


@functools.lru_cache(maxsize=None)
def u8_batch(dtype):
    """(2,3,3,5,7): batch, frame and channel addressing at an odd H * W, values that straddle [-1, 1]."""
    g = torch.Generator().manual_seed(7000)
    return (0.8 * torch.randn((2, 3, 3, 5, 7), generator=g)).to(DTYPES[dtype])


def run_u8(ops, dev, video, misalign=False):
    """One t2v_video_to_u8 -> (B,T,H,W,3) uint8, input and output in a guarded arena (``misalign``: both bases off by one element)."""
    arena = cc.Arena(dev)
    B, _, T, H, Wd = video.shape
    v = arena.put(video, video.element_size() if misalign else 0)
    out = arena.take((B, T, H, Wd, 3), torch.uint8, fill=0x5A, misalign=1 if misalign else 0)
    ops.video_to_u8(v, out)
    _sync(dev)
    arena.check()
    return out.clone()


def check_u8(video, out, tag=""):
    want = u8_expected(video)
    bad = torch.nonzero(out.cpu().reshape(-1) != want.reshape(-1)).reshape(-1)
    assert bad.numel() == 0, (tag, int(bad.numel()), [(int(j), int(out.cpu().reshape(-1)[j]), int(want.reshape(-1)[j])) for j in bad[:5]])


def check_u8_refusals(ops, dev):
    EINVAL, ESHAPE = -1, -2
    v = torch.zeros((1, 3, 1, 2, 4), device=dev)
    out = torch.full((1, 1, 2, 4, 3), 0x5A, dtype=torch.uint8, device=dev)
    lib = ops.lib

    def call(x=v.data_ptr(), dt=nt.F32, B=1, T=1, H=2, Wd=4, o=out.data_ptr()):
        return lib.t2v_video_to_u8(x, dt, B, T, H, Wd, o, None)

    assert call(x=None) == EINVAL and call(o=None) == EINVAL
    assert call(B=0) == EINVAL and call(T=0) == EINVAL and call(H=-1) == EINVAL and call(Wd=0) == EINVAL
    assert call(dt=3) == ESHAPE and call(dt=-1) == ESHAPE and call(x=v.data_ptr() + 2) == ESHAPE
    _sync(dev)
    assert bool((out == 0x5A).all()), "a refused call wrote an output"
    assert call() == 0
    _sync(dev)
    assert bool((out == 127).all())          # ((0 + 1) * 0.5) * 255 = 127.5 -> 127
