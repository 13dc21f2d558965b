"""Shared cases of the consistency-head kernels (csrc/train.hip: ``t2v_cd_solver_step``, ``t2v_cd_loss_fwd``, ``t2v_cd_loss_bwd``) for the
host-simulator and the device tests.

Yardstick: the ``cd_head.*_torch`` twin evaluated in float64 on the same rounded inputs (activations rounded to the case's input
dtype, the schedule tables rounded to the fp32 the kernels read).

Bounds, none taken from what the kernels give:
  * an elementwise fp32 output (x_prev in fp32, model_pred, d_noise_pred in fp32): max |kernel - ref64| <= E, where
    E = max(4 * max |twin32 - ref64|, one fp32 ulp of max |ref64|) — the same twin in fp32 computed for that case; the factor is for
    the other operation order of the fused coefficients, the floor for a case the fp32 twin happens to hit exactly;
  * an output rounded to bf16 / fp16 (x_prev, a bf16 d_noise_pred): |out - ref64| <= ulp_out(ref64) / 2 + E for every element;
  * loss: relative error <= 1e-5 (positive terms of a few fp32 roundings each; a blocked sum of at most 9 serial adds per lane,
    a log-depth tree and a double finishing stage stay far below that; the fp32 twin is at 7e-7);
  * two runs give the same bits; every output is pre-filled with NaN and carved, between guard bytes, out of one allocation."""
import functools
import math

import numpy as np
import torch

from t2v_turbo_amd import cd_head, cd_math

TOPK, SCALING, HUBER_C, NUM_DDIM, PERCENTAGE = 20, 10.0, 0.001, 50, 0.5
MIN_INDEX = cd_head.motion_min_index(PERCENTAGE, NUM_DDIM)
assert MIN_INDEX == 25

# name -> (shape [B, C, F, H, W], index per clip, use_motion_guide per clip)
GEOMS = {
    # one clip of 36 elements: a tail and no full vector in some lanes
    "tail": ((1, 4, 1, 3, 3), [7], [1]),
    # 180 elements a clip: clip 1 of a 2-byte tensor starts off a 16-byte boundary; t_e clamps to 0 at index 0, t_s = 999 at index 49
    "misaligned": ((3, 4, 3, 5, 3), [0, 24, 49], [1, 1, 0]),
    # 10 560 elements a clip: six workgroups each, the last one partial; the two sides of the motion-guidance threshold
    "workgroups": ((2, 4, 4, 20, 33), [MIN_INDEX - 1, MIN_INDEX], [1, 1]),
}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


@functools.lru_cache(maxsize=None)
def schedule():
    """(alphas_cumprod fp32 [1000], DDIMSolver on the 50-point grid): the scaled-linear schedule of the latent-diffusion models."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    acp = torch.cumprod(1.0 - betas, dim=0).float()
    return acp, cd_math.DDIMSolver(acp.numpy(), timesteps=1000, ddim_timesteps=NUM_DDIM)


def ulp(x, dtype):
    """Spacing of ``dtype`` at |x| (elementwise, float64)."""
    mant, emin = {torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    x = torch.as_tensor(x, dtype=torch.float64).abs().clamp_min(2.0 ** emin)
    return torch.exp2(torch.floor(torch.log2(x)) - mant)


def allowance(twin32, ref64):
    return max(4.0 * float((twin32.double() - ref64).abs().max()), float(ulp(ref64.abs().max(), torch.float32)))


def check_elementwise(name, out, ref64, twin32):
    """The bound of the module docstring for one output (fp32: max error; bf16 / fp16: per element with the rounding's half ulp)."""
    out = out.detach().cpu()
    assert bool(torch.isfinite(out).all()), f"{name}: an element was not written"
    E = allowance(twin32, ref64)
    err = (out.double() - ref64).abs()
    if out.dtype == torch.float32:
        print(f"{name}: max err {float(err.max()):.3e}  bound {E:.3e}  (fp32 twin {float((twin32.double() - ref64).abs().max()):.3e}, max|ref| {float(ref64.abs().max()):.3e})")
        assert float(err.max()) <= E, (name, float(err.max()), E)
    else:
        slack = err - (ulp(ref64, out.dtype) / 2 + E)
        print(f"{name} ({out.dtype}): max err {float(err.max()):.3e}, worst excess over ulp/2 + E {float(slack.max()):.3e}  (E {E:.3e})")
        assert float(slack.max()) <= 0.0, (name, float(slack.max()), E)


class Arena:
    """Outputs carved out of ONE allocation with 64 guard bytes around each; ``check`` asserts that no guard byte moved."""
    GUARD, MAGIC = 64, 0xA5

    def __init__(self, dev, nbytes=1 << 20):
        self.buf = torch.full((nbytes,), self.MAGIC, dtype=torch.uint8, device=dev)
        self.off, self.spans = self.GUARD, []

    def take(self, shape, dtype, fill=float("nan"), misalign=0):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.off = (self.off + 15) // 16 * 16 + misalign
        assert self.off + n + self.GUARD <= self.buf.numel()
        t = self.buf[self.off:self.off + n].view(dtype).view(shape)
        t.fill_(fill)
        self.spans.append((self.off, self.off + n))
        self.off += n + self.GUARD
        return t

    def put(self, src, misalign=0):
        t = self.take(tuple(src.shape), src.dtype, 0, misalign)
        t.copy_(src)
        return t

    def check(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for a, b in self.spans:
            keep[a:b] = False
        assert bool((self.buf[keep] == self.MAGIC).all()), "a write outside the outputs"


def _round(t, dtype):
    return t.to(dtype)


@functools.lru_cache(maxsize=None)
def solver_case(geom, in_dtype, with_score):
    """Seeded inputs of one solver-step case (CPU) and its float64 / fp32 twin results, computed once."""
    shape, index, umg = GEOMS[geom]
    dt = DTYPES[in_dtype]
    g = torch.Generator().manual_seed(1000 + sorted(GEOMS).index(geom))
    z = _round(torch.randn(shape, generator=g), dt)
    c = _round(torch.randn(shape, generator=g), dt)
    u = _round(c.float() + 0.3 * torch.randn(shape, generator=g), dt)
    score = _round(0.2 * torch.randn(shape, generator=g), dt) if with_score else None
    B = shape[0]
    case = dict(z=z, c=c, u=u, score=score, index=torch.tensor(index), umg=torch.tensor(umg, dtype=torch.bool),
                w=(5.0 + 10.0 * torch.rand(B, generator=g)).float(), mgs=torch.full((B,), 0.8), shape=shape)
    acp, solver = schedule()

    def twin(cdt):
        f = lambda t: None if t is None else t.to(cdt)   # noqa: E731
        return cd_head.solver_step_v2_torch(solver, acp, case["index"], f(z), f(c), f(u), f(score), case["w"], case["mgs"], case["umg"],
                                            min_index=MIN_INDEX, out_dtype=cdt)
    case["ref64"], case["twin32"] = twin(torch.float64), twin(torch.float32)
    return case


def run_solver(ops, dev, case, out_dtype, misalign=False):
    """One t2v_cd_solver_step on ``dev`` through ``ops`` -> x_prev (in an arena, checked)."""
    acp, solver = schedule()
    arena = Arena(dev)
    tabs = (acp.to(dev), solver.ddim_timesteps.to(dev), solver.ddim_alpha_cumprods_prev.float().to(dev), case["index"].to(dev))
    sched = ops.cd_sched(*tabs, 0, 1.0)
    es = case["z"].element_size() if misalign else 0
    z, c, u = (arena.put(case[k], es) for k in ("z", "c", "u"))
    score = None if case["score"] is None else arena.put(case["score"], es)
    x_prev = arena.take(case["shape"], out_dtype, misalign=torch.empty((), dtype=out_dtype).element_size() if misalign else 0)
    ops.cd_solver_step(sched, z, c, u, score, case["w"].to(dev), case["mgs"].to(dev), case["umg"].to(dev), MIN_INDEX, x_prev)
    if dev != "cpu":
        torch.cuda.synchronize()
    arena.check()
    return x_prev.clone()


def check_solver(case, x_prev, tag=""):
    check_elementwise(f"x_prev{tag}", x_prev, case["ref64"], case["twin32"])


@functools.lru_cache(maxsize=None)
def loss_case(geom, in_dtype, xp_dtype, loss_type, with_g):
    """Seeded inputs of one loss case and the twin's loss / model_pred / d_noise_pred in float64 and fp32.  noise_pred and
    target_noise_pred are bf16 when the inputs are, fp32 otherwise; x_prev is the float64 solver result rounded to ``xp_dtype``."""
    shape, index, _ = GEOMS[geom]
    dt, np_dt = DTYPES[in_dtype], (torch.bfloat16 if in_dtype == "bf16" else torch.float32)
    sc = solver_case(geom, in_dtype, True)
    g = torch.Generator().manual_seed(2000 + sorted(GEOMS).index(geom))
    case = dict(z=sc["z"], x_prev=sc["ref64"].to(DTYPES[xp_dtype]), np=torch.randn(shape, generator=g).to(np_dt),
                tnp=torch.randn(shape, generator=g).to(np_dt), index=sc["index"], shape=shape, loss_type=loss_type,
                g_loss=torch.tensor(0.5) if with_g else None,
                g_mp=(1e-4 * torch.randn(shape, generator=g)).float() if with_g else None)
    acp, solver = schedule()

    def twin(cdt):
        npd = case["np"].clone().to(cdt).requires_grad_(True)
        loss, mp = cd_head.consistency_loss_torch(solver, acp, case["index"], npd, case["tnp"].to(cdt), case["z"].to(cdt),
                                                  case["x_prev"].to(cdt), topk=TOPK, timestep_scaling=SCALING, loss_type=loss_type,
                                                  huber_c=HUBER_C)
        total = loss * (case["g_loss"].to(cdt) if with_g else 1.0)
        if with_g:
            total = total + (mp * case["g_mp"].to(cdt)).sum()
        total.backward()
        return loss.detach(), mp.detach(), npd.grad
    case["ref64"], case["twin32"] = twin(torch.float64), twin(torch.float32)
    return case


def run_loss(ops, dev, case, misalign=False):
    """t2v_cd_loss_fwd + t2v_cd_loss_bwd on ``dev`` -> (loss, model_pred, d_noise_pred), outputs in one guarded arena."""
    acp, solver = schedule()
    arena = Arena(dev)
    tabs = (acp.to(dev), solver.ddim_timesteps.to(dev), solver.ddim_alpha_cumprods_prev.float().to(dev), case["index"].to(dev))
    sched = ops.cd_sched(*tabs, TOPK, SCALING)
    mis = (lambda t: t.element_size()) if misalign else (lambda t: 0)
    np_, tnp, z, xp = (arena.put(case[k], mis(case[k])) for k in ("np", "tnp", "z", "x_prev"))
    B, shape = case["shape"][0], case["shape"]
    model_pred, u = arena.take(shape, torch.float32, misalign=4 if misalign else 0), arena.take(shape, torch.float32, misalign=4 if misalign else 0)
    ws = arena.take((ops.cd_loss_ws_floats(B, np_.numel() // B),), torch.float32)
    loss = arena.take((1,), torch.float32)
    d = arena.take(shape, np_.dtype, misalign=mis(np_))
    g_loss = None if case["g_loss"] is None else arena.put(case["g_loss"].reshape(1))
    g_mp = None if case["g_mp"] is None else arena.put(case["g_mp"], 4 if misalign else 0)
    ops.cd_loss_fwd(sched, np_, tnp, z, xp, {"huber": 0, "l2": 1}[case["loss_type"]], HUBER_C, model_pred, u, ws, loss)
    ops.cd_loss_bwd(sched, u, g_loss, g_mp, d)
    if dev != "cpu":
        torch.cuda.synchronize()
    arena.check()
    assert bool(torch.isfinite(ws).all()) and bool(torch.isfinite(u).all())
    return loss.clone(), model_pred.clone(), d.clone()


def check_loss(case, loss, model_pred, d, tag=""):
    l64, mp64, d64 = case["ref64"]
    l32, mp32, d32 = case["twin32"]
    rel = abs(float(loss) - float(l64)) / float(l64)
    print(f"loss{tag}: {float(loss):.8e} ref {float(l64):.8e} rel err {rel:.3e} (bound 1e-5; fp32 twin {abs(float(l32) - float(l64)) / float(l64):.3e})")
    assert math.isfinite(float(loss)) and rel <= 1e-5, rel
    check_elementwise(f"model_pred{tag}", model_pred, mp64, mp32)
    check_elementwise(f"d_noise_pred{tag}", d, d64, d32)


SOLVER_PARAMS = [(g, i, o, s) for g in GEOMS for i in DTYPES for o in ("bf16", "fp32") for s in (True, False)]
LOSS_PARAMS = [(g, i, x, lt, wg) for g in GEOMS for i in DTYPES for x in ("bf16", "fp32") for lt in ("huber", "l2") for wg in (False, True)]
