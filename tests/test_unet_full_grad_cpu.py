"""FULL fine-tuning of the student UNet on the native gradient engine's dataflow (CPU, emulated op backend, fp32): the gradient of EVERY
parameter, d(loss)/d(latents) and d(loss)/d(emb_all) against torch autograd through the reference-shaped module — the call pattern of
train_latent_t2v_turbo_v2.py (:669 ``unet.requires_grad_(True)``, :798-816 every parameter in an optimizer group, :1262 backward).  Pins:
the token-contracted weight gradients of Linear leaves (q | k | v groups split per leaf, virtual-concat inputs split per part, GEGLU's
row permutation undone), the im2col matrices of every conv gather mode (3x3, stride 2, nearest-x2, (3,1,1), the 4-channel entry conv
and the 4-channel exit conv) and their tap-major -> parameter-layout gather, bias / GroupNorm(+SiLU) / LayerNorm affine gradients,
per-layer text K / V projections, the per-clip column sums that carry d(loss)/d(emb_all), and the in-place pack refresh after an
optimizer step (Packer.refresh) under an unchanged launch plan.  Both op backends of tests/emu_ops.py: ``EmuOps`` (the plan is the Python
closures, re-run every step) and ``ReplayOps`` (the device's protocol: launches recorded once with their operand pointers, later steps
re-issue the list).  Call patterns beyond one plan: two input signatures (the partial last batch of an epoch) with optimizer steps
between them — every plan owns its packs and is refreshed when ITS packs are behind the parameters —, eviction of a plan, and B = 2 with
two timesteps and ``motion_cond`` (per-clip column sums, per-clip text K / V weight gradients, motion_cond_proj / combine_proj)."""
import gc
import warnings
import weakref

import pytest
import torch

from oracle.synth import synth_state_dict
from t2v_turbo_amd.unet3d import UNetModel
from tests.emu_ops import EmuOps, ReplayOps
from tests.util import load, manifest, rel_l2, tiny_unet_params


def _student(fixture="unet_tiny", **cfg):
    m = UNetModel(**tiny_unet_params(**cfg))
    m.load_state_dict(synth_state_dict(manifest(fixture)), strict=True)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for p in m.parameters():   # zero-initialised output projections would make most gradients vanish
            if float(p.abs().max()) == 0:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    m.requires_grad_(True)
    m.eval()   # (dropout masks are the engine's counter-based ones in train mode: compared separately on the device with replayed masks)
    return m


BACKENDS = pytest.mark.parametrize("backend", [EmuOps, ReplayOps], ids=["closures", "replay"])


def _grads(m, route, x, ts, ctx, tc, r_out, fps=16, mc=None):
    for p in m.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    m.native_mode = route
    y = m(xg, ts, context=ctx, fps=fps, timestep_cond=tc, **({} if mc is None else {"motion_cond": mc}))
    (y * r_out).sum().backward()
    return y.detach(), xg.grad.clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}


def _compare(got, ref, tol=3e-4):
    worst = (0.0, None)
    for n, r in ref.items():
        g = got[n]
        assert (g is None) == (r is None), n
        if r is None:
            continue
        if float(r.abs().max()) == 0:
            assert float(g.abs().max()) < 1e-6, n
            continue
        e = rel_l2(g, r)
        if e > worst[0]:
            worst = (e, n)
    assert worst[0] < tol, worst


def _update(m, gen, factor=0.02):
    """The seeded optimizer-style step of this file: every parameter moves by ``factor`` of its mean magnitude."""
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn(p.shape, generator=gen) * factor * float(p.abs().mean() + 1e-3))


def test_every_parameter_gradient_matches_autograd_and_survives_an_optimizer_step():
    _single_plan_weight_update(EmuOps)


def test_single_plan_weight_update_under_the_replay_protocol():
    """The same under the device's record-once / replay-by-pointer protocol: the recorded launch list must see the re-filled packs."""
    _single_plan_weight_update(ReplayOps)


def _single_plan_weight_update(backend):
    g = load("unet_tiny")
    m = _student()
    m._native_ops_factory = backend
    x, ts, ctx, tc = g["x"], g["ts"], g["ctx"], g["tc"]
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3))
    y_ref, dx_ref, ref = _grads(m, "off", x, ts, ctx, tc, r_out)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # the route must not fall back to the torch composite (it warns when it does)
        assert m._auto_route(x.clone().requires_grad_(True), ctx, tc, None)[0] == "train_full"
        y, dx, got = _grads(m, "train", x, ts, ctx, tc, r_out)
    eng = m._engine_box.full
    assert eng is not None and eng.training_full and len(eng.plans) == 1
    assert rel_l2(y, y_ref) < 2e-5 and rel_l2(dx, dx_ref) < 3e-4
    assert all(v is not None for v in ref.values())
    _compare(got, ref)
    # an optimizer step moves every weight: the SAME plan must give the gradients of the new weights (packs re-filled in place)
    plan = next(iter(eng.plans.values()))
    _update(m, torch.Generator().manual_seed(5))
    y_ref2, dx_ref2, ref2 = _grads(m, "off", x, ts, ctx, tc, r_out)
    y2, dx2, got2 = _grads(m, "train", x, ts, ctx, tc, r_out)
    assert next(iter(eng.plans.values())) is plan and len(eng.plans) == 1
    assert rel_l2(y_ref2, y_ref) > 1e-3, "the weight update must change the output for this check to mean anything"
    assert rel_l2(y2, y_ref2) < 2e-5 and rel_l2(dx2, dx_ref2) < 3e-4
    _compare(got2, ref2)


def test_partially_frozen_network_and_auto_route():
    """requires_grad on a subset (the v2 script's temporal / other parameter groups can be trained separately): frozen parameters get no
    gradient, the others are unchanged; the auto route takes full fine-tuning only when a parameter is trainable."""
    g = load("unet_tiny")
    m = _student()
    m._native_ops_factory = EmuOps
    x, ts, ctx, tc = g["x"], g["ts"], g["ctx"], g["tc"]
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(4))
    for n, p in m.named_parameters():
        p.requires_grad_("temporal" in n or "temopral" in n or n.startswith("time_embed"))
    _, dx_ref, ref = _grads(m, "off", x, ts, ctx, tc, r_out)
    _, dx, got = _grads(m, "train", x, ts, ctx, tc, r_out)
    assert any(v is None for v in ref.values()) and any(v is not None for v in ref.values())
    assert rel_l2(dx, dx_ref) < 3e-4
    _compare(got, ref)
    m.requires_grad_(False)
    assert m._auto_route(x.clone().requires_grad_(True), ctx, tc, None)[0] == "composite"   # input gradients only: not this route


def _fixture_step(m, x, ts, ctx, tc, r_out, route, fps=16, mc=None):
    """(output, d/d latents, gradients in named_parameters order) through ``route``."""
    y, dx, grads = _grads(m, route, x, ts, ctx, tc, r_out, fps, mc)
    return y, dx, [grads[n] for n, _ in m.named_parameters()]


def check_against_reference_fixture(y, dx, grads, names, gg, out_tol, dx_tol, norm_tol, proj_tol, full_tol):
    """Compare one step with tests/golden/unet_tiny_full_grad.npz / unet_mid_full_grad.npz / unet_tiny_mg_b2_full_grad.npz (made by the
    imported reference: make_golden_full_grad.py; the mid-width fixture holds digests only, the B = 2 one also the motion projections)."""
    from tests.golden.make_golden_full_grad import KEEP_FULL, KEEP_FULL_MOTION, digests
    if "g_" + KEEP_FULL[0].replace(".", "__") not in gg:
        KEEP_FULL = ()
    elif "g_" + KEEP_FULL_MOTION[0].replace(".", "__") in gg:
        KEEP_FULL = KEEP_FULL + KEEP_FULL_MOTION
    assert [str(n) for n in gg["names"]] == names, "parameter registration order differs from the reference's"
    e_out, e_dx = rel_l2(y, gg["out"]), rel_l2(dx, gg["dx"])
    d, ref = torch.from_numpy(digests(grads)), gg["digests"]
    # A gradient the reference has as exactly zero (B = 2 fixture: to_q / to_k of the middle block's spatial self-attention, which sees ONE
    # token at 8 x 8 latents — softmax over one key has no derivative) has no relative error.  Its norm must stay below the error allowed on
    # the SMALLEST non-zero gradient of the network, and it is left out of the relative figures.
    zero = ref[:, 0] == 0
    if bool(zero.any()):
        floor = norm_tol * float(ref[~zero, 0].min())
        worst = int(torch.where(zero, d[:, 0], torch.full_like(d[:, 0], -1.0)).argmax())
        print(f"[full fine-tuning fixture] {int(zero.sum())} gradients are zero in the reference: largest norm here {float(d[worst, 0]):.3e} "
              f"(allowed {floor:.3e})", flush=True)
        assert float(d[worst, 0]) < floor, names[worst]
        keep = (~zero).nonzero().flatten().tolist()
        d, ref, names = d[keep], ref[keep], [names[i] for i in keep]
        grads = [grads[i] for i in keep]
    norm_err = (d[:, 0] - ref[:, 0]).abs() / ref[:, 0]
    proj_err = ((d[:, 1:] - ref[:, 1:]).abs() / ref[:, :1]).max(dim=1).values
    print(f"[full fine-tuning fixture] out {e_out:.3e} dx {e_dx:.3e}; per-parameter norm err max {float(norm_err.max()):.4f} median "
          f"{float(norm_err.median()):.5f}; projection err / norm max {float(proj_err.max()):.4f} median {float(proj_err.median()):.5f}", flush=True)
    assert e_out < out_tol and e_dx < dx_tol
    assert float(norm_err.max()) < norm_tol, names[int(norm_err.argmax())]
    assert float(proj_err.max()) < proj_tol[0] and float(proj_err.median()) < proj_tol[1], names[int(proj_err.argmax())]
    for n in KEEP_FULL:
        assert rel_l2(grads[names.index(n)], gg["g_" + n.replace(".", "__")]) < full_tol, n


@pytest.mark.parametrize("fixture,width", [("unet_tiny_full_grad", 64), ("unet_mid_full_grad", 128), ("unet_tiny_mg_b2_full_grad", 64)])
def test_module_autograd_reproduces_the_reference_full_gradient_fixture(fixture, width):
    """The checker of the engine tests — autograd through this repository's torch module — against the REFERENCE's own parameter
    gradients (tests/golden/unet_tiny_full_grad.npz, unet_mid_full_grad.npz: the reference at model_channels = 128, and
    unet_tiny_mg_b2_full_grad.npz: B = 2 with two timesteps, fps = 8 and motion_cond): same registration order, every gradient to fp32
    round-off."""
    from oracle.synth import manifest_of
    from tests.golden.make_golden_full_grad import SEED_R
    motion = "mg_b2" in fixture
    g, gg = load("unet_tiny_mg_b2" if motion else "unet_tiny"), load(fixture)
    m = UNetModel(**tiny_unet_params(model_channels=width, **({"motion_cond_proj_dim": 256} if motion else {})))
    m.load_state_dict(synth_state_dict(manifest_of(m)), strict=True)
    m.requires_grad_(True)
    m.eval()
    r_out = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(SEED_R))
    assert torch.equal(r_out, gg["r_out"])
    y, dx, grads = _fixture_step(m, g["x"], g["ts"], g["ctx"], g["tc"], r_out, "off", *((8, g["mc"]) if motion else ()))
    check_against_reference_fixture(y, dx, grads, [n for n, _ in m.named_parameters()], gg, 1e-5, 1e-4, 1e-4, (1e-3, 1e-4), 1e-4)


# ---------------------------------------------------------------------------------- more than one plan; B = 2 with motion_cond
OUT_TOL, DX_TOL, PAR_TOL = 2e-5, 3e-4, 3e-4


def _moved(new, olds, what):
    """Guard of the checks behind a weight update: the autograd reference itself must have moved, from its value at EVERY earlier weight
    version, by more than 10x the tolerance it is compared at — output, d/d(latents) and every conv / Linear weight gradient — so that
    a step on stale packs (whichever version they hold) cannot pass inside the tolerance."""
    (y, dx, grads), out = new, None
    for y0, dx0, grads0 in olds:
        d_out, d_dx = rel_l2(y, y0), rel_l2(dx, dx0)
        # (a gradient that is identically zero at both versions — to_q / to_k of a one-token self-attention — has nothing to be stale about)
        d_w, n_w = min((rel_l2(g, grads0[n]), n) for n, g in grads.items()
                       if g is not None and g.dim() >= 2 and (float(g.abs().max()) > 0 or float(grads0[n].abs().max()) > 0))
        print(f"[{what}] the reference moved: out {d_out:.3e} dx {d_dx:.3e}; least-moved weight gradient {d_w:.3e} ({n_w})", flush=True)
        assert d_out > 10 * OUT_TOL and d_dx > 10 * DX_TOL and d_w > 10 * PAR_TOL, (what, d_out, d_dx, d_w, n_w)


def _step_and_check(m, sig, history, what, updated):
    """One step through the native route against autograd ("off") at the CURRENT weights; ``history``: the references of this signature
    at earlier weight versions."""
    args, kw = sig
    ref = _grads(m, "off", *args, **kw)
    if updated:
        _moved(ref, history, what)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y, dx, got = _grads(m, "train", *args, **kw)
    e_out, e_dx = rel_l2(y, ref[0]), rel_l2(dx, ref[1])
    print(f"[{what}] out {e_out:.3e} dx {e_dx:.3e}", flush=True)
    assert e_out < OUT_TOL and e_dx < DX_TOL, (what, e_out, e_dx)
    assert all(v is not None for v in ref[2].values())
    _compare(got, ref[2], PAR_TOL)
    history.append(ref)


def _two_signatures():
    """A: the unet_tiny inputs (1, 4, 4, 16, 16); B: the same latent cropped to 2 frames of 8 x 8 — another key of ``forward_tape``, with
    another frame count and another grid (what the engine keeps per recording: F, the pool, the tape)."""
    g = load("unet_tiny")
    xa = g["x"]
    xb = xa[:, :, :2, :8, :8].contiguous()
    ra = torch.randn(xa.shape, generator=torch.Generator().manual_seed(3))
    rb = torch.randn(xb.shape, generator=torch.Generator().manual_seed(4))
    return ((xa, g["ts"], g["ctx"], g["tc"], ra), {}), ((xb, g["ts"], g["ctx"], g["tc"], rb), {})


def _plan_of(eng, x):
    hit = [p for k, p in eng.plans.items() if k[2] == tuple(x.shape)]
    assert len(hit) == 1, [k[2] for k in eng.plans]
    return hit[0]


def _live_packer_is_the_last_plans(eng):
    """What the engine works on belongs to the plan it ran last: pool, Packer and kept tensors (``plan["owned"]``).  The engine keeps no
    refresh state of its own: the weight fingerprint and the captured refresh live in the plan (and go with it), and a captured refresh
    names the Packer it writes into.  (That the packs hold the current weights is what the comparisons with autograd show.)"""
    last = eng._last
    assert eng.pool is last["owned"][0] and eng.pk is last["owned"][1] and eng.keep is last["owned"][2] and eng.plan is last
    assert all("full_fp" in plan for plan in eng.plans.values())
    assert "_full_fp" not in vars(eng) and "_refresh_state" not in vars(eng)
    for plan in eng.plans.values():
        assert plan.get("refresh") is None or plan["refresh"]["sig"][0] == id(plan["owned"][1])
    assert eng._refresh_state is last.get("refresh")


@BACKENDS
def test_two_input_signatures_with_weight_updates_between(backend):
    """The data loader keeps the partial last batch: a second input signature shows up at the end of every epoch, with optimizer steps
    between the visits of either one.  Each recorded plan owns its Packer; going back to a plan must first bring ITS packs to the
    current weights (and, for the closure backend, put the engine back on that plan's pool).  Before the fix: under the replay protocol
    the earlier plan ran on the bf16 / transposed packs of the OLD weights next to live fp32 affines (a wrong gradient, silently); the
    closure backend raised in ``_conditioning``."""
    m = _student()
    m._native_ops_factory = backend
    A, B = _two_signatures()
    hist = {"A": [], "B": []}
    gen = torch.Generator().manual_seed(5)
    _step_and_check(m, A, hist["A"], "A, v0", False)
    eng = m._engine_box.full
    plan_a = _plan_of(eng, A[0][0])
    _step_and_check(m, B, hist["B"], "B, v0", False)
    plan_b = _plan_of(eng, B[0][0])
    assert len(eng.plans) == 2 and plan_a is not plan_b and plan_a["owned"][1] is not plan_b["owned"][1]
    _live_packer_is_the_last_plans(eng)
    version, sigs = 0, {"A": A, "B": B}
    for order in ("AB", "BA"):
        _update(m, gen)
        version += 1
        for name in order:
            _step_and_check(m, sigs[name], hist[name], f"{name}, v{version}", True)
            # the plans are re-used, never re-recorded: each one's packs were re-filled in place
            assert len(eng.plans) == 2 and _plan_of(eng, A[0][0]) is plan_a and _plan_of(eng, B[0][0]) is plan_b
            assert eng._last is (plan_a if name == "A" else plan_b)
            _live_packer_is_the_last_plans(eng)


@BACKENDS
def test_every_parameter_gradient_batch2_motion_cond(backend):
    """B = 2 with two different timesteps, fps = 8 and ``motion_cond`` (train_latent_t2v_turbo_v2.py --train_batch_size > 1
    --use_motion_cond): the per-clip column sums behind d(loss)/d(emb_all) (sum_rows = F h w, one row per clip), the per-clip text K / V
    weight gradients, and motion_cond_proj / combine_proj, which torch differentiates behind ``emb_all``.  Then one weight update and a
    second step on the same plan."""
    g = load("unet_tiny_mg_b2")
    m = _student("unet_tiny_mg_b2", motion_cond_proj_dim=256)
    m._native_ops_factory = backend
    assert g["x"].shape[0] == 2 and int(g["ts"][0]) != int(g["ts"][1])
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(6))
    sig = ((g["x"], g["ts"], g["ctx"], g["tc"], r_out), dict(fps=8, mc=g["mc"]))
    assert m._auto_route(g["x"].clone().requires_grad_(True), g["ctx"], g["tc"], None)[0] == "train_full"
    hist = []
    _step_and_check(m, sig, hist, "B = 2 motion_cond, v0", False)
    names = [n for n, _ in m.named_parameters()]
    assert {"motion_cond_proj.weight", "combine_proj.weight"} <= set(names)
    assert all(float(hist[0][2][n].abs().max()) > 0 for n in ("motion_cond_proj.weight", "combine_proj.weight", "time_cond_proj.weight"))
    eng = m._engine_box.full
    plan = next(iter(eng.plans.values()))
    _update(m, torch.Generator().manual_seed(5))
    _step_and_check(m, sig, hist, "B = 2 motion_cond, v1", True)
    assert len(eng.plans) == 1 and next(iter(eng.plans.values())) is plan
    _live_packer_is_the_last_plans(eng)


@BACKENDS
def test_an_evicted_plan_is_recorded_again_and_leaves_nothing_behind(backend, monkeypatch):
    """``max_plans`` = 1: recording B evicts A; after a weight update A is recorded again, on packs of the current weights.  The engine
    keeps neither the Packer nor any refresh state of a plan that is gone."""
    m = _student()
    m._native_ops_factory = backend
    A, B = _two_signatures()
    hist = {"A": [], "B": []}
    _step_and_check(m, A, hist["A"], "A, v0", False)
    eng = m._engine_box.full
    monkeypatch.setattr(eng, "max_plans", 1)
    gone = [weakref.ref(eng._last["owned"][0]), weakref.ref(eng._last["owned"][1])]   # (pool and Packer: the plan itself is a dict)
    _step_and_check(m, B, hist["B"], "B, v0", False)
    assert len(eng.plans) == 1 and eng._last is _plan_of(eng, B[0][0])
    _live_packer_is_the_last_plans(eng)
    gone += [weakref.ref(eng._last["owned"][0]), weakref.ref(eng._last["owned"][1])]
    _update(m, torch.Generator().manual_seed(5))
    _step_and_check(m, A, hist["A"], "A again, v1", True)
    assert len(eng.plans) == 1 and eng._last is _plan_of(eng, A[0][0])
    _live_packer_is_the_last_plans(eng)
    for p in m.parameters():
        p.grad = None
    gc.collect()
    assert [r() for r in gone] == [None] * 4, "an evicted plan (or its Packer) is still referenced"
