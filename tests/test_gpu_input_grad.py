"""The motion-prior score through the module call on the device (tiny bf16 UNet): with ``native_input_grad`` on, the reference's call
pattern (motion_prior_sample.py:40-84: frozen eval-mode network, ``latents.requires_grad_(True)``, ``attn1.attention_probs``, the torch
loss, ``autograd.grad``) lands on the data-gradient engine without the composite path's RuntimeWarning; ``get_motion_prior_score`` then
also takes the loss gradients from the fused kernel."""
import warnings

import pytest
import torch

from tests.test_gpu_engine import E2E_TOL, _unet
from tests.util import load, rel_l2, tiny_unet_params

pytestmark = pytest.mark.gpu

# rel-L2 between the score with the fused loss kernel and the score with the torch loss, measured on MI355X (this test prints it): the
# two d(probs) differ by fp32 roundings (~1e-7), which a bf16 backward can carry across a rounding boundary — at this size it does not:
# the measurement is 0.0, the two scores are equal bit for bit.  Gate: 4 x the measurement, never above the end-to-end bf16 tolerance.
FUSED_VS_TORCH_MEASURED = 0.0
FUSED_VS_TORCH_GATE = min(4 * FUSED_VS_TORCH_MEASURED, E2E_TOL)


@pytest.fixture(scope="module")
def case():
    g, gg = load("unet_tiny"), load("unet_tiny_grad")
    m = _unet(tiny_unet_params(record_attn_probs=True), "unet_tiny", torch.bfloat16)
    m.dtype = torch.bfloat16
    m.requires_grad_(False)
    ctx = {"context": g["ctx"].cuda().bfloat16(), "fps": 16, "timestep_cond": g["tc"].cuda().bfloat16()}
    return m, ctx, g["x"].cuda().bfloat16(), g["ts"].cuda(), gg["example"].cuda().bfloat16(), gg


@pytest.fixture(scope="module")
def reference_pattern(case):
    """(a): the reference's call pattern written out, with the route on."""
    from t2v_turbo_amd import motion_prior as mp
    m, ctx, x, ts, example, _ = case
    m.native_input_grad = True
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with torch.no_grad():
            _, ex = mp.get_temp_attn_prob(m, example, ts, ctx)
        lat = x.clone().requires_grad_(True)
        out, probs = mp.get_temp_attn_prob(m, lat, ts, ctx)
        assert len(probs) == 9 and all(p.grad_fn is not None and p.dtype == torch.float32 for p in probs.values())
        loss = 500.0 * mp.compute_temp_loss(probs, ex)
        (score,) = torch.autograd.grad(loss, lat)
    assert m._engine_box.input is not None and len(m._engine_box.input.plans) == 1
    return score.detach(), out.detach()


def test_reference_call_pattern_lands_on_the_engine(case, reference_pattern):
    """Against the reference's own numbers under the bounds of tests/test_gpu_engine.py for the same computation, and bit for bit
    against ``get_motion_prior_score_native`` on an engine of its own (same launch lists, same inputs)."""
    from t2v_turbo_amd import motion_prior as mp
    from t2v_turbo_amd.engine_unet_bwd import UNetGradEngine
    from t2v_turbo_amd.native import HipOps
    m, ctx, x, ts, example, gg = case
    score, out = reference_pattern
    e_out, e_score = rel_l2(out.float().cpu(), gg["out"]), rel_l2(score.float().cpu(), gg["score"])
    print(f"route on, torch loss vs the reference fixture: out {e_out:.3e}, score {e_score:.3e}")
    assert e_out < E2E_TOL and torch.isfinite(score).all() and e_score < 0.15
    eng = UNetGradEngine(m, HipOps())
    score_n, out_n = mp.get_motion_prior_score_native(eng, m, x.clone(), ts, example, ctx, ctx, 500.0)
    assert torch.equal(out, out_n)
    assert torch.equal(score, score_n.to(score.dtype)), f"rel-L2 {rel_l2(score.float(), score_n.float()):.3e}"


def test_fused_loss_path(case, reference_pattern):
    """``mp.get_motion_prior_score`` with the route on: d(loss)/d(probs) from ``t2v_rank_loss``, fed to ``autograd.grad`` as
    ``grad_outputs``.  Measured on MI355X against the torch-loss score of the same route: rel-L2 0.0 (FUSED_VS_TORCH_MEASURED), so the
    gate of 4 x the measurement asks for equal bits; against the reference fixture: out 2.18e-2, score 1.01e-1, as with the torch loss."""
    from t2v_turbo_amd import motion_prior as mp
    m, ctx, x, ts, example, gg = case
    score_a, out_a = reference_pattern
    m.native_input_grad = True
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        score, out = mp.get_motion_prior_score(m, x.clone(), ts, example, ctx, ctx, 500.0)
    out = out.detach()
    e_out, e_score = rel_l2(out.float().cpu(), gg["out"]), rel_l2(score.float().cpu(), gg["score"])
    e_ab = rel_l2(score.float(), score_a.float())
    print(f"route on, fused loss vs the reference fixture: out {e_out:.3e}, score {e_score:.3e}; vs the torch loss: {e_ab:.3e} "
          f"(gate {FUSED_VS_TORCH_GATE:.3e})")
    assert e_out < E2E_TOL and torch.isfinite(score).all() and e_score < 0.15
    assert torch.equal(out, out_a)
    assert e_ab <= FUSED_VS_TORCH_GATE


def test_default_still_warns(case):
    """With the switch off the same module call takes the torch composite path and says so."""
    from t2v_turbo_amd import unet3d
    m, ctx, x, ts, _, _ = case
    plans = len(m._engine_box.input.plans) if m._engine_box.input is not None else 0
    fwd_ids = [p["fwd_id"] for p in m._engine_box.input.plans.values()] if plans else []
    m.native_input_grad = None
    unet3d._WARNED_ATEN.clear()     # (the warning is issued once per reason and process)
    try:
        with pytest.warns(RuntimeWarning, match="input gradients only"):
            out = m(x.clone().requires_grad_(True), ts, **ctx)
    finally:
        m.native_input_grad = True
    assert out.grad_fn is not None and torch.isfinite(out).all()
    if plans:   # the engine of the route was not called
        assert [p["fwd_id"] for p in m._engine_box.input.plans.values()] == fwd_ids
