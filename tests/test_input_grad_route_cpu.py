"""The input-gradient route of ``UNetModel`` (``native_input_grad`` / ``native_mode = "input_grad"``) on CPU: the route table, and
the module call of the motion-prior score (motion_prior_sample.py:59-84: frozen eval-mode network, ``latents.requires_grad_(True)``,
``attn1.attention_probs``, ``autograd.grad``) landing on the data-gradient engine with the emulated op backend (fp32), against the
numbers the REFERENCE computed (tests/golden/unet_tiny_grad.npz) and against autograd through the torch composite path.  Bounds: those of
tests/test_unet_grad_cpu.py for the same computations (out < 2e-5, gradients < 1e-4)."""
import warnings

import pytest
import torch

from oracle.synth import synth_state_dict
from t2v_turbo_amd import motion_prior as mp
from t2v_turbo_amd.unet3d import UNetModel
from tests.emu_ops import EmuOps
from tests.util import load, manifest, rel_l2, tiny_unet_params


def _frozen(fixture="unet_tiny", **cfg):
    m = UNetModel(**tiny_unet_params(**cfg)).eval()
    m.load_state_dict(synth_state_dict(manifest(fixture)), strict=True)
    m.requires_grad_(False)
    return m


def _forced(fixture="unet_tiny", **cfg):
    m = _frozen(fixture, **cfg)
    m._native_ops_factory = lambda: EmuOps(strict=True)
    m.native_mode = "input_grad"
    return m


def _recorded(m):
    return [mod for mod in m.modules() if getattr(mod, "record_attn_probs", False)]


# ------------------------------------------------------------------------------------------------------------------ route table
def test_route_table(monkeypatch):
    monkeypatch.delenv("T2V_NATIVE_INPUT_GRAD", raising=False)
    g = load("unet_tiny")
    m = _frozen(record_attn_probs=True)
    ctx, tc = g["ctx"], g["tc"]
    x = g["x"].clone().requires_grad_(True)
    assert m.native_input_grad is None and not m.input_grad_route_on()
    assert m._auto_route(x, ctx, tc, None)[0] == "composite"                  # the default stays what it was
    monkeypatch.setenv("T2V_NATIVE_INPUT_GRAD", "1")
    assert m._auto_route(x, ctx, tc, None) == ("input_grad", None)            # None follows the variable
    m.native_input_grad = False
    assert m._auto_route(x, ctx, tc, None)[0] == "composite"                  # ... and the attribute overrides it
    monkeypatch.delenv("T2V_NATIVE_INPUT_GRAD")
    m.native_input_grad = True
    assert m._auto_route(x, ctx, tc, None) == ("input_grad", None)
    with torch.no_grad():
        assert m._auto_route(x, ctx, tc, None) == ("infer", None)
    assert m._auto_route(g["x"], ctx, tc, None) == ("infer", None)            # nothing requires grad

    def same_as_switch_off(mod, *args):
        mod.native_input_grad = True
        on = mod._auto_route(*args)
        mod.native_input_grad = False
        off = mod._auto_route(*args)
        mod.native_input_grad = True
        assert on == off and on[0] != "input_grad"
        return on

    assert same_as_switch_off(m, x, ctx.clone().requires_grad_(True), tc, None)[0] == "composite"
    assert same_as_switch_off(m, x, ctx, tc.clone().requires_grad_(True), None)[0] == "composite"
    assert same_as_switch_off(m, x, None, tc, None)[0] == "composite"
    m.train()       # a frozen network left in train mode: the TemporalConvBlock dropouts are live, the unbound engine refuses them
    route, why = same_as_switch_off(m, x, ctx, tc, None)
    assert route == "composite" and "input gradients only" in why
    m.eval()
    p = next(m.parameters())
    p.requires_grad_(True)      # one trainable parameter: full fine-tuning
    assert same_as_switch_off(m, x, ctx, tc, None) == ("train_full", None)
    p.requires_grad_(False)
    assert m._auto_route(x, ctx, tc, None) == ("input_grad", None)
    from tests.test_unet_lora_grad_cpu import _student
    lm, _ = _student("unet_tiny", 8)
    assert same_as_switch_off(lm, x, ctx, tc, None) == ("train", None)        # LoRA-injected: the LoRA training route


def test_forced_mode_raises_where_the_route_cannot_run():
    g = load("unet_tiny")
    x = g["x"].clone().requires_grad_(True)
    m = _forced()
    with pytest.raises(RuntimeError, match="latents only"):
        m(x, g["ts"], context=g["ctx"].clone().requires_grad_(True), fps=16, timestep_cond=g["tc"])
    with pytest.raises(ValueError, match="text context"):
        m(x, g["ts"], context=None, fps=16, timestep_cond=g["tc"])
    next(m.parameters()).requires_grad_(True)
    with pytest.raises(RuntimeError, match="frozen network"):
        m(x, g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"])
    m.requires_grad_(False)
    m.train()
    with pytest.raises(RuntimeError, match="Dropout"):
        m(x, g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"])
    del m._native_ops_factory
    m.eval()
    with pytest.raises(RuntimeError, match="CUDA"):
        m(x, g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"])


# ------------------------------------------------------------------------------------------------------ forced mode, emulated ops
def test_motion_prior_score_through_the_module_call_matches_the_reference_fixture():
    """``mp.get_motion_prior_score`` unchanged: its differentiated pass is the module call, which lands on the engine; the loss is
    the torch one on the graph-connected ``attention_probs``."""
    g, gg = load("unet_tiny"), load("unet_tiny_grad")
    m = _forced(record_attn_probs=True)
    ctx = {"context": g["ctx"], "fps": 16, "timestep_cond": g["tc"]}
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        score, out = mp.get_motion_prior_score(m, g["x"].clone(), g["ts"], gg["example"], ctx, ctx, 500.0)
    eng = m._engine_box.input
    assert eng is not None and not eng.trains and len(eng.plans) == 1 and m._engine_box.full is None and m._engine_box.grad is None
    e_out, e_score = rel_l2(out.detach(), gg["out"]), rel_l2(score, gg["score"])
    print(f"input-grad route vs the reference fixture: out {e_out:.2e}, score {e_score:.2e}")
    assert e_out < 2e-5 and e_score < 1e-4
    assert all(mod.attention_probs.grad_fn is not None for mod in _recorded(m)) and len(_recorded(m)) == 9


def test_loss_on_the_output_alone_and_second_backward_refused():
    g, gg = load("unet_tiny"), load("unet_tiny_grad")
    m = _forced(record_attn_probs=True)
    x = g["x"].clone().requires_grad_(True)
    y = m(x, g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"])
    assert rel_l2(y.detach(), gg["out"]) < 2e-5
    loss = (y * gg["r_out"]).sum()
    (dx,) = torch.autograd.grad(loss, x, retain_graph=True)
    assert rel_l2(dx, gg["dx_out"]) < 1e-4
    with pytest.raises(RuntimeError, match="already run"):
        torch.autograd.grad(loss, x)
    # a network that records nothing: the function has the one output
    m2 = _forced()
    x2 = g["x"].clone().requires_grad_(True)
    y2 = m2(x2, g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"])
    (dx2,) = torch.autograd.grad((y2 * gg["r_out"]).sum(), x2)
    assert not m2._engine_box.input._last["probs"] and rel_l2(dx2, gg["dx_out"]) < 1e-4


def _both_ways(m, x, ts, ctx, tc, fps, mc, r_out, r_probs):
    """d/d(latents) of sum(y * r_out) (unless r_out is None) + sum_i sum(probs_i * r_probs[i]) through the engine route and through
    the composite path."""
    res = []
    kw = {} if mc is None else {"motion_cond": mc}
    for mode in ("input_grad", "off"):
        m.native_mode = mode
        xg = x.clone().requires_grad_(True)
        y = m(xg, ts, context=ctx, fps=fps, timestep_cond=tc, **kw)
        loss = 0.0 if r_out is None else (y * r_out).sum()
        for mod, r in zip(_recorded(m), r_probs):
            if r is not None:
                loss = loss + (mod.attention_probs * r).sum()
        res.append((y.detach(), torch.autograd.grad(loss, xg)[0]))
    return res


def test_loss_on_output_and_probabilities_matches_composite_autograd():
    g = load("unet_tiny")
    m = _forced(record_attn_probs=True)
    gen = torch.Generator().manual_seed(5)
    r_out = torch.randn(g["x"].shape, generator=gen)
    with torch.no_grad():
        m.native_mode = "off"
        m(g["x"], g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"])
    # gradients enter at three of the nine recorded layers; the others get none (their dprobs arrive as None)
    r_probs = [torch.randn(mod.attention_probs.shape, generator=gen) if i % 3 == 0 else None for i, mod in enumerate(_recorded(m))]
    (y, dx), (y_ref, dx_ref) = _both_ways(m, g["x"], g["ts"], g["ctx"], g["tc"], 16, None, r_out, r_probs)
    assert rel_l2(y, y_ref) < 2e-5 and rel_l2(dx, dx_ref) < 1e-4
    # the probabilities alone (dout arrives as None)
    (_, dx), (_, dx_ref) = _both_ways(m, g["x"], g["ts"], g["ctx"], g["tc"], 16, None, None, r_probs)
    assert float(dx_ref.abs().max()) > 0 and rel_l2(dx, dx_ref) < 1e-4


def test_batch_of_two_with_motion_cond_matches_composite_autograd():
    g = load("unet_tiny_mg_b2")
    m = _forced("unet_tiny_mg_b2", motion_cond_proj_dim=256)
    r_out = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(11))
    (y, dx), (y_ref, dx_ref) = _both_ways(m, g["x"], g["ts"], g["ctx"], g["tc"], 8, g["mc"], r_out, [])
    assert rel_l2(y, g["y"]) < 2e-5 and rel_l2(y, y_ref) < 2e-5
    assert rel_l2(dx, dx_ref) < 1e-4


# ------------------------------------------------------------------------------------------------------------------- fused loss
@pytest.mark.parametrize("rank_k", [1, 3])
def test_fused_loss_on_cpu_matches_the_torch_loss_and_its_autograd(rank_k):
    from tests.rank_loss_cases import closed_form
    gen = torch.Generator().manual_seed(2)
    shapes = {"a": (37, 4, 4), "b": (130, 4, 4), "c": (8, 16, 16)}
    ex = {k: torch.softmax(2 * torch.randn(s, generator=gen), -1) for k, s in shapes.items()}
    pr = {k: torch.softmax(2 * torch.randn(s, generator=gen), -1).requires_grad_(True) for k, s in shapes.items()}
    losses = [mp.calculate_motion_rank_new(ex[k], pr[k], rank_k=rank_k) for k in pr]
    ref = 7.0 * (torch.stack(losses) * 100).mean()
    g_ref = torch.autograd.grad(ref, [pr[k] for k in pr])
    if rank_k == 1:
        assert torch.equal(ref, 7.0 * mp.compute_temp_loss(pr, ex))
    loss, grads = mp.compute_temp_loss_fused(pr, ex, rank_k=rank_k, scale=7.0)
    assert loss.dim() == 0 and abs(float(loss) - float(ref.detach())) < 1e-5 * float(ref.detach())
    for k, gr in zip(pr, g_ref):
        assert grads[k].shape == pr[k].shape and torch.equal(grads[k] != 0, gr != 0)
        assert rel_l2(grads[k], gr) < 1e-6
        # ... and the float64 closed form the kernel tests use is the same function
        sel, _, d64 = closed_form(ex[k].reshape(-1, ex[k].shape[-1]), pr[k].detach().reshape(-1, ex[k].shape[-1]), rank_k, 700.0 / 3)
        assert torch.equal(sel.reshape(gr.shape), gr != 0) and rel_l2(gr, d64.reshape(gr.shape)) < 1e-6
    with pytest.raises(ValueError):
        mp.compute_temp_loss_fused(pr, ex, rank_k=5)
