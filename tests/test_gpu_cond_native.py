"""The conditioning branch on the gradient engine (``T2V_NATIVE_COND=1`` / ``UNetModel.native_conditioning``) on the device.  Full
fine-tuning: the reference's own gradient fixtures (which hold every conditioning parameter's digests, ``g_motion_cond_proj__weight``
and ``g_combine_proj__weight`` in full) at the tolerances of the existing device tests, a weight update between two steps, checkpointed
blocks and hipGraph replay bit for bit, and the autograd graph behind the output.  LoRA training: the reference's LoRA-gradient fixture (all 1 150 tensors) in eval
mode, train mode with the engine's masks replayed into the torch module, hipGraph replay, the order of the gradient-exchange markers."""
import copy
import warnings

import pytest
import torch

from tests.cond_native_util import assert_engine_node_only, cond_slots_before_their_segments, lora_step_owned, run_lora_train_masks
from tests.test_gpu_train_parity import (DX_TOL, OUT_TOL, _full_step_vs_cpu_autograd, _seeded_update, run_full_fine_tuning_batch2_motion_cond)
from tests.util import load, manifest, rel_l2, tiny_unet_params

pytestmark = pytest.mark.gpu

FIXTURE_TOL = (OUT_TOL, DX_TOL, 0.10, (0.30, 0.06), 0.12)


@pytest.fixture
def cond_on(monkeypatch):
    from t2v_turbo_amd.unet3d import UNetModel
    monkeypatch.setenv("T2V_NATIVE_COND", "1")

    def gone(*a, **k):
        raise AssertionError("conditioning_emb_all was called although the engine owns the conditioning branch")
    monkeypatch.setattr(UNetModel, "conditioning_emb_all", gone)


def _tiny():
    from oracle.synth import synth_state_dict
    from t2v_turbo_amd.unet3d import UNetModel
    ref = UNetModel(**tiny_unet_params())
    ref.load_state_dict(synth_state_dict(manifest("unet_tiny")), strict=True)
    ref.requires_grad_(True)
    ref.eval()
    return ref


def test_tiny_full_fixture_and_a_weight_update_with_the_branch_on_the_engine(cond_on):
    """tests/golden/unet_tiny_full_grad.npz (all 1485 parameters), a recording pass and a replay; then every weight moves and the same plan
    must give the gradients of the new weights — the row kernels read the live parameters, there is no pack of theirs to refresh."""
    from tests.golden.make_golden_full_grad import SEED_R
    from tests.test_unet_full_grad_cpu import _fixture_step, check_against_reference_fixture
    g, gg = load("unet_tiny"), load("unet_tiny_full_grad")
    ref = _tiny()
    m = copy.deepcopy(ref).cuda()
    names = [n for n, _ in m.named_parameters()]
    r_out = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(SEED_R))
    args = tuple(t.cuda() for t in (g["x"], g["ts"], g["ctx"], g["tc"], r_out))
    for rep in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y, dx, grads = _fixture_step(m, *args, "auto")
        eng = m._engine_box.full
        assert eng.owns_conditioning(1) and len(eng.plans) == 1 and "cond" in eng._last
        check_against_reference_fixture(y.cpu(), dx.cpu(), [t.cpu() for t in grads], names, gg, *FIXTURE_TOL)
    plan = eng._last
    assert any(e[2] == "t2v_rowlin_fwd" for e in plan["rec"]) and plan["rec_bwd"][-1][2] in ("t2v_rowlin_wgrad", "t2v_rowlin_bwd_data")
    _seeded_update(ref, m, torch.Generator().manual_seed(5))
    _full_step_vs_cpu_autograd(ref, m, (g["x"], g["ts"], g["ctx"], g["tc"], r_out), {}, (gg["out"], gg["dx"]), "native conditioning, after the update")
    assert eng._last is plan and len(eng.plans) == 1


def test_batch2_motion_cond_fixture_with_the_branch_on_the_engine(cond_on):
    run_full_fine_tuning_batch2_motion_cond(torch.device("cuda", 0), None, FIXTURE_TOL)


def _step(m, g, r_out):
    for p in m.parameters():
        p.grad = None
    xg = g["x"].cuda().requires_grad_(True)
    y = m(xg, g["ts"].cuda(), context=g["ctx"].cuda(), fps=16, timestep_cond=g["tc"].cuda())
    (y * r_out).sum().backward()
    torch.cuda.synchronize()
    return y.detach().clone(), xg.grad.clone(), [p.grad.clone() for p in m.parameters()]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


def test_checkpointing_graph_replay_and_the_autograd_graph(cond_on):
    """Mode on: ``native_checkpoint = True`` gives the bits of the tape; the plan's hipGraph replay gives the bits of its eager replay; and
    behind the output there is the engine's autograd node and AccumulateGrad nodes only."""
    g = load("unet_tiny")
    r_out = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(3)).cuda()
    m = _tiny().cuda()
    first = _step(m, g, r_out)
    eng = m._engine_box.full
    assert eng.owns_conditioning(1)
    eager = _step(m, g, r_out)                       # a replay of the recorded lists
    assert _same(first, eager)
    xg = g["x"].cuda().requires_grad_(True)
    assert_engine_node_only(m(xg, g["ts"].cuda(), context=g["ctx"].cuda(), fps=16, timestep_cond=g["tc"].cuda()), "_NativeStudentFullBackward")
    eng.use_graph = True
    try:
        for rep in range(3):                         # plain replay, capture + graph replay, graph replay
            assert _same(_step(m, g, r_out), eager), rep
        assert eng._last.get("graph_rec") is not None and eng._last.get("graph_rec_bwd") is not None and "graph_failed" not in eng._last
    finally:
        eng.use_graph = False
    m.native_checkpoint = True
    assert len(eng.plans) == 0
    assert _same(_step(m, g, r_out), eager)
    assert eng.owns_conditioning(1) and "cond" in eng._last


def test_tiny_lora_gradient_fixture_in_eval_mode_with_the_branch_on_the_engine():
    """tests/golden/unet_tiny_lora_grad.npz (the REFERENCE's gradients of all 1 150 LoRA tensors, the 54 of the conditioning leaves among
    them) with no emb_all in and no torch branch behind: helpers and tolerances of
    test_tiny_student_on_device_vs_the_reference_lora_gradient_fixture.  Recording pass, replay, then hipGraph replay bit for bit."""
    from t2v_turbo_amd import lora
    from t2v_turbo_amd.engine_unet_bwd import UNetGradEngine
    from t2v_turbo_amd.native import HipOps
    from tests.golden.make_golden_lora_grad import SEED_R, digests, draw_lora
    from tests.test_gpu_train_parity import _tiny_student
    g, gg = load("unet_tiny"), load("unet_tiny_lora_grad")
    m, params = _tiny_student(64, draw_lora)
    m = m.cuda()
    params = lora.lora_parameters(m)
    assert len(params) == 2 * int(gg["n_leaves"]) == 1150
    eng = UNetGradEngine(m, HipOps())
    eng.native_conditioning = True
    eng.bind_lora(params)
    x, ts, ctx, tc = g["x"], g["ts"], g["ctx"], g["tc"]
    r_out = torch.randn(x.shape, generator=torch.Generator().manual_seed(SEED_R))
    for rep in range(2):
        y, dx, grads = lora_step_owned(eng, params, x, ts, ctx, tc, r_out, dev="cuda")
        assert eng._last.get("cond") is not None and eng.conditioning_index().numel() == 0
        e_out, e_dx = rel_l2(y, gg["out"]), rel_l2(dx, gg["dx"])
        d, ref = torch.from_numpy(digests(grads)), gg["digests"]
        norm_err = ((d[:, 0] - ref[:, 0]).abs() / ref[:, 0])
        proj_err = ((d[:, 1:] - ref[:, 1:]).abs() / ref[:, :1])
        print(f"[LoRA fixture, native conditioning, pass {rep}] out {e_out:.3e} dx {e_dx:.3e}; norm err max {float(norm_err.max()):.3f} median "
              f"{float(norm_err.median()):.4f}; projection err / norm max {float(proj_err.max()):.3f} median {float(proj_err.median()):.4f}", flush=True)
        assert e_out < OUT_TOL and e_dx < DX_TOL
        assert float(norm_err.max()) < 0.10, int(norm_err.argmax())
        assert float(proj_err.max()) < 0.30 and float(proj_err.median()) < 0.06, int(proj_err.max(dim=1).values.argmax())
        for k in ("g10", "g11", "g1148", "g1149"):
            assert rel_l2(grads[int(k[1:])], gg[k]) < 0.12, k
    eager = (y, dx, grads)
    eng.use_graph = True
    try:
        for rep in range(3):
            assert _same(lora_step_owned(eng, params, x, ts, ctx, tc, r_out, dev="cuda"), eager), rep
        assert eng._last.get("graph_rec") is not None and eng._last.get("graph_rec_bwd") is not None and "graph_failed" not in eng._last
    finally:
        eng.use_graph = False


def test_lora_train_mode_with_replayed_masks_marker_order_and_the_autograd_graph():
    """Train mode: the conditioning leaves' dropouts draw from the engine's generator and are replayed into the torch module with every
    other site's (helpers and tolerances of test_train_mode_student_on_device_with_replayed_masks); no piece of the gradient arena that
    holds a B-row slot is sent before the last B-row weight gradient; through the module route the graph is the engine's node alone."""
    from t2v_turbo_amd.native import HipOps
    eng = run_lora_train_masks("cuda", HipOps(), OUT_TOL, DX_TOL, 0.985, 0.12)
    cond_slots_before_their_segments(eng, [e[2] for e in eng._last["rec_bwd"]])
    m, g = eng.model, load("unet_tiny")
    m.native_conditioning = True
    xg = g["x"].cuda().requires_grad_(True)
    y = m(xg, g["ts"].cuda(), context=g["ctx"].cuda(), fps=16, timestep_cond=g["tc"].cuda())
    assert_engine_node_only(y, "_NativeStudentBackward")
    (y.float() ** 2).mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters() if p.requires_grad)
