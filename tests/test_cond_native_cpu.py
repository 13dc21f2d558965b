"""The conditioning branch on the gradient engine (``T2V_NATIVE_COND=1`` / ``UNetModel.native_conditioning``), CPU: the engine's dataflow
on the emulated backend (``tests/cond_native_util.CondEmuOps``: the three B-row entries written out in torch) under the record / replay
protocol, against the reference's own gradients and fp32 autograd — the existing full-fine-tuning bodies, unchanged, with the mode on —
and what the mode is for: behind the output there is the engine's autograd node and nothing of torch's."""
import pytest
import torch

from tests.cond_native_util import CondEmuOps, assert_engine_node_only, cond_slots_before_their_segments, graph_nodes, run_lora_train_masks
from tests.emu_ops import EmuOps, ReplayOps
from tests.test_gpu_train_parity import run_full_fine_tuning_batch2_motion_cond, run_full_fine_tuning_two_signatures
from tests.test_unet_full_grad_cpu import _compare, _grads, _student
from tests.util import load, rel_l2


def _replay_backend():
    return ReplayOps(CondEmuOps(strict=True))


@pytest.fixture
def cond_on(monkeypatch):
    """The mode through the environment, and the torch branch gone: a step that still asks for it fails."""
    from t2v_turbo_amd.unet3d import UNetModel
    monkeypatch.setenv("T2V_NATIVE_COND", "1")

    def gone(*a, **k):
        raise AssertionError("conditioning_emb_all was called although the engine owns the conditioning branch")
    monkeypatch.setattr(UNetModel, "conditioning_emb_all", gone)


def test_full_fine_tuning_batch2_motion_cond_with_the_branch_on_the_engine(cond_on):
    """B = 2, two timesteps, fps = 8, motion_cond, against the reference's gradients of all 1487 parameters — time_cond_proj,
    motion_cond_proj, combine_proj, time_embed, fps_embedding and every emb_layers among them — at the fp32 tolerances of
    tests/test_train_parity_cpu.py."""
    run_full_fine_tuning_batch2_motion_cond(torch.device("cpu"), _replay_backend, (2e-5, 3e-4, 3e-4, (3e-3, 3e-4), 3e-4),
                                            out_tol=2e-5, dx_tol=3e-4, cos_min=0.99999, cos_median=0.999999)


def test_full_fine_tuning_two_signatures_with_the_branch_on_the_engine(cond_on):
    run_full_fine_tuning_two_signatures(torch.device("cpu"), _replay_backend, out_tol=2e-5, dx_tol=3e-4, cos_min=0.99999, cos_median=0.999999)


def _full_step(m, g):
    xg = g["x"].clone().requires_grad_(True)
    m.native_mode = "train"
    y = m(xg, g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"])
    return xg, y


def test_full_route_graph_is_the_engine_node_and_accumulate_grad_only():
    g = load("unet_tiny")
    m = _student()
    m._native_ops_factory = _replay_backend
    m.native_conditioning = True
    xg, y = _full_step(m, g)
    assert_engine_node_only(y, "_NativeStudentFullBackward")
    # ... and with the mode off the torch branch is there (what the assertion above would see on it)
    m.native_conditioning = False
    _, y_off = _full_step(m, g)
    assert "AddmmBackward0" in graph_nodes(y_off) or "MmBackward0" in graph_nodes(y_off)


def test_full_route_step_runs_without_torch_linear(monkeypatch):
    """No ``F.linear`` anywhere in a step: forward, backward, a weight update, a replayed step — and the gradients are autograd's."""
    g = load("unet_tiny")
    m = _student()
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3))
    y_ref, dx_ref, ref = _grads(m, "off", g["x"], g["ts"], g["ctx"], g["tc"], r_out)
    m._native_ops_factory = _replay_backend
    m.native_conditioning = True

    def no_linear(*a, **k):
        raise AssertionError("torch.nn.functional.linear ran inside a native training step")
    with monkeypatch.context() as mp:
        mp.setattr(torch.nn.functional, "linear", no_linear)
        y, dx, got = _grads(m, "train", g["x"], g["ts"], g["ctx"], g["tc"], r_out)
    assert rel_l2(y, y_ref) < 2e-5 and rel_l2(dx, dx_ref) < 3e-4
    _compare(got, ref)
    eng = m._engine_box.full
    assert eng.owns_conditioning(1) and len(eng.plans) == 1 and "cond" in next(iter(eng.plans.values()))


def test_switch_is_read_when_the_engine_is_built_and_a_change_drops_the_plans(monkeypatch):
    g = load("unet_tiny")
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3))
    m = _student()
    m._native_ops_factory = CondEmuOps
    monkeypatch.setenv("T2V_NATIVE_COND", "1")      # after import, before the engine exists
    y1, dx1, g1 = _grads(m, "train", g["x"], g["ts"], g["ctx"], g["tc"], r_out)
    eng = m._engine_box.full
    assert eng.native_conditioning and len(eng.plans) == 1 and len(eng.full_params) == len(list(m.parameters()))
    m.native_conditioning = False                    # the module's switch wins over the variable; plans and the binding follow
    assert not eng.native_conditioning and len(eng.plans) == 0 and len(eng.full_params) < len(list(m.parameters()))
    y0, dx0, g0 = _grads(m, "train", g["x"], g["ts"], g["ctx"], g["tc"], r_out)
    assert rel_l2(y1, y0) < 2e-5 and rel_l2(dx1, dx0) < 3e-4
    _compare(g1, g0)
    m.native_conditioning = None
    assert eng.native_conditioning


def test_more_than_eight_clips_keep_the_torch_branch():
    """B = 9 does not raise: that plan takes emb_all from torch, and the conditioning gradients still arrive (through autograd)."""
    g = load("unet_tiny")
    m = _student()
    m._native_ops_factory = CondEmuOps
    m.native_conditioning = True
    B = 9
    x = g["x"][:, :, :2, :8, :8].repeat(B, 1, 1, 1, 1).contiguous()
    ts, ctx, tc = g["ts"].repeat(B), g["ctx"].repeat(B, 1, 1), g["tc"].repeat(B, 1)
    r_out = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    y_ref, dx_ref, ref = _grads(m, "off", x, ts, ctx, tc, r_out)
    y, dx, got = _grads(m, "train", x, ts, ctx, tc, r_out)
    eng = m._engine_box.full
    assert not eng.owns_conditioning(B) and "cond" not in next(iter(eng.plans.values()))
    assert rel_l2(y, y_ref) < 2e-5 and rel_l2(dx, dx_ref) < 3e-4
    _compare(got, ref)


def test_checkpointed_blocks_give_the_same_bits_with_the_branch_on_the_engine():
    g = load("unet_tiny")
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3))
    res = []
    for ckpt in (False, True):
        m = _student()
        m._native_ops_factory = _replay_backend
        m.native_conditioning, m.native_checkpoint = True, ckpt
        res.append(_grads(m, "train", g["x"], g["ts"], g["ctx"], g["tc"], r_out))
    (y0, dx0, g0), (y1, dx1, g1) = res
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1) and all(torch.equal(g0[n], g1[n]) for n in g0)


def test_lora_route_graph_no_torch_linear_and_every_gradient(monkeypatch):
    """LoRA training through the module route with the mode on: behind the output there is the engine's node and AccumulateGrad nodes
    only, the step runs with ``F.linear`` patched to raise, and all LoRA gradients — the 54 B-row tensors of the conditioning leaves
    among them — are autograd's.  A second step replays the recorded lists."""
    from tests.test_unet_lora_grad_cpu import _autograd, _student as lora_student
    g = load("unet_tiny")
    m, params = lora_student("unet_tiny", 64)
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3))
    y_ref, dx_ref, g_ref = _autograd(m, params, g["x"], g["ts"], g["ctx"], 16, g["tc"], None, r_out)
    m._native_ops_factory = _replay_backend
    m.native_conditioning = True
    m.native_mode = "train"

    def no_linear(*a, **k):
        raise AssertionError("torch.nn.functional.linear ran inside a native training step")
    for rep in range(2):
        for p in params:
            p.grad = None
        with monkeypatch.context() as mp:
            mp.setattr(torch.nn.functional, "linear", no_linear)
            xg = g["x"].clone().requires_grad_(True)
            y = m(xg, g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"])
            assert_engine_node_only(y, "_NativeStudentBackward")
            (y * r_out).sum().backward()
        assert rel_l2(y.detach(), y_ref) < 2e-5 and rel_l2(xg.grad, dx_ref) < 3e-4
        eng = m._engine_box.grad
        cond = {id(w) for mod in eng.cond_lora_leaves() for w in (mod.lora_up.weight, mod.lora_down.weight)}
        assert len(cond) == 54 and eng._last.get("cond") is not None and eng.conditioning_index().numel() == 0
        for p, r in zip(params, g_ref):
            assert p.grad is not None
            if float(r.abs().max()) > 0:
                assert rel_l2(p.grad, r) < 3e-4, ("conditioning" if id(p) in cond else "token-row")
    rec = eng._last["rec_bwd"]
    cond_slots_before_their_segments(eng, ["allreduce_segment" if getattr(fn, "__name__", "") == "_segment_hook" else getattr(fn, "__name__", "") for fn, a, k in rec])


def test_lora_train_mode_with_replayed_masks_and_the_branch_on_the_engine():
    run_lora_train_masks("cpu", CondEmuOps(strict=True), 2e-5, 1e-4, 0.99999, 1e-3)


def _digest(rec):
    """(entries, sha256 of the [name, argument count] list) of a recorded launch list."""
    import hashlib
    import json
    names = [(getattr(fn, "__name__", str(fn)), len(a) + len(k)) for fn, a, k in rec]
    return [len(names), hashlib.sha256(json.dumps(names).encode()).hexdigest()]


def test_mode_off_records_the_launch_lists_of_the_commit_before_the_mode_existed():
    """Default off: the recorded forward / backward lists of the tiny full and LoRA fixtures, every entry by name and argument count, are
    those of the commit before this mode existed (tests/golden/cond_native_parent_launch_lists.json: entry counts and digests recorded
    there with this very function on ``ReplayOps(EmuOps(strict=True))``)."""
    import json
    import os
    from tests.test_unet_lora_grad_cpu import _student as lora_student
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cond_native_parent_launch_lists.json")))
    g = load("unet_tiny")
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3))
    m = _student()
    m._native_ops_factory = lambda: ReplayOps(EmuOps(strict=True))      # (not CondEmuOps: a B-row op would not even exist)
    _grads(m, "train", g["x"], g["ts"], g["ctx"], g["tc"], r_out)
    plan = next(iter(m._engine_box.full.plans.values()))
    assert {"rec": _digest(plan["rec"]), "rec_bwd": _digest(plan["rec_bwd"])} == want["full"]
    m, params = lora_student("unet_tiny", 64)
    m._native_ops_factory = lambda: ReplayOps(EmuOps(strict=True))
    m.native_mode = "train"
    xg = g["x"].clone().requires_grad_(True)
    y = m(xg, g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"])
    (y * r_out).sum().backward()
    plan = next(iter(m._engine_box.grad.plans.values()))
    assert {"rec": _digest(plan["rec"]), "rec_bwd": _digest(plan["rec_bwd"])} == want["lora"]
