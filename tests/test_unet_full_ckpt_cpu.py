"""Activation checkpointing under FULL fine-tuning (CPU, emulated op backends, fp32): ``UNetModel.native_checkpoint`` /
``UNetGradEngine.checkpoint_blocks`` together with ``bind_full`` — the configuration of train_latent_t2v_turbo_v2.py (every UNet parameter
trainable, yaml ``use_checkpoint: true``).  Every residual block and spatial / temporal transformer keeps only its input and re-runs its
forward inside the backward; the leaf inputs the full mixin keeps for the weight gradients (``_fsaved``) follow the same protocol.  Pins:
checkpoint off against on bit for bit (output, d/d(latents), every parameter gradient; eval and train mode with the counter-based
dropout masks), a smaller activation pool and one more forward's worth of launches in the backward list, gradients against torch
autograd before and after a weight update on the same plan, two input signatures, eviction, B = 2 with ``motion_cond``, and the public
switch.  Helpers and tolerances are those of tests/test_unet_full_grad_cpu.py."""
import gc
import weakref

import pytest
import torch

from t2v_turbo_amd.engine_unet_bwd import UNetGradEngine
from tests.emu_ops import EmuOps, ReplayOps
from tests.test_unet_full_grad_cpu import (BACKENDS, _compare, _grads, _live_packer_is_the_last_plans, _plan_of, _step_and_check, _student,
                                           _two_signatures, _update)
from tests.util import load, rel_l2


def _ckpt_student(backend, fixture="unet_tiny", on=True, **cfg):
    m = _student(fixture, **cfg)
    m._native_ops_factory = backend
    m.native_checkpoint = on
    return m


def _engine(m, on=True):
    eng = m._engine_box.full
    assert eng is not None and eng.training_full and eng.checkpoint_blocks is on
    return eng


def _off_against_on(backend, train):
    g = load("unet_tiny")
    x, ts, ctx, tc = g["x"], g["ts"], g["ctx"], g["tc"]
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3))
    res = {}
    for ck in (False, True):
        m = _ckpt_student(backend, on=ck)
        if train:
            m.train()
        steps = []
        for rep in range(2):          # record, then the same plan again
            torch.manual_seed(77)     # (train mode: the forward draws its dropout seed from torch's generator)
            y, dx, got = _grads(m, "train", x, ts, ctx, tc, r_out)
            steps.append((y, dx, got))
        eng = _engine(m, ck)
        assert len(eng.plans) == 1
        plan = eng._last
        assert all(v is not None for v in steps[0][2].values())
        assert torch.equal(steps[1][0], steps[0][0]) and torch.equal(steps[1][1], steps[0][1])
        assert all(torch.equal(steps[1][2][n], v) for n, v in steps[0][2].items()), "a second step on the same plan gives other bits"
        res[ck] = dict(step=steps[0], pool=eng.pool.bytes, live=len(eng.pool.live), sites=len(eng.drop_sites),
                       n_fwd=len(plan.get("rec", ())), n_bwd=len(plan.get("rec_bwd", ())))
    a, b = res[False], res[True]
    print(f"[full fine-tuning, checkpoint, {backend.__name__}, {'train' if train else 'eval'}] activation pool {a['pool']} -> {b['pool']} bytes "
          f"({b['pool'] / a['pool']:.3f}); launches forward {a['n_fwd']} / {b['n_fwd']}, backward {a['n_bwd']} -> {b['n_bwd']}; "
          f"dropout sites {a['sites']} / {b['sites']}", flush=True)
    assert torch.equal(a["step"][0], b["step"][0]) and torch.equal(a["step"][1], b["step"][1])
    for n, v in a["step"][2].items():
        assert torch.equal(v, b["step"][2][n]), n
    assert float(a["step"][1].abs().sum()) > 0 and all(float(v.abs().sum()) > 0 for v in a["step"][2].values())
    assert a["live"] == 0 and b["live"] == 0, "buffers left in pool.live after the backward"
    assert b["pool"] < 0.6 * a["pool"], (a["pool"], b["pool"])
    if backend is ReplayOps:
        assert a["n_fwd"] == b["n_fwd"] > 0 and b["n_bwd"] > a["n_bwd"] + 0.8 * a["n_fwd"], (a["n_fwd"], b["n_fwd"], a["n_bwd"], b["n_bwd"])
    return a, b


@BACKENDS
def test_checkpointing_is_the_tape_bit_for_bit_through_the_module(backend):
    """Checkpoint off against on through ``native_mode = "train"``: same bits, a second step on the same plan the same again, nothing
    left in ``pool.live``, pool below 0.6 x the tape's, forward list unchanged and the backward list longer by most of a forward."""
    _off_against_on(backend, train=False)


@BACKENDS
def test_checkpointing_in_train_mode_recomputes_the_same_dropout_masks(backend):
    """``m.train()``: the TemporalConvBlock dropouts are live, and a recomputed block must draw the masks of its first forward (same
    site numbers under the same seed) — a wrong mask would change the gradients behind it."""
    a, b = _off_against_on(backend, train=True)
    assert a["sites"] == b["sites"] > 0


@BACKENDS
def test_checkpointed_gradients_match_autograd_and_survive_an_optimizer_step(backend):
    g = load("unet_tiny")
    m = _ckpt_student(backend)
    x, ts, ctx, tc = g["x"], g["ts"], g["ctx"], g["tc"]
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3))
    y_ref, dx_ref, ref = _grads(m, "off", x, ts, ctx, tc, r_out)
    y, dx, got = _grads(m, "train", x, ts, ctx, tc, r_out)
    eng = _engine(m)
    assert len(eng.plans) == 1
    assert rel_l2(y, y_ref) < 2e-5 and rel_l2(dx, dx_ref) < 3e-4
    assert all(v is not None for v in ref.values())
    _compare(got, ref)
    plan = next(iter(eng.plans.values()))
    _update(m, torch.Generator().manual_seed(5))
    y_ref2, dx_ref2, ref2 = _grads(m, "off", x, ts, ctx, tc, r_out)
    y2, dx2, got2 = _grads(m, "train", x, ts, ctx, tc, r_out)
    assert next(iter(eng.plans.values())) is plan and len(eng.plans) == 1
    assert rel_l2(y_ref2, y_ref) > 1e-3, "the weight update must change the output for this check to mean anything"
    assert rel_l2(y2, y_ref2) < 2e-5 and rel_l2(dx2, dx_ref2) < 3e-4
    _compare(got2, ref2)


@BACKENDS
def test_two_input_signatures_with_weight_updates_between_under_checkpointing(backend):
    """The step sequence of test_two_input_signatures_with_weight_updates_between, with every block recomputed in the backward."""
    m = _ckpt_student(backend)
    A, B = _two_signatures()
    hist = {"A": [], "B": []}
    gen = torch.Generator().manual_seed(5)
    _step_and_check(m, A, hist["A"], "ckpt A, v0", False)
    eng = _engine(m)
    plan_a = _plan_of(eng, A[0][0])
    _step_and_check(m, B, hist["B"], "ckpt B, v0", False)
    plan_b = _plan_of(eng, B[0][0])
    assert len(eng.plans) == 2 and plan_a is not plan_b and plan_a["owned"][1] is not plan_b["owned"][1]
    _live_packer_is_the_last_plans(eng)
    version, sigs = 0, {"A": A, "B": B}
    for order in ("AB", "BA"):
        _update(m, gen)
        version += 1
        for name in order:
            _step_and_check(m, sigs[name], hist[name], f"ckpt {name}, v{version}", True)
            assert len(eng.plans) == 2 and _plan_of(eng, A[0][0]) is plan_a and _plan_of(eng, B[0][0]) is plan_b
            assert eng._last is (plan_a if name == "A" else plan_b)
            _live_packer_is_the_last_plans(eng)
            assert not eng.pool.live
    assert eng.checkpoint_blocks is True


@BACKENDS
def test_an_evicted_plan_is_recorded_again_under_checkpointing(backend, monkeypatch):
    """The step sequence of test_an_evicted_plan_is_recorded_again_and_leaves_nothing_behind under checkpointing."""
    m = _ckpt_student(backend)
    A, B = _two_signatures()
    hist = {"A": [], "B": []}
    _step_and_check(m, A, hist["A"], "ckpt A, v0", False)
    eng = _engine(m)
    monkeypatch.setattr(eng, "max_plans", 1)
    gone = [weakref.ref(eng._last["owned"][0]), weakref.ref(eng._last["owned"][1])]
    _step_and_check(m, B, hist["B"], "ckpt B, v0", False)
    assert len(eng.plans) == 1 and eng._last is _plan_of(eng, B[0][0])
    _live_packer_is_the_last_plans(eng)
    gone += [weakref.ref(eng._last["owned"][0]), weakref.ref(eng._last["owned"][1])]
    _update(m, torch.Generator().manual_seed(5))
    _step_and_check(m, A, hist["A"], "ckpt A again, v1", True)
    assert len(eng.plans) == 1 and eng._last is _plan_of(eng, A[0][0])
    _live_packer_is_the_last_plans(eng)
    for p in m.parameters():
        p.grad = None
    gc.collect()
    assert [r() for r in gone] == [None] * 4, "an evicted plan (or its Packer) is still referenced"


@BACKENDS
def test_batch2_motion_cond_under_checkpointing(backend):
    """B = 2 with two timesteps, fps = 8 and ``motion_cond``: per-clip column sums of d(loss)/d(emb_all) written once by the recomputed
    blocks' backward, per-clip text K / V projections made again inside the recomputation."""
    g = load("unet_tiny_mg_b2")
    m = _ckpt_student(backend, "unet_tiny_mg_b2", motion_cond_proj_dim=256)
    assert g["x"].shape[0] == 2 and int(g["ts"][0]) != int(g["ts"][1])
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(6))
    sig = ((g["x"], g["ts"], g["ctx"], g["tc"], r_out), dict(fps=8, mc=g["mc"]))
    hist = []
    _step_and_check(m, sig, hist, "ckpt B = 2 motion_cond, v0", False)
    assert all(float(hist[0][2][n].abs().max()) > 0 for n in ("motion_cond_proj.weight", "combine_proj.weight", "time_cond_proj.weight"))
    eng = _engine(m)
    plan = next(iter(eng.plans.values()))
    _update(m, torch.Generator().manual_seed(5))
    _step_and_check(m, sig, hist, "ckpt B = 2 motion_cond, v1", True)
    assert len(eng.plans) == 1 and next(iter(eng.plans.values())) is plan
    _live_packer_is_the_last_plans(eng)
    assert not eng.pool.live


def test_native_checkpoint_attribute_switches_the_engines(monkeypatch):
    """``UNetModel.native_checkpoint``: True / False force the mode of the engines the module builds; None (the default) follows
    T2V_NATIVE_CHECKPOINT, which unset means off; a later change goes through the ``checkpoint_blocks`` setter and drops the plans."""
    monkeypatch.setattr(UNetGradEngine, "_ckpt_env", "0")        # what an unset T2V_NATIVE_CHECKPOINT reads as
    m = _student()
    m._native_ops_factory = EmuOps
    assert m.native_checkpoint is None
    assert m.native_full_engine().checkpoint_blocks is False

    m = _student()
    m._native_ops_factory = EmuOps
    m.native_checkpoint = True
    eng = m.native_full_engine()
    assert eng.checkpoint_blocks is True and eng.training_full
    eng.plans["sentinel"] = {}
    m.native_checkpoint = True                                    # unchanged: the plans stay
    assert "sentinel" in eng.plans
    m.native_checkpoint = False
    assert eng.checkpoint_blocks is False and not eng.plans
    m.native_checkpoint = None
    assert eng.checkpoint_blocks is False

    monkeypatch.setattr(UNetGradEngine, "_ckpt_env", "1")        # the variable still rules where the attribute says nothing
    assert eng.checkpoint_blocks is True
    m.native_checkpoint = False
    assert eng.checkpoint_blocks is False


def test_native_checkpoint_attribute_reaches_the_lora_engines():
    from t2v_turbo_amd import lora
    from tests.test_unet_lora_grad_cpu import _student as lora_student
    m, _ = lora_student("unet_tiny", 64)
    m._native_ops_factory = EmuOps
    m.native_checkpoint = True
    assert lora.lora_parameters(m)
    assert m.native_train_engine().checkpoint_blocks is True and m.native_train_engine(forward_only=True).checkpoint_blocks is True
