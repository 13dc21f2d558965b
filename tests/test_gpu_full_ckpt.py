"""Activation checkpointing under FULL fine-tuning on MI355X (``UNetModel.native_checkpoint = True``: the yaml's ``use_checkpoint: true``
with every UNet parameter trainable, train_latent_t2v_turbo_v2.py).  Tiny width only — the smallest shape at which every leaf type and
gather mode occurs.  The recomputation issues the recorded launches of each block's forward again inside the backward list, so on the
device the result must be the tape's bit for bit; the gradients themselves are checked against the imported reference's own
(tests/golden/unet_tiny_full_grad.npz, unet_tiny_mg_b2_full_grad.npz) and against fp32 CPU autograd after weight updates, with the
helpers and tolerances of tests/test_gpu_train_parity.py.  (The bodies take a device and an op-backend factory so that they can be
dry-run on the CPU under the replay protocol.)"""
import copy
import warnings

import pytest
import torch

from tests.util import load, manifest, tiny_unet_params

pytestmark = pytest.mark.gpu


def _tiny(fixture="unet_tiny", **cfg):
    from oracle.synth import synth_state_dict
    from t2v_turbo_amd.unet3d import UNetModel
    ref = UNetModel(**tiny_unet_params(**cfg))
    ref.load_state_dict(synth_state_dict(manifest(fixture)), strict=True)
    ref.requires_grad_(True)
    ref.eval()
    return ref


def test_full_fine_tuning_checkpointing_on_device_is_the_tape_bit_for_bit():
    run_off_against_on(torch.device("cuda", 0), None)


def run_off_against_on(dev, emu_factory):
    """Train mode (live TemporalConvBlock dropouts: the recomputed counter-based masks must be the forward's), checkpoint off against on,
    three repetitions each (record, replay, replay): output, d/d(latents) and all parameter gradients bit-identical between the modes and
    across the repetitions, from a pool below 0.6 x the tape's, an unchanged forward list and a backward list longer by most of a
    forward.  Then the same plan under hipGraph replay of both lists."""
    from tests.test_unet_full_grad_cpu import _fixture_step
    g = load("unet_tiny")
    cuda = torch.device(dev).type == "cuda"
    route = "auto" if cuda else "train"
    args = tuple(t.to(dev) for t in (g["x"], g["ts"], g["ctx"], g["tc"], torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(5))))
    res = {}

    def step(m):
        torch.manual_seed(4242)     # the forward draws its dropout seed from torch's generator: the same masks in every step
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y, dx, grads = _fixture_step(m, *args, route)
        assert all(t is not None for t in grads)
        return [y.clone(), dx.clone()] + [t.clone() for t in grads]

    def same(a, b):
        return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))

    for ck in (False, True):
        m = _tiny().to(dev).train()
        if emu_factory is not None:
            m._native_ops_factory = emu_factory
        m.native_checkpoint = ck
        outs = [step(m) for rep in range(3)]
        eng = m._engine_box.full
        assert eng is not None and eng.checkpoint_blocks is ck and len(eng.plans) == 1
        assert same(outs[1], outs[0]) and same(outs[2], outs[0])
        plan = eng._last
        res[ck] = dict(out=outs[0], pool=eng.pool.bytes, n_fwd=len(plan["rec"]), n_bwd=len(plan["rec_bwd"]), sites=len(eng.drop_sites),
                       live=len(eng.pool.live))
        if cuda:
            eng.use_graph = True
            for rep in range(3):    # capture both lists, then replay the graphs
                assert same(step(m), outs[0]), (ck, rep)
            assert eng._last is plan and "graph_failed" not in plan, plan.get("graph_failed")
            assert plan.get("graph_rec") is not None and plan.get("graph_rec_bwd") is not None
            eng.use_graph = False
            torch.cuda.synchronize()
    a, b = res[False], res[True]
    print(f"[full fine-tuning, checkpoint] activation pool {a['pool'] / 2**20:.1f} MiB (tape) -> {b['pool'] / 2**20:.1f} MiB "
          f"({b['pool'] / a['pool']:.3f}); launches forward {a['n_fwd']} / {b['n_fwd']}, backward {a['n_bwd']} -> {b['n_bwd']}; "
          f"dropout sites {a['sites']} / {b['sites']}", flush=True)
    assert all(float(t.float().abs().sum()) > 0 for t in a["out"])
    assert same(a["out"], b["out"])
    assert a["sites"] == b["sites"] > 0
    assert a["live"] == 0 and b["live"] == 0
    assert b["pool"] < 0.6 * a["pool"] and a["n_fwd"] == b["n_fwd"] and b["n_bwd"] > a["n_bwd"] + 0.8 * a["n_fwd"]


def test_full_fine_tuning_checkpointing_on_device_vs_the_reference_gradient_fixture():
    from tests.test_gpu_train_parity import DX_TOL, OUT_TOL
    run_vs_the_reference_fixture(torch.device("cuda", 0), None, (OUT_TOL, DX_TOL, 0.10, (0.30, 0.06), 0.12))


def run_vs_the_reference_fixture(dev, emu_factory, fixture_tol, **tol):
    """Checkpointing on, the module route "auto" without the torch-composite warning: one step (recording pass, then a replay) against the
    imported reference's own gradients of all 1485 parameters, then three optimizer-style updates of every weight on the SAME plan, each
    against fp32 CPU autograd — eager pack refresh, captured refresh, replayed refresh (engine_full._refresh), under a backward list that
    re-reads the packs in every recomputed block."""
    from tests.golden.make_golden_full_grad import SEED_R
    from tests.test_gpu_train_parity import _full_step_vs_cpu_autograd, _module_route, _seeded_update
    from tests.test_unet_full_grad_cpu import _fixture_step, check_against_reference_fixture
    g, gg = load("unet_tiny"), load("unet_tiny_full_grad")
    ref = _tiny()
    m = copy.deepcopy(ref).to(dev)
    if emu_factory is not None:
        m._native_ops_factory = emu_factory
    m.native_checkpoint = True
    names = [n for n, _ in m.named_parameters()]
    r_out = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(SEED_R))
    cpu_args = (g["x"], g["ts"], g["ctx"], g["tc"], r_out)
    for rep in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y, dx, grads = _fixture_step(m, *(t.to(dev) for t in cpu_args), _module_route(dev))
        eng = m._engine_box.full
        assert eng is not None and eng.checkpoint_blocks is True and len(eng.plans) == 1
        check_against_reference_fixture(y.cpu(), dx.cpu(), [t.cpu() for t in grads], names, gg, *fixture_tol)
    plan = next(iter(eng.plans.values()))
    gen = torch.Generator().manual_seed(5)
    prev = (gg["out"], gg["dx"])
    for upd in range(3):
        _seeded_update(ref, m, gen)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            prev = _full_step_vs_cpu_autograd(ref, m, cpu_args, {}, prev, f"checkpointed, after update {upd + 1}", **tol)
        assert next(iter(eng.plans.values())) is plan and len(eng.plans) == 1
    if eng.refresh_graph and torch.device(dev).type == "cuda":
        assert eng._refresh_state["graph"] is not None and not eng._refresh_state["failed"], "the pack refresh was not captured"


def test_full_fine_tuning_checkpointing_batch2_motion_cond_on_device_vs_the_reference_fixture():
    from tests.test_gpu_train_parity import DX_TOL, OUT_TOL
    run_batch2_motion_cond(torch.device("cuda", 0), None, (OUT_TOL, DX_TOL, 0.10, (0.30, 0.06), 0.12))


def run_batch2_motion_cond(dev, emu_factory, fixture_tol, **tol):
    """B = 2 with two timesteps, fps = 8 and ``motion_cond`` under checkpointing against tests/golden/unet_tiny_mg_b2_full_grad.npz
    (recording pass and one replay), then one weight update against fp32 CPU autograd: the steps and tolerances of the B = 2 device test."""
    from tests.golden.make_golden_full_grad import SEED_R
    from tests.test_gpu_train_parity import _full_step_vs_cpu_autograd, _module_route, _seeded_update
    from tests.test_unet_full_grad_cpu import _fixture_step, check_against_reference_fixture
    g, gg = load("unet_tiny_mg_b2"), load("unet_tiny_mg_b2_full_grad")
    ref = _tiny("unet_tiny_mg_b2", motion_cond_proj_dim=256)
    m = copy.deepcopy(ref).to(dev)
    if emu_factory is not None:
        m._native_ops_factory = emu_factory
    m.native_checkpoint = True
    names = [n for n, _ in m.named_parameters()]
    r_out = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(SEED_R))
    cpu_args = (g["x"], g["ts"], g["ctx"], g["tc"], r_out)
    for rep in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert m._auto_route(g["x"].to(dev).clone().requires_grad_(True), g["ctx"].to(dev), g["tc"].to(dev), None)[0] == "train_full"
            y, dx, grads = _fixture_step(m, *(t.to(dev) for t in cpu_args), _module_route(dev), 8, g["mc"].to(dev))
        eng = m._engine_box.full
        assert eng is not None and eng.checkpoint_blocks is True and len(eng.plans) == 1
        check_against_reference_fixture(y.cpu(), dx.cpu(), [t.cpu() for t in grads], names, gg, *fixture_tol)
    plan = next(iter(eng.plans.values()))
    _seeded_update(ref, m, torch.Generator().manual_seed(5))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _full_step_vs_cpu_autograd(ref, m, cpu_args, dict(fps=8, mc=g["mc"]), (gg["out"], gg["dx"]), "checkpointed B = 2 motion_cond, after the update", **tol)
    assert next(iter(eng.plans.values())) is plan and len(eng.plans) == 1
