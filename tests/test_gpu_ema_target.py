"""-m gpu: the EMA target network of train_latent_t2v_turbo_v2.py --use_target_unet on the device — ``t2v_ema_multi`` on the shared case
table, the inference engine keeping its plans across ``optim.update_ema`` (eager refresh, captured refresh, replayed refresh; plain
replay and hipGraph), the train-mode target, and the v2 step through the module route."""
import copy
import itertools
import warnings

import pytest
import torch

from t2v_turbo_amd import native as nt
from t2v_turbo_amd import optim
from t2v_turbo_amd.engine import UNetEngine
from tests.ema_cases import EmaCase, RATE
from tests.test_ema_target_cpu import _model, _tiny_case
from tests.util import load

pytestmark = pytest.mark.gpu


def test_ema_multi_on_the_case_table():
    ops = nt.HipOps()
    case = EmaCase("cuda")
    table, n, work = case.table()
    ops.ema_multi(table, n, work, RATE)
    torch.cuda.synchronize()
    case.check(ops)
    lib = ops.lib
    assert lib.t2v_ema_multi(None, n, work, RATE, None) == -1 and lib.t2v_ema_multi(table.data_ptr(), 0, work, RATE, None) == -1
    assert lib.t2v_ema_multi(table.data_ptr(), n, 0, RATE, None) == -1


def test_update_ema_is_one_launch_with_a_cached_table():
    """``optim.update_ema`` on device tensors: one ``t2v_ema_multi`` for the pairs that qualify (fp32 and bf16 sources), the torch
    expression for the rest (a non-contiguous target, an fp16 target), the table built once, the target's fingerprint moved."""
    from t2v_turbo_amd.engine import params_fingerprint
    gen = torch.Generator().manual_seed(2)
    shapes = [(320,), (64, 33), (5000,), (3, 3, 3, 7)]
    tg = [torch.nn.Parameter(torch.randn(s, generator=gen).cuda(), requires_grad=False) for s in shapes]
    sr = [torch.randn(s, generator=gen).cuda() for s in shapes]
    sr[2] = sr[2].bfloat16()
    tg += [torch.nn.Parameter(torch.randn(6, 8, generator=gen).cuda().t(), requires_grad=False),
           torch.nn.Parameter(torch.randn(9, generator=gen).cuda().half(), requires_grad=False)]
    sr += [torch.randn(8, 6, generator=gen).cuda(), torch.randn(9, generator=gen).cuda()]
    holder = torch.nn.ParameterList(tg)
    want = [t.detach().clone() for t in tg]
    calls = []
    ops = nt.shared_ops()
    real = ops.ema_multi
    ops.ema_multi = lambda *a: (calls.append(a[1:3]), real(*a))[1]
    try:
        for rnd in range(3):
            fp = params_fingerprint(holder)
            for w, s in zip(want, sr):
                w.copy_(w * RATE + s.to(w.dtype) * (1 - RATE))
            optim.update_ema(holder.parameters(), (s for s in sr), RATE)
            assert params_fingerprint(holder) != fp
    finally:
        del ops.ema_multi
    torch.cuda.synchronize()
    assert calls == [(4, sum((t.numel() + nt.EMA_BLOCK - 1) // nt.EMA_BLOCK for t in tg[:4]))] * 3
    key = [k for k in optim._EMA_TABLES if k[0][0] == tg[0].data_ptr()]
    assert len(key) == 1                                       # one table for the three updates
    for t, w in zip(tg[:4], want[:4]):
        assert torch.allclose(t, w, rtol=3e-6, atol=3e-7)      # (three updates: three times the single update's bound)
    for t, w in zip(tg[4:], want[4:]):
        assert torch.allclose(t.float(), w.float(), rtol=2e-3, atol=1e-6)


def _cuda_case():
    cfg, args = _tiny_case()
    return cfg, tuple(a.cuda() if torch.is_tensor(a) else a for a in args)


@pytest.mark.parametrize("use_graph", [False, True], ids=["replay", "hipgraph"])
def test_three_updates_keep_the_plan_and_equal_a_fresh_engine(use_graph):
    """Forward, then three rounds of ``update_ema`` + forward — on the device the eager refresh, its capture, and the replay of the
    captured refresh (``use_graph``: the plan's own hipGraph is captured in round 2 and replayed in round 3).  After each round the
    output is bit-identical to a fresh engine's on the same weights; one recording in all."""
    cfg, args = _cuda_case()
    m, other = _model(cfg).cuda(), _model(cfg, seed=77).cuda()
    ops = nt.HipOps()
    eng = UNetEngine(m, ops)
    eng.use_graph = use_graph
    with warnings.catch_warnings():
        # (a refresh or a launch list that cannot be captured warns and stays eager: not here)
        warnings.filterwarnings("error", message="pack refresh not capturable")
        warnings.filterwarnings("error", message="hipGraph capture of")
        with torch.no_grad():
            last = eng(*args)
        (key, plan), = eng.plans.items()
        ptrs = eng.pk.pointers()
        for rnd in range(1, 4):
            optim.update_ema(m.parameters(), other.parameters(), 0.5)
            with torch.no_grad():
                y = eng(*args)
                fresh = UNetEngine(m, ops)(*args)
            assert eng.plans[key] is plan and eng.counters == {"recorded": 1, "refreshed": rnd}
            assert eng.pk.pointers() == ptrs
            assert torch.isfinite(y).all() and not torch.equal(y, last)
            assert torch.equal(y, fresh), (use_graph, rnd, float((y - fresh).abs().max()))
            last = y
    if eng.refresh_graph:
        st = eng.pk_refresh["refresh"]
        assert st["graph"] is not None and not st["failed"], "the pack refresh was not captured"
    if use_graph:
        assert plan.get("graph") is not None, plan.get("graph_failed")


def test_train_mode_target_keeps_its_plan():
    """The target as the reference leaves it: frozen, in ``.train()`` (train_latent_t2v_turbo_v2.py:671-675), called under ``no_grad``
    — the TemporalConvBlock dropouts are live and applied as counter-based masks.  The plan (and its seed buffer) is kept across
    updates; outputs are finite and follow the weights.  Bit-equality with a fresh engine is asserted in eval mode only (the test
    above): the counter-based masks advance per call, so two engines agree only call for call from the same seed sequence."""
    cfg, args = _cuda_case()
    m, other = _model(cfg).cuda(), _model(cfg, seed=77).cuda()
    m.train()
    eng = UNetEngine(m, nt.HipOps())
    eng.seed_source = itertools.repeat(1234)    # one mask for every call: what moves the output below is the update
    with torch.no_grad():
        y0 = eng(*args)
        assert torch.equal(eng(*args), y0)
    (key, plan), = eng.plans.items()
    assert "seed" in plan["static"] and len(eng.drop_sites) > 0
    last = y0
    for rnd in range(1, 4):
        optim.update_ema(m.parameters(), other.parameters(), 0.5)
        with torch.no_grad():
            y = eng(*args)
        assert eng.plans[key] is plan and eng.counters == {"recorded": 1, "refreshed": rnd}
        assert torch.isfinite(y).all() and not torch.equal(y, last)
        last = y
    assert not torch.equal(last, y0)


def test_v2_step_with_a_target_network_through_the_module_route():
    """train_latent_t2v_turbo_v2.py --use_target_unet at tiny width, three steps: the student (every parameter trainable, train mode,
    ``motion_cond``) forward / backward on the full fine-tuning route, ``AdamW8bit.step()``, ``update_ema`` of the frozen train-mode
    target, the target's forward under ``no_grad`` on the inference route.  No composite path (RuntimeWarning), ONE recording of the
    target, finite outputs, and the target's parameters equal the torch EMA of the recorded student weights."""
    from tests.test_unet_full_grad_cpu import _student
    g = load("unet_tiny_mg_b2")
    student = _student("unet_tiny_mg_b2", motion_cond_proj_dim=256).cuda()
    student.requires_grad_(True).train()
    target = copy.deepcopy(student).requires_grad_(False).train()
    x, ts, ctx, tc, mc = (g[k].cuda() for k in ("x", "ts", "ctx", "tc", "mc"))
    kw = dict(context=ctx, fps=8, timestep_cond=tc, motion_cond=mc)
    opt = optim.AdamW8bit(student.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    want = [p.detach().clone() for p in target.parameters()]
    outs = []
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for step in range(3):
            opt.zero_grad()
            y = student(x, ts, **kw)
            loss = (y.float() - 0.1).pow(2).mean()
            loss.backward()
            opt.step()
            optim.update_ema(target.parameters(), student.parameters(), 0.95)
            for w, s in zip(want, student.parameters()):
                w.copy_(w * 0.95 + s.detach() * 0.05)
            with torch.no_grad():
                outs.append(target(x, ts, **kw))
            assert torch.isfinite(y).all() and torch.isfinite(outs[-1]).all() and bool(torch.isfinite(loss))
    torch.cuda.synchronize()
    eng = target._engine_box.engine
    # (the target's first forward comes after the first update: it records; the other two find moved weights and refresh)
    assert type(eng) is UNetEngine and eng.counters == {"recorded": 1, "refreshed": 2} and len(eng.plans) == 1
    assert student._engine_box.full is not None and all(p.grad is not None for p in student.parameters())
    assert not torch.equal(outs[0], outs[2])
    for (name, p), w in zip(target.named_parameters(), want):
        assert torch.allclose(p, w, rtol=1e-6, atol=1e-7), name
