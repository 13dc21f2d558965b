"""``t2v_adamw_multi`` / ``t2v_sumsq_multi`` / ``t2v_scale_multi`` — the kernel SOURCE on the host SIMT simulator — on the shared case
table (tests/adamw_cases.py): bit-identical to ``t2v_adamw8_step`` of the same build with every tensor under fp32 state, the moments
bit-equal to the torch definition of ``optim.py``, a deterministic gradient norm inside its derived bound, torch's clip coefficient,
nothing read or written outside the tensors, refusals of a malformed call."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from t2v_turbo_amd import native as nt
from tests.adamw_cases import B, CASES, NO_GRAD, AdamwCase, bits, check_against_adamw8, check_twin, many_groups, norm_bound, twin_step

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))


@pytest.fixture(scope="module")
def sim_ops():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    return HostSimOps(hostsim_build.build_full())


@pytest.mark.parametrize("host_scale, dev_scale", [(1.0, None), (0.37, None), (0.5, 0.74)])
def test_adamw_multi_is_the_fp32_state_branch_of_adamw8_bit_for_bit(sim_ops, host_scale, dev_scale):
    """One ``adamw_multi`` over the table: parameter and both moments bit-identical to ``t2v_adamw8_step`` (same build, same
    expressions) and to nothing less; the moments also bit-equal to the torch definition; guards and gradients bit-unchanged."""
    case = AdamwCase("cpu")
    snap = case.snapshot()
    table, n, work, hyper, order = case.table()
    scale_dev = None if dev_scale is None else torch.tensor([dev_scale])
    sim_ops.adamw_multi(table, n, work, hyper, host_scale, scale_dev)
    total = float(np.float32(host_scale) * np.float32(1.0 if dev_scale is None else dev_scale))
    check_against_adamw8(sim_ops, case, snap, total)
    case.check_guards(grads_equal_to=snap)
    assert case.no_grad_unchanged(snap, 3)
    case.check_against_definition(snap, total, label=f"hostsim x{total}")


def test_optimizer_step_through_the_table_matches_the_definition(sim_ops):
    """``optim.AdamW.step`` with the simulator as its library: one launch for the three rows, only the stepped tensors' ``step``
    advances, a second step reuses the table."""
    case = AdamwCase("cpu", seed=7, native_ops=sim_ops)
    for s in range(2):
        snap = case.snapshot()
        steps = {i: int(case.opt.state[case.params[i]]["step"]) + 1 for i in case.active}
        case.opt.step(grad_scale=0.37)
        case.check_against_definition(snap, 0.37, steps=steps, label=f"step {s + 1}")
        case.check_guards(grads_equal_to=snap)
        assert case.no_grad_unchanged(snap, 3)
        case.new_grads()
    assert len(case.opt._plan["launches"]) == 1 and case.opt.table_uploads == 1
    assert [int(case.opt.state[p]["step"]) for p in case.params[:3]] == [5, 5, 8]
    assert all(p._version > 0 for i, p in enumerate(case.params) if i != NO_GRAD)


def test_more_than_16_hyper_rows_take_a_second_launch(sim_ops):
    opt, params = many_groups("cpu", sim_ops)
    for s in range(2):
        want = twin_step(opt)
        opt.step()
        check_twin(opt, want, f"17 groups step {s + 1}")
    assert [(e - s, rows) for s, e, _, _, rows in opt._plan["launches"]] == [(16, 16), (1, 1)] and opt.table_uploads == 1


def _grad_table(case):
    table, n, work, _, order = case.table()
    return table, n, work, order


def _sum64(case, order):
    return sum(float((case.tensors(i)[1].double() ** 2).sum()) for i in order)


def test_sumsq_multi_is_deterministic_and_inside_its_bound(sim_ops):
    """The relative error of the squared norm against the float64 sum of squares is at most (k + 2) * 2**-24, doubled for margin,
    with k = 23: the longest chain of fp32 additions in a block partial (15 serial additions of a lane's 16 squares + 6 levels of
    the wave shuffle tree + 2 levels over the four waves); the finishing sum is in double.  A finite norm also shows that no guard
    (a NaN) was read."""
    case = AdamwCase("cpu", seed=8)
    table, n, work, order = _grad_table(case)
    want = _sum64(case, order)
    for max_norm in (0.5 * want ** 0.5, 4.0 * want ** 0.5, 0.0):   # one that clips, one that does not, clipping off
        outs = []
        for _ in range(2):
            ws, out = torch.full((work + 3,), 7.0), torch.full((3,), 7.0)
            sim_ops.sumsq_multi(table, n, work, ws, max_norm, out)
            outs.append((ws, out))
        assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
        ws, out = outs[0]
        assert bool(torch.isfinite(out).all()) and bool((ws[work:] == 7.0).all()) and float(out[2]) == 7.0
        err = abs(float(out[0].double() ** 2) - want) / want
        print(f"sum of squares: relative error {err:.3e}, bound {norm_bound():.3e}", flush=True)
        assert err <= norm_bound()
        coef = torch.clamp(max_norm / (out[0] + 1e-6), max=1.0) if max_norm > 0 else torch.tensor(1.0)
        ulp = float(torch.nextafter(coef, torch.tensor(2.0)) - coef)
        assert abs(float(out[1]) - float(coef)) <= 2 * ulp
        assert (float(out[1]) < 1.0) == (0 < max_norm < want ** 0.5)
    case.check_guards()


def test_sumsq_multi_unowned_blocks_write_zero(sim_ops):
    case = AdamwCase("cpu", seed=8)
    table, n, work, order = _grad_table(case)
    ws, out, ref = torch.full((work + 3,), 7.0), torch.zeros(2), torch.zeros(2)
    sim_ops.sumsq_multi(table, n, work + 3, ws, 1.0, out)
    sim_ops.sumsq_multi(table, n, work, torch.zeros(work), 1.0, ref)
    assert bool((ws[work:] == 0.0).all()) and bool((ws[:work] > 0).all()) and torch.equal(bits(out), bits(ref))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_gives_torchs_coefficient(sim_ops, bad):
    case = AdamwCase("cpu", seed=9)
    case.params[10].grad[4100] = bad
    table, n, work, order = _grad_table(case)
    out = torch.zeros(2)
    sim_ops.sumsq_multi(table, n, work, torch.zeros(work), 1.0, out)
    want = torch.clamp(1.0 / (out[0] + 1e-6), max=1.0)
    assert not bool(torch.isfinite(out[0])) and bool(torch.isnan(out[0])) == bool(torch.isnan(want))
    if bad == float("inf"):
        assert float(want) == 0.0 and torch.equal(bits(out[1:]), bits(want.reshape(1)))
    else:
        assert bool(torch.isnan(want)) and bool(torch.isnan(out[1]))


def test_scale_multi(sim_ops):
    case = AdamwCase("cpu", seed=10)
    table, n, work, order = _grad_table(case)
    norm = _sum64(case, order) ** 0.5
    for max_norm, clips in ((0.25 * norm, True), (4.0 * norm, False)):
        snap = case.snapshot()
        out = torch.zeros(2)
        sim_ops.sumsq_multi(table, n, work, torch.zeros(work), max_norm, out)
        sim_ops.scale_multi(table, n, work, out[1:])
        assert (float(out[1]) < 1.0) == clips
        if clips:
            for i in order:
                assert torch.equal(bits(case.tensors(i)[1]), bits(case._span(snap, "g", i) * out[1])), CASES[i]
            case.check_guards()
        else:
            assert float(out[1]) == 1.0
            case.check_guards(grads_equal_to=snap)
        for k in "pmv":
            assert torch.equal(bits(case.arena[k]), bits(snap[k]))


def test_malformed_calls_are_refused(sim_ops):
    case = AdamwCase("cpu", seed=11)
    snap = case.snapshot()
    table, n, work, hyper, order = case.table()
    lib = sim_ops.lib
    rows = (nt.AdamwHyper * 17)(*[nt.AdamwHyper(*hyper[i % 3]) for i in range(17)])
    hp = ctypes.cast(rows, ctypes.c_void_p)
    t = table.data_ptr()
    assert lib.t2v_adamw_multi(t, n, work, hp, 3, 1.0, None, None) == 0
    case.restore(snap)
    for args in ((None, n, work, hp, 3), (t, n, work, None, 3), (t, 0, work, hp, 3), (t, -1, work, hp, 3), (t, n, n - 1, hp, 3),
                 (t, n, work, hp, 0), (t, n, work, hp, 17)):
        assert lib.t2v_adamw_multi(*args, 1.0, None, None) == -1, args                    # T2V_EINVAL
    zero_step = (nt.AdamwHyper * 3)(*[nt.AdamwHyper(*(hyper[i][:5] + (0 if i == 2 else 4,))) for i in range(3)])
    assert lib.t2v_adamw_multi(t, n, work, ctypes.cast(zero_step, ctypes.c_void_p), 3, 1.0, None, None) == -1
    off = torch.zeros(table.numel() + 8, dtype=torch.uint8)
    off[4:4 + table.numel()] = table
    assert off.data_ptr() % 8 == 0 and lib.t2v_adamw_multi(off.data_ptr() + 4, n, work, hp, 3, 1.0, None, None) == -2   # T2V_ESHAPE
    ws, out = torch.zeros(work), torch.zeros(2)
    assert lib.t2v_sumsq_multi(None, n, work, ws.data_ptr(), 1.0, out.data_ptr(), None) == -1
    assert lib.t2v_sumsq_multi(t, n, n - 1, ws.data_ptr(), 1.0, out.data_ptr(), None) == -1
    assert lib.t2v_scale_multi(t, n, work, None, None) == -1 and lib.t2v_scale_multi(t, 0, work, out.data_ptr(), None) == -1
    for k in "pgmv":
        assert torch.equal(bits(case.arena[k]), bits(snap[k]))
    assert nt.C.sizeof(nt.AdamwTensor) == 56 and table.numel() == 56 * n and nt.C.sizeof(nt.AdamwHyper) == 24 and B == 4096
