"""The consistency-head kernels of csrc/train.hip (``t2v_cd_solver_step``, ``t2v_cd_loss_fwd``, ``t2v_cd_loss_bwd``) executed thread by thread
on the host SIMT simulator, through ``HostSimOps``: the case table and bounds of tests/cd_head_cases.py."""
import ctypes as C
import os
import shutil
import sys

import pytest
import torch

from t2v_turbo_amd import native as nt
from tests import cd_head_cases as cc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))


@pytest.fixture(scope="module")
def sim():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    return HostSimOps(hostsim_build.build())


@pytest.mark.parametrize("geom,in_dtype,out_dtype,with_score", cc.SOLVER_PARAMS)
def test_solver_step_on_the_case_table(sim, geom, in_dtype, out_dtype, with_score):
    case = cc.solver_case(geom, in_dtype, with_score)
    x0 = cc.run_solver(sim, "cpu", case, cc.DTYPES[out_dtype])
    cc.check_solver(case, x0)
    assert torch.equal(cc.run_solver(sim, "cpu", case, cc.DTYPES[out_dtype]).view(torch.uint8), x0.view(torch.uint8))


@pytest.mark.parametrize("geom,in_dtype,xp_dtype,loss_type,with_g", cc.LOSS_PARAMS)
def test_loss_forward_and_backward_on_the_case_table(sim, geom, in_dtype, xp_dtype, loss_type, with_g):
    case = cc.loss_case(geom, in_dtype, xp_dtype, loss_type, with_g)
    first = cc.run_loss(sim, "cpu", case)
    cc.check_loss(case, *first)
    again = cc.run_loss(sim, "cpu", case)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, again))


@pytest.mark.parametrize("in_dtype", list(cc.DTYPES))
def test_bases_off_a_16_byte_boundary_take_the_scalar_path(sim, in_dtype):
    case = cc.solver_case("misaligned", in_dtype, True)
    cc.check_solver(case, cc.run_solver(sim, "cpu", case, torch.bfloat16, misalign=True), " (unaligned)")
    lcase = cc.loss_case("misaligned", in_dtype, "bf16", "huber", True)
    cc.check_loss(lcase, *cc.run_loss(sim, "cpu", lcase, misalign=True), " (unaligned)")


def test_an_index_outside_the_tables_reads_nothing_out_of_bounds(sim):
    """The kernels clamp: an index far outside [0, 50) behaves as the nearest valid one (the Python layer refuses it beforehand)."""
    case = dict(cc.solver_case("tail", "fp32", True))
    ok = cc.run_solver(sim, "cpu", dict(case, index=torch.tensor([49])), torch.float32)
    assert torch.equal(cc.run_solver(sim, "cpu", dict(case, index=torch.tensor([1 << 40])), torch.float32), ok)
    lo = cc.run_solver(sim, "cpu", dict(case, index=torch.tensor([0])), torch.float32)
    assert torch.equal(cc.run_solver(sim, "cpu", dict(case, index=torch.tensor([-7])), torch.float32), lo)


def test_refusals_return_the_error_codes_before_any_launch(sim):
    EINVAL, ESHAPE = -1, -2
    acp, solver = cc.schedule()
    tabs = (acp, solver.ddim_timesteps, solver.ddim_alpha_cumprods_prev.float(), torch.tensor([3, 4]))
    sched = sim.cd_sched(*tabs, cc.TOPK, cc.SCALING)
    B, per = 2, 40
    x = torch.randn(B, per)
    w, mgs, umg = torch.ones(B), torch.ones(B), torch.ones(B, dtype=torch.bool)
    nan = float("nan")
    out, mp, u, d = (torch.full((B, per), nan) for _ in range(4))
    ws, loss = torch.full((8,), nan), torch.full((1,), nan)
    lib, p, S = sim.lib, (lambda t: None if t is None else t.data_ptr()), C.byref(sched)

    def solver_step(s=S, z=x, score=x, dt_in=nt.F32, dt_out=nt.F32, w_=w, B_=B, per_=per):
        return lib.t2v_cd_solver_step(s, p(z), p(x), p(x), p(score), dt_in, p(w_), p(mgs), p(umg), 25, p(out), dt_out, B_, per_, None)

    def loss_fwd(s=S, np_=x, dt_np=nt.F32, dt_z=nt.F32, lt=nt.CD_HUBER, nws=8, B_=B, per_=per, u_=u):
        return lib.t2v_cd_loss_fwd(s, p(np_), dt_np, p(x), nt.F32, p(x), dt_z, p(x), nt.F32, lt, 0.001, p(mp), p(u_), p(ws), nws, p(loss),
                                   B_, per_, None)

    def loss_bwd(s=S, u_=x, dt_out=nt.F32, B_=B, per_=per):
        return lib.t2v_cd_loss_bwd(s, p(u_), None, None, p(d), dt_out, B_, per_, None)

    for call in (solver_step, loss_fwd, loss_bwd):
        assert call(s=None) == EINVAL and call(B_=0) == EINVAL and call(per_=0) == EINVAL and call(per_=-5) == EINVAL
        assert call(B_=nt.CD_MAX_CLIPS + 1) == ESHAPE
        broken = nt.CdSched.from_buffer_copy(sched)
        broken.ddim_timesteps = None
        assert call(s=C.byref(broken)) == EINVAL
        broken = nt.CdSched.from_buffer_copy(sched)
        broken.n_ddim = 0
        assert call(s=C.byref(broken)) == EINVAL
    assert solver_step(z=None) == EINVAL and solver_step(w_=None) == EINVAL
    assert solver_step(dt_in=3) == ESHAPE and solver_step(dt_out=-1) == ESHAPE
    assert loss_fwd(np_=None) == EINVAL and loss_fwd(u_=None) == EINVAL and loss_fwd(lt=2) == EINVAL
    assert loss_fwd(dt_np=nt.F16) == ESHAPE and loss_fwd(dt_z=7) == ESHAPE
    assert sim.cd_loss_ws_floats(B, per) == 2 and sim.cd_loss_ws_floats(3, 2049) == 6
    assert loss_fwd(nws=1) == ESHAPE
    assert loss_bwd(u_=None) == EINVAL and loss_bwd(dt_out=nt.F16) == ESHAPE
    for t in (out, mp, u, d, ws, loss):
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"
    assert solver_step() == 0 and solver_step(score=None) == 0 and loss_fwd() == 0 and loss_bwd() == 0
    assert not any(bool(torch.isnan(t).any()) for t in (out, mp, u, d, loss)) and bool(torch.isnan(ws[2:]).all())
