"""-m gpu: the consistency-head kernels on the device — the case table and bounds of tests/cd_head_cases.py (shared with the host-simulator
test), and ``cd_head``'s public entry points (the autograd Function) against the twin's autograd at the seam."""
import pytest
import torch

from t2v_turbo_amd import cd_head
from t2v_turbo_amd import native as nt
from tests import cd_head_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return nt.HipOps()


def _same_bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("geom,in_dtype,out_dtype,with_score", cc.SOLVER_PARAMS)
def test_solver_step_on_the_case_table(ops, geom, in_dtype, out_dtype, with_score):
    case = cc.solver_case(geom, in_dtype, with_score)
    x0 = cc.run_solver(ops, "cuda", case, cc.DTYPES[out_dtype])
    cc.check_solver(case, x0)
    assert _same_bits(cc.run_solver(ops, "cuda", case, cc.DTYPES[out_dtype]), x0)


@pytest.mark.parametrize("geom,in_dtype,xp_dtype,loss_type,with_g", cc.LOSS_PARAMS)
def test_loss_forward_and_backward_on_the_case_table(ops, geom, in_dtype, xp_dtype, loss_type, with_g):
    case = cc.loss_case(geom, in_dtype, xp_dtype, loss_type, with_g)
    first = cc.run_loss(ops, "cuda", case)
    cc.check_loss(case, *first)
    again = cc.run_loss(ops, "cuda", case)
    assert all(_same_bits(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("in_dtype", list(cc.DTYPES))
def test_bases_off_a_16_byte_boundary_take_the_scalar_path(ops, in_dtype):
    case = cc.solver_case("misaligned", in_dtype, True)
    cc.check_solver(case, cc.run_solver(ops, "cuda", case, torch.bfloat16, misalign=True), " (unaligned)")
    lcase = cc.loss_case("misaligned", in_dtype, "bf16", "huber", True)
    cc.check_loss(lcase, *cc.run_loss(ops, "cuda", lcase, misalign=True), " (unaligned)")


@pytest.mark.parametrize("geom,in_dtype,loss_type,with_g", [("misaligned", "bf16", "huber", True), ("workgroups", "fp32", "huber", False),
                                                            ("workgroups", "fp16", "l2", True), ("tail", "bf16", "l2", False)])
def test_public_entry_points_against_the_twins_autograd_at_the_seam(geom, in_dtype, loss_type, with_g):
    """``solver_step_v2`` and ``consistency_loss`` on CUDA tensors (the kernels, through the autograd Function): x_prev, loss,
    model_pred and ``noise_pred.grad`` against the float64 twin, by the bounds of the case table."""
    acp, solver = cc.schedule()
    sc = cc.solver_case(geom, in_dtype, True)
    x_prev = cd_head.solver_step_v2(solver, acp, sc["index"].cuda(), sc["z"].cuda(), sc["c"].cuda(), sc["u"].cuda(), sc["score"].cuda(),
                                    sc["w"].cuda(), sc["mgs"].cuda(), sc["umg"].cuda(), min_index=cc.MIN_INDEX)
    assert x_prev.is_cuda and x_prev.dtype == cc.DTYPES[in_dtype]
    cc.check_solver(sc, x_prev)
    xp_dtype = "fp32" if in_dtype == "fp32" else "bf16"
    case = cc.loss_case(geom, in_dtype, xp_dtype, loss_type, with_g)
    noise_pred = case["np"].cuda().requires_grad_(True)
    loss, model_pred = cd_head.consistency_loss(solver, acp, case["index"].cuda(), noise_pred, case["tnp"].cuda(), case["z"].cuda(),
                                                case["x_prev"].cuda(), topk=cc.TOPK, timestep_scaling=cc.SCALING, loss_type=loss_type,
                                                huber_c=cc.HUBER_C)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and model_pred.dtype == torch.float32 and model_pred.requires_grad
    total = loss * case["g_loss"].cuda() + (model_pred * case["g_mp"].cuda()).sum() if with_g else loss
    total.backward()
    torch.cuda.synchronize()
    assert noise_pred.grad.dtype == noise_pred.dtype
    cc.check_loss(case, loss.detach(), model_pred.detach(), noise_pred.grad)
    # T2V_NATIVE_CD_HEAD=0: the twin on the same CUDA tensors
    import os
    os.environ["T2V_NATIVE_CD_HEAD"] = "0"
    try:
        np2 = case["np"].cuda().requires_grad_(True)
        loss2, mp2 = cd_head.consistency_loss(solver, acp, case["index"].cuda(), np2, case["tnp"].cuda(), case["z"].cuda(),
                                              case["x_prev"].cuda(), topk=cc.TOPK, timestep_scaling=cc.SCALING, loss_type=loss_type,
                                              huber_c=cc.HUBER_C)
        assert type(loss2.grad_fn).__name__ != "_ConsistencyLossBackward"
    finally:
        del os.environ["T2V_NATIVE_CD_HEAD"]
    assert abs(float(loss2.detach()) - float(loss.detach())) <= 2e-5 * float(loss.detach())


def test_refusals_are_raised_before_any_launch(ops):
    acp, solver = cc.schedule()
    dev = "cuda"
    tabs = (acp.to(dev), solver.ddim_timesteps.to(dev), solver.ddim_alpha_cumprods_prev.float().to(dev), torch.tensor([3, 4], device=dev))
    sched = ops.cd_sched(*tabs, cc.TOPK, cc.SCALING)
    B, per = 2, 40
    x = torch.randn(B, per, device=dev)
    w, mgs, umg = torch.ones(B, device=dev), torch.ones(B, device=dev), torch.ones(B, dtype=torch.bool, device=dev)
    nan = float("nan")
    out, mp, u, d = (torch.full((B, per), nan, device=dev) for _ in range(4))
    ws, loss = torch.full((8,), nan, device=dev), torch.full((1,), nan, device=dev)
    bad = nt.CdSched.from_buffer_copy(sched)
    bad.n_ddim = 0
    null = nt.CdSched.from_buffer_copy(sched)
    null.index = None
    refused = [
        lambda: ops.cd_solver_step(bad, x, x, x, x, w, mgs, umg, 25, out),                                  # non-positive size
        lambda: ops.cd_solver_step(null, x, x, x, x, w, mgs, umg, 25, out),                                 # null pointer
        lambda: ops.cd_solver_step(sched, x.double(), x.double(), x.double(), None, w, mgs, umg, 25, out),  # dtype code
        lambda: ops.cd_solver_step(sched, x, x, x, None, w, mgs, umg, 25, out.to(torch.int32)),             # dtype code
        lambda: ops.cd_loss_fwd(sched, x, x, x, x, 2, 0.001, mp, u, ws, loss),                              # unknown loss type
        lambda: ops.cd_loss_fwd(sched, x.half(), x, x, x, 0, 0.001, mp, u, ws, loss),                       # noise_pred fp16
        lambda: ops.cd_loss_fwd(sched, x, x, x, x, 0, 0.001, mp, u, ws[:1], loss),                          # workspace too small
        lambda: ops.cd_loss_fwd(bad, x, x, x, x, 0, 0.001, mp, u, ws, loss),
        lambda: ops.cd_loss_bwd(sched, x, None, None, d.half()),                                            # d_noise_pred fp16
        lambda: ops.cd_loss_bwd(null, x, None, None, d),
    ]
    for call in refused:
        with pytest.raises(nt.NativeError):
            call()
    lib, p = ops.lib, (lambda t: t.data_ptr())
    big = nt.CD_MAX_CLIPS + 1
    assert lib.t2v_cd_solver_step(nt.C.byref(sched), p(x), p(x), p(x), None, nt.F32, p(w), None, None, 25, p(out), nt.F32, big, 1, None) == -2
    assert lib.t2v_cd_loss_bwd(nt.C.byref(sched), p(x), None, None, p(d), nt.F32, big, 1, None) == -2
    assert lib.t2v_cd_loss_bwd(nt.C.byref(sched), p(x), None, None, p(d), nt.F32, B, 0, None) == -1
    torch.cuda.synchronize()
    for t in (out, mp, u, d, ws, loss):
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"
