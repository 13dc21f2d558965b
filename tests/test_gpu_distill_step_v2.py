"""-m gpu: ``distill.distill_step_v2`` at the ``unet_tiny_mg_b2`` geometry (B = 2, ``motion_cond``) — three train-mode steps of full
fine-tuning with a frozen train-mode target, ``AdamW8bit`` and ``update_ema``, all on the native routes with the native head; and in
eval mode the native head against ``T2V_NATIVE_CD_HEAD=0`` at the seam (``noise_pred.grad``)."""
import copy
import os
import warnings

import pytest
import torch

from t2v_turbo_amd import cd_head, cd_math, optim
from t2v_turbo_amd import native as nt
from t2v_turbo_amd.distill import distill_step_v2
from t2v_turbo_amd.engine import UNetEngine
from t2v_turbo_amd.scheduler import T2VTurboScheduler
from tests import cd_head_cases as cc
from tests.util import load

pytestmark = pytest.mark.gpu

KW = dict(topk=20, motion_gs=0.8, percentage=0.5, use_motion_cond=True, fps=8, weight_dtype=torch.bfloat16)


def _setup(train):
    from tests.test_unet_full_grad_cpu import _student
    g = load("unet_tiny_mg_b2")
    student = _student("unet_tiny_mg_b2", motion_cond_proj_dim=256).cuda().requires_grad_(True)
    student.train(train)
    shape = tuple(g["x"].shape)
    gen = torch.Generator().manual_seed(3)
    c = torch.randn(shape, generator=gen)
    # the records are fp16 CPU tensors (latent_io); the step casts them to bf16 as the script does
    batch = {"index": torch.tensor([30, 49]), "z_t": g["x"].half(), "cond_teacher_out": c.half(),
             "uncond_teacher_out": (c + 0.3 * torch.randn(shape, generator=gen)).half(), "score": (0.2 * torch.randn(shape, generator=gen)).half(),
             "use_motion_guide": torch.tensor([True, False]), "prompt_emb": g["ctx"].half(), "txt": ["a", "b"]}
    sched = T2VTurboScheduler()
    return student, batch, sched, cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=50)


def test_three_train_mode_steps_on_the_native_routes_with_the_native_head():
    student, batch, sched, solver = _setup(train=True)
    target = copy.deepcopy(student).requires_grad_(False).train()
    opt = optim.AdamW8bit(student.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    want = [p.detach().clone() for p in target.parameters()]
    ops = nt.shared_ops()
    calls = {"cd_solver_step": 0, "cd_loss_fwd": 0, "cd_loss_bwd": 0}

    def counted(name):
        real = getattr(ops, name)

        def wrapper(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return wrapper

    for name in calls:
        setattr(ops, name, counted(name))
    losses = []
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)        # the composite UNet path must not be taken
            for step in range(3):
                loss, info = distill_step_v2(student, solver, sched, batch, target_unet=target, optimizer=opt, ema_decay=0.95,
                                             rng=dict(w=torch.tensor([6.0 + step, 11.5])), **KW)
                assert calls == {k: step + 1 for k in calls}, calls
                for w, s in zip(want, student.parameters()):
                    w.copy_(w * 0.95 + s.detach() * 0.05)
                losses.append(loss.detach())
                assert bool(torch.isfinite(loss)) and bool(torch.isfinite(info["x_prev"]).all()) and bool(torch.isfinite(info["grad_norm"]))
                assert info["x_prev"].dtype == torch.bfloat16 and type(loss.grad_fn).__name__ == "_ConsistencyLossBackward"
    finally:
        for name in calls:
            delattr(ops, name)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in student.parameters())
    eng = target._engine_box.engine
    # (the target's first forward records; the other two come after an update and refresh)
    assert type(eng) is UNetEngine and eng.counters == {"recorded": 1, "refreshed": 2} and len(eng.plans) == 1
    assert student._engine_box.full is not None and all(p.grad is None for p in student.parameters())
    assert float(losses[0]) != float(losses[2])
    for (name, p), w in zip(target.named_parameters(), want):
        assert torch.allclose(p, w, rtol=1e-6, atol=1e-7), name


def _seam_reference(solver, acp, info, batch, cdt):
    """The twin's d(loss)/d(noise_pred) in ``cdt`` from the tensors one run had at the seam."""
    npd = info["noise_pred"].detach().cpu().to(cdt).requires_grad_(True)
    loss, _ = cd_head.consistency_loss_torch(solver, acp, batch["index"], npd, info["target_noise_pred"].cpu().to(cdt),
                                             batch["z_t"].bfloat16().to(cdt), info["x_prev"].cpu().to(cdt), topk=20)
    loss.backward()
    return npd.grad


def test_native_head_and_the_torch_head_agree_at_the_seam_in_eval_mode():
    student, batch, sched, solver = _setup(train=False)
    acp = sched.alphas_cumprod
    grads = {}
    for native in ("1", "0"):
        os.environ["T2V_NATIVE_CD_HEAD"] = native
        try:
            loss, info = distill_step_v2(student, solver, sched, batch, rng=dict(w=torch.tensor([6.0, 11.5])), keep_noise_pred=True, **KW)
            assert (type(loss.grad_fn).__name__ == "_ConsistencyLossBackward") == (native == "1")
            loss.backward()
        finally:
            del os.environ["T2V_NATIVE_CD_HEAD"]
        torch.cuda.synchronize()
        got = info["noise_pred"].grad
        assert got is not None and bool(torch.isfinite(got).all())
        # each head against the float64 twin on ITS OWN seam tensors (the bf16 engines behind the seam are not the subject)
        cc.check_elementwise(f"noise_pred.grad (T2V_NATIVE_CD_HEAD={native})", got, _seam_reference(solver, acp, info, batch, torch.float64),
                             _seam_reference(solver, acp, info, batch, torch.float32))
        grads[native] = (got.detach().cpu(), info)
        for p in student.parameters():
            p.grad = None
    (g1, i1), (g0, i0) = grads["1"], grads["0"]
    if all(torch.equal(i1[k], i0[k]) for k in ("noise_pred", "target_noise_pred", "x_prev")):
        # the same seam tensors: the two heads then differ by at most the sum of their bounds
        ref64 = _seam_reference(solver, acp, i1, batch, torch.float64)
        E = cc.allowance(_seam_reference(solver, acp, i1, batch, torch.float32), ref64)
        assert float((g1.double() - g0.double()).abs().max()) <= 2 * E
