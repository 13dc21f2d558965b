"""``optim.AdamW`` / ``optim.clip_grad_norm_`` without a GPU and without the library: the constructor surface of ``torch.optim.AdamW``,
checkpoints in both directions, schedulers, parameter groups added later, parameters that skip a step, the closure, version counters."""
import copy

import pytest
import torch

from t2v_turbo_amd.optim import AdamW, clip_grad_norm_, grad_clip_coef

RTOL, ATOL = 1e-6, 1e-7          # fp32 rounding: the constants of tests/optim8_util.py
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def _params(seed=0, sizes=((5,), (4097,), (3, 7))):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=gen) * 0.1) for s in sizes], gen


def _grads(params, gen):
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen) * 0.3


def test_the_v2_two_group_call():
    """train_latent_t2v_turbo_v2.py:833-845: two groups, the second with its own lr; foreach / fused accepted and ignored."""
    params, gen = _params()
    for kw in ({}, dict(foreach=True), dict(fused=True), dict(foreach=False, fused=False)):
        opt = AdamW([{"params": params[:2]}, {"params": params[2:], "lr": 2e-5}], lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, **kw)
        assert isinstance(opt, torch.optim.Optimizer) and [g["lr"] for g in opt.param_groups] == [1e-5, 2e-5]
        _grads(params, gen)
        opt.step()
        assert all(float(opt.state[p]["step"]) == 1 and opt.state[p]["step"].device.type == "cpu" for p in params)
        assert set(opt.state[params[0]]) == {"step", "exp_avg", "exp_avg_sq"} and opt.state[params[0]]["step"].dtype == torch.float32
    opt = AdamW(params, lr=torch.tensor(1e-3))   # a 0-d tensor lr
    opt.step()


@pytest.mark.parametrize("flag", ["amsgrad", "maximize", "capturable", "differentiable"])
def test_refused_flags_raise(flag):
    params, _ = _params()
    with pytest.raises(NotImplementedError):
        AdamW(params, **{flag: True})
    opt = AdamW(params[:1])
    with pytest.raises(NotImplementedError):
        opt.add_param_group({"params": params[1:], flag: True})


def test_non_contiguous_or_bf16_parameters_raise_at_step():
    base = torch.randn(6, 8)
    p = torch.nn.Parameter(base.t())
    assert not p.is_contiguous()
    p.grad = torch.randn(8, 6)
    with pytest.raises(ValueError):
        AdamW([p]).step()
    q = torch.nn.Parameter(torch.randn(9).bfloat16())
    q.grad = torch.randn(9).bfloat16()
    with pytest.raises(ValueError):
        AdamW([q]).step()
    r = torch.nn.Parameter(torch.randn(6, 8))
    r.grad = torch.randn(8, 6).t()
    with pytest.raises(ValueError):
        AdamW([r]).step()


def _compare(a, b, label):
    """Both optimizers' parameters and moments after a step from the same state."""
    for (pa, pb) in zip(a.param_groups[0]["params"], b.param_groups[0]["params"]):
        assert torch.allclose(pa, pb, rtol=RTOL, atol=ATOL), (label, "p", float((pa - pb).abs().max()))
        for k in ("exp_avg", "exp_avg_sq"):
            x, y = a.state[pa][k], b.state[pb][k]
            assert torch.allclose(x, y, rtol=RTOL, atol=ATOL), (label, k, float((x - y).abs().max()))
        assert float(a.state[pa]["step"]) == float(b.state[pb]["step"])


def test_state_dict_round_trips_with_torch_in_both_directions():
    """Seed 0, three tensors, eight steps against ``torch.optim.AdamW(foreach=False)``; every step starts from the same state (each
    side is re-loaded from the other's checkpoint, in alternating directions), so nothing compounds."""
    ours_p, gen = _params(0)
    torch_p = [torch.nn.Parameter(p.detach().clone()) for p in ours_p]
    ours, ref = AdamW(ours_p, **HYPER), torch.optim.AdamW(torch_p, foreach=False, **HYPER)
    for s in range(8):
        _grads(ours_p, gen)
        for p, q in zip(ours_p, torch_p):
            q.grad = p.grad.clone()
        ours.step()
        ref.step()
        _compare(ours, ref, f"step {s + 1}")
        sd = copy.deepcopy(ref.state_dict() if s % 2 == 0 else ours.state_dict())   # torch -> ours, then ours -> torch, ...
        assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
        if s % 2 == 0:
            ours.load_state_dict(sd)
            for p, q in zip(ours_p, torch_p):
                p.data.copy_(q.data)
        else:
            ref.load_state_dict(sd)
            for p, q in zip(ours_p, torch_p):
                q.data.copy_(p.data)
        for p, q in zip(ours_p, torch_p):
            for k in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(ours.state[p][k], ref.state[q][k])
        assert ours.state[ours_p[0]]["step"].device.type == "cpu" and float(ours.state[ours_p[0]]["step"]) == s + 1


def test_a_step_tensor_saved_on_another_device_form_comes_to_the_host_at_load():
    """A ``fused=True`` checkpoint keeps ``step`` with the parameter; a plain number is also taken."""
    params, gen = _params(1)
    _grads(params, gen)
    ref = torch.optim.AdamW(params, **HYPER)
    ref.step()
    sd = ref.state_dict()
    for g in sd["param_groups"]:
        g["fused"] = True
    sd["state"][1]["step"] = 1
    opt = AdamW(params, **HYPER)
    opt.load_state_dict(sd)
    assert all(torch.is_tensor(opt.state[p]["step"]) and opt.state[p]["step"].device.type == "cpu" and opt.state[p]["step"].dim() == 0
               and float(opt.state[p]["step"]) == 1 for p in params)
    opt.step()
    assert all(float(opt.state[p]["step"]) == 2 for p in params)


def test_an_lr_scheduler_drives_lr():
    params, gen = _params(2)
    ours_p = params
    torch_p = [torch.nn.Parameter(p.detach().clone()) for p in ours_p]
    ours, ref = AdamW(ours_p, **HYPER), torch.optim.AdamW(torch_p, foreach=False, **HYPER)
    scheds = [torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5) for o in (ours, ref)]
    for s in range(3):
        _grads(ours_p, gen)
        for p, q in zip(ours_p, torch_p):
            q.grad = p.grad.clone()
            q.data.copy_(p.data)
            for k in ("exp_avg", "exp_avg_sq"):
                if k in ours.state[p]:
                    ref.state[q][k].copy_(ours.state[p][k])
        ours.step()
        ref.step()
        for sc in scheds:
            sc.step()
        _compare(ours, ref, f"scheduled step {s + 1}")
    assert ours.param_groups[0]["lr"] == pytest.approx(1e-3 * 0.125)


def test_add_param_group_and_a_parameter_that_skips_a_step():
    params, gen = _params(3)
    opt = AdamW(params[:2], **HYPER)
    _grads(params[:2], gen)
    opt.step()
    opt.add_param_group({"params": params[2:], "lr": 5e-4})
    _grads(params, gen)
    params[0].grad = None            # no gradient this step: nothing of it moves, its step count stays
    before = params[0].detach().clone()
    opt.step()
    assert torch.equal(params[0].detach(), before)
    assert [float(opt.state[p]["step"]) for p in params] == [1, 2, 1]
    _grads(params, gen)
    want = []
    for p, g in ((params[0], opt.param_groups[0]), (params[1], opt.param_groups[0]), (params[2], opt.param_groups[1])):
        q = torch.nn.Parameter(p.detach().clone())
        q.grad = p.grad.clone()
        ref = torch.optim.AdamW([q], foreach=False, **{**HYPER, "lr": g["lr"]})
        ref.state[q] = {k: v.clone() for k, v in opt.state[p].items()}
        ref.step()
        want.append(q)
    opt.step()                       # three tensors, three (group, step) combinations: its own bias correction each
    assert [float(opt.state[p]["step"]) for p in params] == [2, 3, 2]
    for p, q in zip(params, want):
        assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), float((p - q).abs().max())


def test_the_closure_is_honoured_and_version_counters_move():
    params, gen = _params(4)
    opt = AdamW(params, **HYPER)
    calls = []

    def closure():
        calls.append(torch.is_grad_enabled())
        loss = sum((p ** 2).sum() for p in params)
        opt.zero_grad()
        loss.backward()
        return loss

    versions = [p._version for p in params]
    loss = opt.step(closure)
    assert calls == [True] and float(loss.detach()) > 0
    assert all(p._version > v for p, v in zip(params, versions))
    assert all(float(opt.state[p]["step"]) == 1 for p in params)
    assert opt.step() is None


def test_clip_grad_norm_on_cpu_tensors_is_torchs_function():
    params, gen = _params(5)
    for norm_type in (2.0, 1.0, float("inf")):
        _grads(params, gen)
        twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for p, q in zip(params, twins):
            q.grad = p.grad.clone()
        a = clip_grad_norm_(params, 0.5, norm_type=norm_type)
        b = torch.nn.utils.clip_grad_norm_(twins, 0.5, norm_type=norm_type)
        assert torch.equal(a, b) and all(torch.equal(p.grad, q.grad) for p, q in zip(params, twins))
    assert torch.equal(clip_grad_norm_(params[0], 0.5), torch.nn.utils.clip_grad_norm_(twins[0], 0.5))   # a single tensor
    params[0].grad[0] = float("inf")
    with pytest.raises(RuntimeError):
        clip_grad_norm_(params, 1.0, error_if_nonfinite=True)
    assert float(clip_grad_norm_((p for p in params[1:]), 1e9)) > 0                                       # a generator
    norm, coef = grad_clip_coef(params[1:], 0.5)
    want = torch.nn.utils.get_total_norm([p.grad for p in params[1:]], 2.0)
    assert torch.equal(norm, want) and torch.equal(coef, torch.clamp(0.5 / (want + 1e-6), max=1.0))
