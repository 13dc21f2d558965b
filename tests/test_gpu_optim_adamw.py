"""``optim.AdamW`` / ``optim.clip_grad_norm_`` / ``optim.grad_clip_coef`` on the device: ``t2v_adamw_multi``, ``t2v_sumsq_multi`` and
``t2v_scale_multi`` on the shared case table (the criteria of tests/test_hostsim_adamw.py), a launch large enough for the grid stride,
table reuse, the two ways to clip, and the trainers' patterns through the module (train_latent_t2v_turbo_v2.py:787-845,1265-1268)."""
import copy
import warnings

import pytest
import torch

from t2v_turbo_amd import native as nt
from t2v_turbo_amd import optim
from t2v_turbo_amd.native import shared_ops
from t2v_turbo_amd.optim import AdamW, clip_grad_norm_, grad_clip_coef
from tests.adamw_cases import (B, NO_GRAD, RTOL, ATOL, AdamwCase, bits, check_against_adamw8, check_twin, many_groups, norm_bound,
                               twin_step)
from tests.util import load, rel_l2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("host_scale, dev_scale", [(1.0, None), (0.37, None), (0.5, 0.74)])
def test_case_list_one_launch_against_adamw8_and_the_definition(host_scale, dev_scale):
    """The kernel called directly over the case table: bit-identical to the fp32-state branch of ``t2v_adamw8_step``, moments
    bit-equal to the torch definition, parameters within fp32 rounding, guards and gradients bit-unchanged."""
    ops = shared_ops()
    case = AdamwCase("cuda")
    snap = case.snapshot()
    table, n, work, hyper, order = case.table()
    scale_dev = None if dev_scale is None else torch.tensor([dev_scale], device="cuda")
    ops.adamw_multi(table, n, work, hyper, host_scale, scale_dev)
    torch.cuda.synchronize()
    total = float(torch.tensor(host_scale) * torch.tensor(1.0 if dev_scale is None else dev_scale))
    check_against_adamw8(ops, case, snap, total)
    case.check_guards(grads_equal_to=snap)
    assert case.no_grad_unchanged(snap, 3)
    case.check_against_definition(snap, total, label=f"device x{total}")


def test_case_list_five_optimizer_steps_with_new_gradients():
    case = AdamwCase("cuda", seed=7)
    for s in range(5):
        snap = case.snapshot()
        steps = {i: int(case.opt.state[case.params[i]]["step"]) + 1 for i in case.active}
        case.opt.step()
        torch.cuda.synchronize()
        case.check_against_definition(snap, 1.0, steps=steps, label=f"step {s + 1}")
        case.check_guards(grads_equal_to=snap)
        assert case.no_grad_unchanged(snap, 3)
        case.new_grads()
    assert len(case.opt._plan["launches"]) == 1 and case.opt.table_uploads == 1
    assert [int(case.opt.state[p]["step"]) for p in case.params[:3]] == [8, 8, 11]
    assert all(p._version > 0 for i, p in enumerate(case.params) if i != NO_GRAD)


def test_more_than_16_hyper_rows_take_a_second_launch():
    opt, params = many_groups("cuda")
    for s in range(2):
        want = twin_step(opt)
        opt.step()
        torch.cuda.synchronize()
        check_twin(opt, want, f"17 groups step {s + 1}")
    assert [(e - s, rows) for s, e, _, _, rows in opt._plan["launches"]] == [(16, 16), (1, 1)]


def test_sumsq_and_scale_on_the_case_table():
    ops = shared_ops()
    case = AdamwCase("cuda", seed=8)
    table, n, work, _, order = case.table()
    want = sum(float((case.tensors(i)[1].double() ** 2).sum()) for i in order)
    for max_norm, clips in ((0.25 * want ** 0.5, True), (4.0 * want ** 0.5, False)):
        snap = case.snapshot()
        outs = []
        for _ in range(2):
            ws, out = torch.full((work + 3,), 7.0, device="cuda"), torch.full((3,), 7.0, device="cuda")
            ops.sumsq_multi(table, n, work, ws, max_norm, out)
            outs.append((ws, out))
        torch.cuda.synchronize()
        assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))   # deterministic
        ws, out = outs[0]
        assert bool(torch.isfinite(out).all()) and bool((ws[work:] == 7.0).all()) and float(out[2]) == 7.0           # no guard was read
        err = abs(float(out[0].double() ** 2) - want) / want
        print(f"sum of squares: relative error {err:.3e}, bound {norm_bound():.3e}", flush=True)
        assert err <= norm_bound()
        coef = torch.clamp(max_norm / (out[0] + 1e-6), max=1.0)
        assert abs(float(out[1]) - float(coef)) <= 2 * float(torch.nextafter(coef, coef + 1) - coef)
        assert (float(out[1]) < 1.0) == clips
        ops.scale_multi(table, n, work, out[1:])
        torch.cuda.synchronize()
        if clips:
            for i in order:
                assert torch.equal(bits(case.tensors(i)[1]), bits(case._span(snap, "g", i) * out[1]))
            case.check_guards()
        else:
            case.check_guards(grads_equal_to=snap)
        for k in "pmv":
            assert torch.equal(bits(case.arena[k]), bits(snap[k]))
        case.restore(snap)   # (the next round's norm is of the unscaled gradients again)


def _large(gen):
    sizes = [320, 1280, 4096, 5000, 77 * 1024 + 3, 640 * 640, 1280 * 1280 + 17, 1 << 20] * 3 + [(1 << 21) + 255] * 4
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.1).cuda()) for n in sizes]
    for p in params:
        p.grad = (torch.randn(p.numel(), generator=gen) * 0.3).cuda()
    return params, sum((n + B - 1) // B for n in sizes)


def test_large_launch_exercises_the_grid_stride():
    """28 tensors from 320 elements to (1 << 21) + 255, 18 M elements: more than twice as many work blocks as the persistent grid has
    workgroups (2048), so every workgroup takes at least two.  Three groups, five steps, each checked against the definition started
    from the device's state."""
    gen = torch.Generator().manual_seed(4)
    params, work = _large(gen)
    assert work >= 2 * 2048
    opt = AdamW([{"params": params[0::3]}, {"params": params[1::3], "lr": 1e-5, "weight_decay": 0.0},
                 {"params": params[2::3], "betas": (0.8, 0.95), "eps": 1e-6, "lr": 2e-3}], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for s in range(5):
        want = twin_step(opt)
        opt.step()
        torch.cuda.synchronize()
        check_twin(opt, want, f"large step {s + 1}")
        for p in params:
            p.grad.mul_(0.5 + 0.25 * s)
    (start, end, launch_work, row0, rows), = opt._plan["launches"]
    assert (end - start, launch_work, rows) == (len(params), work, 3) and opt.table_uploads == 1


def test_table_reuse():
    """The same step twice from the same state is bit-identical; ``zero_grad(set_to_none=True)`` and fresh gradients re-make the table
    and the result still matches; unchanged pointers with a changed lr upload nothing."""
    res = []
    for _ in range(2):
        case = AdamwCase("cuda", seed=3)
        case.opt.step(grad_scale=0.5)
        torch.cuda.synchronize()
        res.append({k: a.clone() for k, a in case.arena.items()})
    assert all(torch.equal(bits(res[0][k]), bits(res[1][k])) for k in "pgmv")

    gen = torch.Generator().manual_seed(12)
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.1).cuda()) for n in (7, 4097, 3 * B + 5)]
    opt = AdamW(params, lr=1e-3)

    def fresh_grads():
        for p in params:
            p.grad = (torch.randn(p.numel(), generator=gen) * 0.3).cuda()

    fresh_grads()
    for s, lr in enumerate((1e-3, 5e-4, 2.5e-4)):   # a moving lr, the same pointers
        opt.param_groups[0]["lr"] = lr
        want = twin_step(opt)
        opt.step()
        torch.cuda.synchronize()
        check_twin(opt, want, f"lr {lr}")
        assert opt.table_uploads == 1
    held = [p.grad for p in params]                 # (kept alive: the new gradients cannot land on the old addresses)
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in params)
    fresh_grads()
    want = twin_step(opt)
    opt.step()
    torch.cuda.synchronize()
    check_twin(opt, want, "after zero_grad(set_to_none=True)")
    assert opt.table_uploads == 2 and len(held) == 3


def test_clip_then_step_against_coefficient_folded_into_the_step():
    """``clip_grad_norm_`` then ``step()`` against ``grad_clip_coef`` then ``step(grad_scale=coef)`` from the same state: g * coef is
    rounded once either way, so the moments are bit-equal; the parameters within fp32 rounding; the norm within the derived bound."""
    gen = torch.Generator().manual_seed(21)
    sizes = (5, 257, 4097, 3 * B + 5, 640 * 640)
    base = [torch.randn(n, generator=gen) * 0.1 for n in sizes]
    grads = [torch.randn(n, generator=gen) * 0.3 for n in sizes]
    norm64 = sum(float((g.double() ** 2).sum()) for g in grads) ** 0.5
    runs = []
    for folded in (False, True):
        params = [torch.nn.Parameter(b.clone().cuda()) for b in base]
        for p, g in zip(params, grads):
            p.grad = g.clone().cuda()
        opt = AdamW([{"params": params[:2]}, {"params": params[2:], "lr": 2e-3}], lr=1e-3)
        for _ in range(2):                      # the second step starts from non-zero moments
            if folded:
                norm, coef = grad_clip_coef(params, 1.0)
                assert norm.dim() == 0 and coef.dim() == 0 and norm.is_cuda and norm.untyped_storage().data_ptr() == coef.untyped_storage().data_ptr()
                opt.step(grad_scale=coef)
                assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(params, grads))   # the gradients are never written
            else:
                norm = clip_grad_norm_(params, 1.0)
                assert norm.dim() == 0 and norm.is_cuda and norm.dtype == torch.float32
                opt.step()
                for p, g in zip(params, grads):
                    p.grad.copy_(g)
            torch.cuda.synchronize()
            assert abs(float(norm) - norm64) / norm64 <= norm_bound() and float(norm) > 1.0   # (it clips)
        runs.append((params, opt))
    (pa, oa), (pb, ob) = runs
    for a, b in zip(pa, pb):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(bits(oa.state[a][k]), bits(ob.state[b][k])), k
        assert torch.allclose(a, b, rtol=RTOL, atol=ATOL)
    # the drop-in against torch's function on the same gradients
    twins = [torch.nn.Parameter(b.clone().cuda()) for b in base]
    for p, q, g in zip(pa, twins, grads):
        p.grad.copy_(g)
        q.grad = g.clone().cuda()
    n_ours, n_torch = clip_grad_norm_(pa, 1.0), torch.nn.utils.clip_grad_norm_(twins, 1.0)
    assert abs(float(n_ours) - float(n_torch)) <= 2 * norm_bound() * norm64
    for p, q in zip(pa, twins):
        assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=0)
    with pytest.raises(RuntimeError, match="non-finite"):
        pa[1].grad[3] = float("nan")
        clip_grad_norm_(pa, 1.0, error_if_nonfinite=True)


def _module_rounds(m, opt, clip, x, ts, ctx, tc, r_out, route, params):
    """Two forward / backward / clip / step rounds through the module.  The second forward must have seen the update: it is closer to
    the fp32 torch composite run with the NEW parameters than to the one with the OLD ones (the assertions of
    tests/test_gpu_optim8.py::test_full_fine_tuning_through_the_module_sees_the_update)."""
    from t2v_turbo_amd.engine import params_fingerprint

    def reference(model):
        ref = copy.deepcopy(model).float()
        ref.native_mode = "off"
        with torch.no_grad():
            return ref(x, ts, context=ctx, fps=16, timestep_cond=tc).float()

    outs, refs, prints = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        assert m._auto_route(x.clone().requires_grad_(True), ctx, tc, None)[0] == route
        for rnd in range(2):
            refs.append(reference(m))
            prints.append(params_fingerprint(m))
            opt.zero_grad()
            y = m(x.clone().requires_grad_(True), ts, context=ctx, fps=16, timestep_cond=tc)
            (y.float() * r_out).sum().backward()
            outs.append(y.detach().float())
            assert all(p.grad is not None for p in params)
            if clip is not None:
                norm = clip_grad_norm_(m.parameters(), clip)
                assert norm.is_cuda and bool(torch.isfinite(norm)) and optim._CLIP_PLANS   # (the native path took it)
            opt.step()
    torch.cuda.synchronize()
    assert prints[0] != prints[1]
    e0, e_new, e_old = rel_l2(outs[0].cpu(), refs[0].cpu()), rel_l2(outs[1].cpu(), refs[1].cpu()), rel_l2(outs[1].cpu(), refs[0].cpu())
    moved = rel_l2(refs[1].cpu(), refs[0].cpu())
    print(f"round 1 vs its reference {e0:.3e}; round 2 vs NEW parameters {e_new:.3e}, vs OLD parameters {e_old:.3e}; the update moved "
          f"the reference by {moved:.3e}", flush=True)
    assert e0 < 3e-2 and e_new < 3e-2 and e_new < e_old and moved > 3 * e_new
    assert all(float(opt.state[p]["step"]) == 2 for p in params)


def test_full_fine_tuning_through_the_module_sees_the_update():
    """The v2 trainer's pattern on the default command line: every parameter of the UNet trainable (native full fine-tuning route),
    ``optim.AdamW`` over ``unet.parameters()`` in two groups (the second with its own lr), ``optim.clip_grad_norm_(.., 1.0)``."""
    from tests.test_unet_full_grad_cpu import _student
    g = load("unet_tiny")
    m = _student().cuda()
    x, ts, ctx, tc = g["x"].cuda(), g["ts"].cuda(), g["ctx"].cuda(), g["tc"].cuda()
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3)).cuda()
    temporal = [p for n, p in m.named_parameters() if "temporal" in n or "temopral" in n]
    ids = {id(p) for p in temporal}
    others = [p for p in m.parameters() if id(p) not in ids]
    assert temporal and others
    opt = AdamW([{"params": others}, {"params": temporal, "lr": 2e-3}], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    _module_rounds(m, opt, 1.0, x, ts, ctx, tc, r_out, "train_full", list(m.parameters()))


def test_lora_student_on_the_train_route_sees_the_update():
    """The v1 trainer's pattern: a LoRA-injected student on the LoRA training route, ``optim.AdamW(lora.lora_parameters(m))``."""
    from t2v_turbo_amd import lora
    from tests.test_unet_lora_grad_cpu import _student
    g = load("unet_tiny")
    m, _ = _student("unet_tiny", 64)
    m = m.cuda()
    params = lora.lora_parameters(m)
    x, ts, ctx, tc = g["x"].cuda(), g["ts"].cuda(), g["ctx"].cuda(), g["tc"].cuda()
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3)).cuda()
    _module_rounds(m, AdamW(params), None, x, ts, ctx, tc, r_out, "train", params)


def test_malformed_calls_are_refused_on_the_device_build():
    case = AdamwCase("cuda", seed=11)
    snap = case.snapshot()
    table, n, work, hyper, order = case.table()
    lib = nt.load()
    rows = (nt.AdamwHyper * 3)(*[nt.AdamwHyper(*h) for h in hyper])
    hp = nt.C.cast(rows, nt.C.c_void_p)
    t = table.data_ptr()
    for args in ((None, n, work, hp, 3), (t, n, work, None, 3), (t, 0, work, hp, 3), (t, n, n - 1, hp, 3), (t, n, work, hp, 0), (t, n, work, hp, 17)):
        assert lib.t2v_adamw_multi(*args, 1.0, None, None) == -1, args
    assert lib.t2v_adamw_multi(t + 4, n, work, hp, 3, 1.0, None, None) == -2
    torch.cuda.synchronize()
    for k in "pgmv":
        assert torch.equal(bits(case.arena[k]), bits(snap[k]))
