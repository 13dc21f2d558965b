"""``optim.AdamW8bit`` on the device: ``t2v_adamw8_step`` against the CPU restatement (the criteria of
tests/test_hostsim_optim8.py), a large multi-tensor launch, state carried in 8 bits over consecutive steps, the module route of
full fine-tuning (train_latent_t2v_turbo_v2.py:798-845) and replay-safety."""
import copy
import warnings

import pytest
import torch

from t2v_turbo_amd.optim import QBLOCK, AdamW8bit
from tests.optim8_util import RTOL, build_case, compare_with_restatement, cpu_twin, random_state, table_gap
from tests.util import load, rel_l2

pytestmark = pytest.mark.gpu


def _check_steps(opt, steps, label, grad_scale=1.0, new_grads=None):
    """Every step on the device is compared with the restatement STARTED FROM THE DEVICE'S STATE before that step, so the 8-bit state
    is carried on the device from step to step and a tolerated one-code difference cannot compound into the next comparison."""
    total = off = 0
    for s in range(steps):
        if new_grads is not None and s > 0:
            new_grads(s)
        twin, pairs = cpu_twin(opt)
        opt.step(grad_scale=grad_scale)
        torch.cuda.synchronize()
        twin.step(grad_scale=grad_scale)
        t, o = compare_with_restatement(opt, pairs, twin, f"{label} step {s + 1}")
        total, off = total + t, off + o
    return total, off


@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_case_list_five_steps_against_the_restatement(grad_scale):
    opt, params = build_case("cuda")
    before = params["no_grad"].detach().clone()
    gen = torch.Generator().manual_seed(9)

    def new_grads(s):
        for n, p in params.items():
            if p.grad is not None:
                g = torch.randn(p.shape, generator=gen) * 0.3
                if n == "zero_block":
                    g[256:512] = 0
                p.grad.copy_(g.cuda())

    _check_steps(opt, 5, f"case list x{grad_scale}", grad_scale, new_grads)
    assert torch.equal(params["no_grad"].detach(), before) and opt.state[params["no_grad"]]["step"] == 3
    assert all(opt.state[p]["step"] == 8 for n, p in params.items() if n != "no_grad")
    assert all(torch.isfinite(p).all() for p in params.values())
    assert opt._table is not None and len(opt._table["launches"]) == 1   # one launch for both groups


def test_large_multi_tensor_launch():
    """96 tensors of mixed sizes (biases of 320 elements up to 4 M-element matrices, some with partial last blocks), 33 M elements,
    three groups — one with its own betas, hence a second launch — five steps."""
    gen = torch.Generator().manual_seed(4)
    sizes = [320, 1280, 4096, 5000, 77 * 1024 + 3, 640 * 640, 1280 * 1280 + 17, 1 << 20] * 11 + [1 << 22] * 2 + [(1 << 21) + 255] * 6
    assert len(sizes) >= 64 and sum(sizes) >= 32 * (1 << 20)
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.1).cuda()) for n in sizes]
    for p in params:
        p.grad = (torch.randn(p.numel(), generator=gen) * 0.01).cuda()
    opt = AdamW8bit([{"params": params[0::3]}, {"params": params[1::3], "lr": 1e-5, "weight_decay": 0.0},
                     {"params": params[2::3], "betas": (0.8, 0.95)}], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    random_state(opt, params[:40], gen)    # the rest starts from the zero state of a fresh optimizer (step 0)

    def new_grads(s):
        for p in params:
            p.grad.mul_(0.5 + 0.25 * s)

    total, off = _check_steps(opt, 5, "large", 1.0, new_grads)
    assert total >= 2 * 32 * (1 << 20) * 5 * 0.99
    assert len(opt._table["launches"]) >= 2


def test_table_goes_up_again_when_a_learning_rate_moves_into_the_same_device_table():
    """The descriptor table's way to the device (pinned, asynchronous, into the table that is there): five tensors on both sides of
    ``min_8bit_size`` in two groups, three steps, the second group's ``lr`` moved before step 2 and left alone before step 3.  Every
    step against the restatement by ``compare_with_restatement``'s bounds — a stale table would step with the old ``lr``, far outside
    them — and the dequantised moments with it: equal codes and bit-equal absmax give equal values, a code off by one at most one table
    gap times the block's absmax (plus 3 * 2**-24 of the absmax: the two values and the gap are one rounded fp32 product each, none
    larger than the absmax); the fp32 moments of the small tensors to fp32 rounding."""
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.1).cuda()) for n in (1, 255, 4096, 4097, 10561)]
    for p in params:
        p.grad = (torch.randn(p.numel(), generator=gen) * 0.3).cuda()
    opt = AdamW8bit([{"params": params[:3]}, {"params": params[3:], "lr": 3e-2}], lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    random_state(opt, params, gen)
    tables, images = [], []
    for s in range(3):
        if s == 1:
            opt.param_groups[1]["lr"] = 5e-3
        twin, pairs = cpu_twin(opt)
        opt.step()
        torch.cuda.synchronize()
        twin.step()
        compare_with_restatement(opt, pairs, twin, f"table upload step {s + 1}")
        for p, q in pairs:
            for k, (a, b) in enumerate(zip(opt.moments(p), twin.moments(q))):
                if "absmax1" in twin.state[q]:
                    absmax = twin.state[q][f"absmax{k + 1}"].repeat_interleave(QBLOCK)[:q.numel()]
                    gap = table_gap((twin.code1, twin.code2)[k]) + 3 * 2.0 ** -24
                    assert bool(((a.cpu() - b).abs() <= gap * absmax).all()), (s, p.numel(), k)
                else:
                    assert torch.allclose(a.cpu(), b, rtol=RTOL, atol=1e-12), (s, p.numel(), k)
        tables.append(opt._table["dev"].data_ptr())
        images.append(opt._table["uploaded"])
    assert len(set(tables)) == 1 and opt._table["dev"].is_cuda and opt._table["pinned"].is_pinned()
    assert images[0] != images[1] and images[1] is images[2]          # one upload for the moved lr, none for the step after
    assert bytes(opt._table["dev"].cpu().numpy().tobytes()) == images[2] and len(opt._table["launches"]) == 1


def test_same_step_twice_from_the_same_state_is_bit_identical():
    res = []
    for _ in range(2):
        opt, params = build_case("cuda", seed=3)
        opt.step(grad_scale=0.5)
        torch.cuda.synchronize()
        res.append(([p.detach().clone() for p in params.values()],
                    [v.clone() for p in params.values() for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]))
    assert all(torch.equal(a, b) for a, b in zip(res[0][0], res[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))


def test_full_fine_tuning_through_the_module_sees_the_update():
    """The v2 trainer's pattern with the drop-in class: every parameter of the UNet trainable (native full fine-tuning route, no
    composite-path RuntimeWarning), ``AdamW8bit`` over ``unet.parameters()`` in two groups (the second with its own lr), two forward /
    backward / step rounds.  The second forward must have seen the update: it is closer to the fp32 torch composite run with the NEW
    parameters than to the one with the OLD ones."""
    from t2v_turbo_amd.engine import params_fingerprint
    from tests.test_unet_full_grad_cpu import _student
    g = load("unet_tiny")
    m = _student().cuda()
    x, ts, ctx, tc = g["x"].cuda(), g["ts"].cuda(), g["ctx"].cuda(), g["tc"].cuda()
    r_out = torch.randn(g["y"].shape, generator=torch.Generator().manual_seed(3)).cuda()
    temporal = [p for n, p in m.named_parameters() if "temporal" in n or "temopral" in n]
    ids = {id(p) for p in temporal}
    others = [p for p in m.parameters() if id(p) not in ids]
    assert temporal and others
    opt = AdamW8bit([{"params": others}, {"params": temporal, "lr": 2e-3}], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)

    def reference(model):
        ref = copy.deepcopy(model).float()
        ref.native_mode = "off"
        with torch.no_grad():
            return ref(x, ts, context=ctx, fps=16, timestep_cond=tc).float()

    outs, refs, prints = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        assert m._auto_route(x.clone().requires_grad_(True), ctx, tc, None)[0] == "train_full"
        for rnd in range(2):
            refs.append(reference(m))
            prints.append(params_fingerprint(m))
            opt.zero_grad()
            y = m(x.clone().requires_grad_(True), ts, context=ctx, fps=16, timestep_cond=tc)
            (y.float() * r_out).sum().backward()
            outs.append(y.detach().float())
            assert all(p.grad is not None for p in m.parameters())
            opt.step()
    torch.cuda.synchronize()
    assert prints[0] != prints[1]
    e0, e_new, e_old = rel_l2(outs[0].cpu(), refs[0].cpu()), rel_l2(outs[1].cpu(), refs[1].cpu()), rel_l2(outs[1].cpu(), refs[0].cpu())
    moved = rel_l2(refs[1].cpu(), refs[0].cpu())
    print(f"round 1 vs its reference {e0:.3e}; round 2 vs NEW parameters {e_new:.3e}, vs OLD parameters {e_old:.3e}; the update moved "
          f"the reference by {moved:.3e}", flush=True)
    assert e0 < 3e-2 and e_new < 3e-2 and e_new < e_old and moved > 3 * e_new
    assert all(opt.state[p]["step"] == 2 for p in m.parameters())
