"""``optim.AdamW8bit`` (block-wise 8-bit AdamW) on the CPU: the ``bitsandbytes`` stand-in of ``compat.install()``, the code books, the
one-step identity with ``torch.optim.AdamW`` started from the dequantised moments, a training trajectory against fp32 AdamW,
checkpoints, schedulers and the parameter fingerprint the native engines re-pack on."""
import json
import os
import subprocess
import sys

import pytest
import torch

from t2v_turbo_amd.optim import AdamW8bit, QBLOCK, dequantize_blockwise, make_code_books, quantize_blockwise
from tests.optim8_util import build_case, table_gap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(torch.finfo(torch.float32).eps)


def test_bitsandbytes_import_resolves_to_the_native_class_and_the_v2_constructor_call_works():
    """train_latent_t2v_turbo_v2.py:787-795 and :833-845, verbatim in shape: import, class lookup, two groups (the second with its own
    lr), keyword hyper-parameters.  In a child process: the alias must not leak into this one."""
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import torch\n"
        "import t2v_turbo_amd.compat as c; c.install()\n"
        "import bitsandbytes as bnb\n"
        "import bitsandbytes.optim\n"
        "from t2v_turbo_amd.optim import AdamW8bit\n"
        "assert getattr(bnb, '__t2v_amd_alias__', False) and bnb.optim.AdamW8bit is AdamW8bit and bnb.optim.AdamW is torch.optim.AdamW\n"
        "optimizer_class = bnb.optim.AdamW8bit\n"
        "assert issubclass(optimizer_class, torch.optim.Optimizer)\n"
        "a, b = [torch.nn.Parameter(torch.randn(64, 128))], [torch.nn.Parameter(torch.randn(5000)), torch.nn.Parameter(torch.randn(8))]\n"
        "opt = optimizer_class([{'params': a}, {'params': b, 'lr': 1e-5}], lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)\n"
        "assert [g['lr'] for g in opt.param_groups] == [1e-4, 1e-5]\n"
        "for p in a + b: p.grad = torch.randn_like(p)\n"
        "opt.step(); opt.zero_grad()\n"
        "import io; f = io.BytesIO(); torch.save(opt.state_dict(), f)\n"
        "for kw in (dict(is_paged=True), dict(percentile_clipping=5), dict(block_wise=False), dict(optim_bits=8)):\n"
        "    try: optimizer_class(a, **kw)\n"
        "    except NotImplementedError: pass\n"
        "    else: raise AssertionError(kw)\n"
        "optimizer_class(a, percentile_clipping=100, optim_bits=32, is_paged=False, args=None, min_8bit_size=4096, block_wise=True)\n"
        "c.uninstall(); assert 'bitsandbytes' not in sys.modules and 'bitsandbytes.optim' not in sys.modules\n"
        "try: import bitsandbytes\n"
        "except ImportError: print('ok')\n") % (ROOT,)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_code_books_and_the_quantisation_error_bound():
    signed, unsigned = make_code_books()
    for code, lo in ((signed, -1.0), (unsigned, 0.0)):
        assert code.dtype == torch.float32 and code.numel() == 256 and bool((code[1:] > code[:-1]).all())
        assert float(code[0]) == lo and float(code[-1]) == 1.0 and bool((code == 0).any())
        gaps = code[1:] - code[:-1]
        zero = int((code == 0).nonzero()[0])
        assert float(gaps[zero]) < 1e-3 * float(gaps[-1])            # denser toward 0
        ident = torch.arange(256, dtype=torch.uint8).repeat(3)      # quantise o dequantise is the identity on codes
        vals = dequantize_blockwise(ident, torch.tensor([1.0, 0.37, 5e3]), code, 768)
        # (each block holds the code of +-1, so its absmax is the scale it was dequantised with)
        back, absmax = quantize_blockwise(vals, code)
        assert torch.equal(back, ident) and torch.allclose(absmax, torch.tensor([1.0, 0.37, 5e3]))
        g = table_gap(code)                                          # the largest adjacent gap, from the table itself
        gen = torch.Generator().manual_seed(0)
        for n in (256 * 40, 1000, 77):
            x = torch.randn(n, generator=gen) * torch.rand(n, generator=gen).mul(10).sub(8).exp()
            x = x if lo < 0 else x.abs()
            codes, absmax = quantize_blockwise(x, code)
            assert codes.numel() == (n + QBLOCK - 1) // QBLOCK * QBLOCK and bool((codes[n:] == zero).all())
            err = (dequantize_blockwise(codes, absmax, code, n) - x).abs()
            bound = absmax.repeat_interleave(QBLOCK)[:n] * (g / 2)
            assert bool((err <= bound).all()), float((err - bound).max())
    assert signed.numel() == 256 and bool((signed == -1).any())


@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_one_step_equals_torch_adamw_from_the_dequantised_moments(grad_scale):
    """Derivable, so no measured tolerance: the parameter after the step equals torch.optim.AdamW's step started from the DEQUANTISED
    moments to fp32 rounding, and the stored moments dequantise to the fp32 moments of that torch step within absmax * gap / 2 (plus
    the fp32 rounding of the reference moment itself, 4 eps * absmax: torch forms it as a lerp, this class as b m + (1 - b) g)."""
    opt, params = build_case()
    refs = {}
    for gi, grp in enumerate(opt.param_groups):
        for p in grp["params"]:
            if p.grad is None:
                continue
            m0, v0 = opt.moments(p)
            q = torch.nn.Parameter(p.detach().clone())
            q.grad = p.grad.detach().clone() * grad_scale
            ref = torch.optim.AdamW([q], lr=grp["lr"], betas=grp["betas"], eps=grp["eps"], weight_decay=grp["weight_decay"])
            ref.state[q] = dict(step=torch.tensor(float(opt.state[p]["step"])), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
            refs[p] = (q, ref)
    before = params["no_grad"].detach().clone()
    opt.step(grad_scale=grad_scale)
    assert torch.equal(params["no_grad"].detach(), before) and opt.state[params["no_grad"]]["step"] == 3
    g1, g2 = (table_gap(c) for c in make_code_books())
    for name, p in params.items():
        if p not in refs:
            continue
        q, ref = refs[p]
        ref.step()
        assert torch.allclose(p.detach(), q.detach(), rtol=1e-6, atol=1e-7), (name, float((p.detach() - q.detach()).abs().max()))
        assert opt.state[p]["step"] == 4 and torch.isfinite(p).all()
        m1, v1 = opt.moments(p)
        for got, want, gap in ((m1, ref.state[q]["exp_avg"], g1), (v1, ref.state[q]["exp_avg_sq"], g2)):
            n = p.numel()
            if p.numel() < opt.min_8bit_size:
                # fp32 state: only the rounding of the two evaluation orders, relative to the operands' magnitude
                assert float((got - want).abs().max()) <= 4 * EPS32 * float(want.abs().max()), name
                continue
            w = torch.zeros((n + QBLOCK - 1) // QBLOCK * QBLOCK)
            w[:n] = want.reshape(-1)
            absmax = w.view(-1, QBLOCK).abs().amax(dim=1).repeat_interleave(QBLOCK)[:n]
            err = (got.reshape(-1) - want.reshape(-1)).abs()
            assert bool((err <= absmax * (gap / 2 + 4 * EPS32)).all()), (name, float((err / absmax.clamp_min(1e-30)).max()))
    z = opt.state[params["zero_block"]]
    assert float(z["absmax1"][1]) == 0.0 and float(z["absmax2"][1]) == 0.0


def _tiny_problem(seed):
    from t2v_turbo_amd.unet3d import UNetModel
    from oracle.synth import synth_state_dict
    from tests.util import manifest, tiny_unet_params
    m = UNetModel(**tiny_unet_params())
    m.load_state_dict(synth_state_dict(manifest("unet_tiny")), strict=True)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for p in m.parameters():
            if float(p.abs().max()) == 0:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    m.requires_grad_(True)
    m.eval()
    m.native_mode = "off"
    gen = torch.Generator().manual_seed(100)
    data = [(torch.randn(1, 4, 2, 8, 8, generator=gen), torch.randint(0, 1000, (1,), generator=gen), torch.randn(1, 77, 128, generator=gen),
             torch.randn(1, 4, 2, 8, 8, generator=gen) * 0.5) for _ in range(8)]
    return m, data, torch.Generator().manual_seed(seed)


def _train(opt_cls, seed, steps=50):
    """A fixed synthetic regression (8 samples: latents, timestep, text -> target), one sample per step in a seed-dependent order; the
    loss reported is the mean over all 8 samples after training."""
    m, data, order = _tiny_problem(seed)
    opt = opt_cls(m.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)

    def loss_of(sample):
        x, ts, ctx, target = sample
        return ((m(x, ts, context=ctx, fps=16) - target) ** 2).mean()

    with torch.no_grad():
        first = float(sum(loss_of(s) for s in data) / len(data))
    for _ in range(steps):
        opt.zero_grad()
        loss_of(data[int(torch.randint(0, len(data), (1,), generator=order))]).backward()
        opt.step()
    with torch.no_grad():
        return first, float(sum(loss_of(s) for s in data) / len(data))


TRAJECTORY_MARGIN = 1.0   # the fp32 runs' own spread (max - min over data orders) is widened by this many spreads on either side


def test_trajectory_lies_within_the_spread_of_fp32_adamw():
    """The yardstick the reference itself offers: torch.optim.AdamW, the other arm of the same ``if``.  The tiny UNet (torch composite
    path) is trained for 50 steps once with AdamW8bit and four times with fp32 AdamW under different data-order seeds; the 8-bit
    run's final loss must lie within [min - margin * spread, max + margin * spread] of the fp32 runs performed HERE (the bound is not
    a constant tuned on the 8-bit run), and training must have reduced the loss.  Recorded numbers:
    profiles/r07_adamw8_vs_fp32_trajectory.json."""
    fp32 = [_train(torch.optim.AdamW, seed) for seed in (1, 2, 3, 4)]
    first, last8 = _train(AdamW8bit, 1)
    finals = [b for _, b in fp32]
    lo, hi = min(finals), max(finals)
    spread = hi - lo
    print(json.dumps(dict(initial_loss=first, fp32_final=finals, adamw8_final=last8, spread=spread, margin=TRAJECTORY_MARGIN)), flush=True)
    assert spread > 0 and last8 < first and all(b < first for b in finals)
    assert lo - TRAJECTORY_MARGIN * spread <= last8 <= hi + TRAJECTORY_MARGIN * spread, (last8, lo, hi)


def test_state_dict_round_trip_continues_bit_identically_and_lambda_lr_drives_the_step():
    def make():
        gen = torch.Generator().manual_seed(2)
        ps = [torch.nn.Parameter(torch.randn(5000, generator=gen)), torch.nn.Parameter(torch.randn(33, generator=gen)),
              torch.nn.Parameter(torch.randn(32, 256, generator=gen))]
        opt = AdamW8bit([{"params": ps[:2]}, {"params": ps[2:], "lr": 1e-2}], lr=1e-3, weight_decay=0.05)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 / (1 + s))
        return ps, opt, sched

    def run(ps, opt, sched, first, count):
        for s in range(first, first + count):
            gen = torch.Generator().manual_seed(50 + s)
            for p in ps:
                p.grad = torch.randn(p.shape, generator=gen)
            opt.step()
            sched.step()

    ps, opt, sched = make()
    run(ps, opt, sched, 0, 3)
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-3 / 4) and opt.param_groups[1]["lr"] == pytest.approx(1e-2 / 4)
    import io
    f = io.BytesIO()
    torch.save(dict(opt=opt.state_dict(), sched=sched.state_dict(), params=[p.detach().clone() for p in ps]), f)
    assert f.getbuffer().nbytes < 4 * sum(p.numel() for p in ps) * 2     # codes, not fp32 moments (and no arena per tensor)
    run(ps, opt, sched, 3, 3)
    f.seek(0)
    ck = torch.load(f, weights_only=False)
    ps2, opt2, sched2 = make()
    with torch.no_grad():
        for p, v in zip(ps2, ck["params"]):
            p.copy_(v)
    opt2.load_state_dict(ck["opt"])
    sched2.load_state_dict(ck["sched"])
    assert [opt2.state[p]["step"] for p in ps2] == [3, 3, 3] and opt2.param_groups[1]["lr"] == pytest.approx(1e-2 / 4)
    run(ps2, opt2, sched2, 3, 3)
    for a, b in zip(ps, ps2):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(ps, ps2):
        for k, v in opt.state[a].items():
            assert torch.equal(v, opt2.state[b][k]) if torch.is_tensor(v) else v == opt2.state[b][k]
    # the scheduler's lr reaches the arithmetic: a step with lr = 0 and no decay leaves the parameters alone
    for g in opt.param_groups:
        g["lr"] = 0.0
    before = [p.detach().clone() for p in ps]
    opt.step()
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, ps))


def test_loading_a_torch_adamw_state_quantises_its_moments_and_add_param_group_keeps_state():
    gen = torch.Generator().manual_seed(6)
    ps = [torch.nn.Parameter(torch.randn(6000, generator=gen)), torch.nn.Parameter(torch.randn(50, generator=gen))]
    ref = torch.optim.AdamW(ps, lr=1e-3, betas=(0.9, 0.99), weight_decay=0.0)
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
        ref.step()
    opt = AdamW8bit(ps, lr=5e-4)
    opt.load_state_dict(ref.state_dict())
    assert opt.param_groups[0]["betas"] == (0.9, 0.99) and opt.param_groups[0]["lr"] == 1e-3 and opt.state[ps[0]]["step"] == 3
    g1, g2 = (table_gap(c) for c in make_code_books())
    m, v = opt.moments(ps[0])
    assert float((m - ref.state[ps[0]]["exp_avg"]).abs().max()) <= float(ref.state[ps[0]]["exp_avg"].abs().max()) * g1 / 2
    assert float((v - ref.state[ps[0]]["exp_avg_sq"]).abs().max()) <= float(ref.state[ps[0]]["exp_avg_sq"].abs().max()) * g2 / 2
    m, v = opt.moments(ps[1])                                      # below min_8bit_size: kept in fp32
    assert torch.equal(m, ref.state[ps[1]]["exp_avg"]) and torch.equal(v, ref.state[ps[1]]["exp_avg_sq"])
    kept = [t.clone() for t in (opt.state[ps[0]]["state1"], opt.state[ps[0]]["absmax2"], opt.state[ps[1]]["state2"])]
    extra = torch.nn.Parameter(torch.randn(4096, generator=gen))
    opt.add_param_group({"params": [extra], "lr": 1e-2})
    for p in ps + [extra]:
        p.grad = torch.zeros_like(p)
    for g in opt.param_groups:
        g["lr"], g["weight_decay"] = 0.0, 0.0
    opt._ensure_state()
    now = (opt.state[ps[0]]["state1"], opt.state[ps[0]]["absmax2"], opt.state[ps[1]]["state2"])
    assert all(torch.equal(a, b) for a, b in zip(kept, now)) and opt.state[extra]["step"] == 0
    opt.step()
    assert opt.state[extra]["step"] == 1 and opt.state[ps[0]]["step"] == 4


def test_params_fingerprint_moves_across_a_step():
    from t2v_turbo_amd.engine import params_fingerprint
    lin = torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.Linear(128, 8))
    opt = AdamW8bit(lin.parameters(), lr=1e-3)
    lin(torch.randn(4, 64)).sum().backward()
    before = params_fingerprint(lin)
    opt.step()
    assert params_fingerprint(lin) != before
