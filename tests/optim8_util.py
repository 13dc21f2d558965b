"""Shared by the AdamW8bit tests (CPU, host simulator, GPU): the case list of the one-step checks and the comparison of a kernel
run with the CPU restatement (``AdamW8bit._step_cpu``)."""
import copy

import torch

from t2v_turbo_amd.optim import AdamW8bit, QBLOCK

RTOL, ATOL = 1e-6, 1e-7          # fp32 rounding, as tests/test_gpu_engine.py uses for the fp32 kernels
MAX_OFF_BY_ONE = 1e-3            # share of codes that may differ by one (value within fp32 rounding of a midpoint)


def table_gap(code):
    return float((code[1:] - code[:-1]).max())


def random_state(opt, params, gen, zero_block_of=None):
    """Arbitrary valid optimizer state: random fp32 moments of very different block magnitudes, quantised; step 3.  The second moment
    is at least the square of the first, as in any Adam history, so that the update m / sqrt(v) stays O(1) and the parameter
    comparison at fp32 rounding is not dominated by cancellation against a huge update."""
    for p in params:
        n = p.numel()
        mag = torch.rand((n + QBLOCK - 1) // QBLOCK, generator=gen).mul(6).sub(4).exp().repeat_interleave(QBLOCK)[:n]
        m = torch.randn(n, generator=gen) * mag
        v = m ** 2 + (torch.randn(n, generator=gen) * mag * 0.3) ** 2
        if p is zero_block_of:
            m[QBLOCK:2 * QBLOCK] = 0
            v[QBLOCK:2 * QBLOCK] = 0
        opt.set_moments(p, m.view_as(p), v.view_as(p), step=3)


def build_case(device="cpu", seed=0):
    """Tensors: 256 k elements; a partial last block; below min_8bit_size; a block whose state and gradient are zero (absmax 0);
    one without a gradient; one whose storage is only 4-byte aligned.  Two groups with different lr / weight_decay."""
    gen = torch.Generator().manual_seed(seed)
    sizes = dict(k256=(20, 256), partial=(5000,), small=(100,), zero_block=(8192,), no_grad=(4103,), misaligned=(4500,))
    params = {}
    for name, shape in sizes.items():
        if name == "misaligned":
            buf = torch.randn(4501, generator=gen).to(device)
            params[name] = torch.nn.Parameter(buf[1:])
        else:
            params[name] = torch.nn.Parameter(torch.randn(*shape, generator=gen).to(device))
    for name, p in params.items():
        if name == "no_grad":
            continue
        g = torch.randn(p.shape, generator=gen) * 0.3
        if name == "zero_block":
            g[QBLOCK:2 * QBLOCK] = 0
        if name == "misaligned":
            gbuf = torch.zeros(4503).to(device)
            gbuf[3:] = g.to(device)
            p.grad = gbuf[3:]
        else:
            p.grad = g.to(device)
    groups = [{"params": [params["k256"], params["partial"], params["small"]]},
              {"params": [params["zero_block"], params["no_grad"], params["misaligned"]], "lr": 3e-2, "weight_decay": 0.1}]
    opt = AdamW8bit(groups, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    random_state(opt, list(params.values()), gen, zero_block_of=params["zero_block"])
    return opt, params


def cpu_twin(opt):
    """A CPU copy of an optimizer with its parameters, gradients and state (the restatement runs on it)."""
    groups = []
    pairs = []
    for g in opt.param_groups:
        ps = []
        for p in g["params"]:
            q = torch.nn.Parameter(p.detach().cpu().clone())
            if p.grad is not None:
                q.grad = p.grad.detach().cpu().clone()
            ps.append(q)
            pairs.append((p, q))
        groups.append({**{k: v for k, v in g.items() if k != "params"}, "params": ps})
    twin = AdamW8bit(groups, min_8bit_size=opt.min_8bit_size)
    twin._ensure_state()
    opt._ensure_state()
    for p, q in pairs:
        for k, v in opt.state[p].items():
            if torch.is_tensor(v):
                twin.state[q][k].copy_(v.cpu())
            else:
                twin.state[q][k] = copy.copy(v)
    return twin, pairs


def compare_with_restatement(opt, pairs, twin, label=""):
    """After the same step on ``opt`` (kernel) and ``twin`` (restatement): parameters to fp32 rounding, absmax bit-equal, codes equal
    except a one-code difference on at most MAX_OFF_BY_ONE of the elements.  Returns (elements, codes off by one)."""
    total = off = 0
    for p, q in pairs:
        a, b = opt.state[p], twin.state[q]
        assert a["step"] == b["step"]
        assert torch.allclose(p.detach().cpu(), q.detach(), rtol=RTOL, atol=ATOL), (label, float((p.detach().cpu() - q.detach()).abs().max()))
        if "absmax1" not in a:
            for k in ("state1", "state2"):
                assert torch.allclose(a[k].cpu(), b[k], rtol=RTOL, atol=1e-12), (label, k)
            continue
        for k in ("absmax1", "absmax2"):
            assert torch.equal(a[k].cpu(), b[k]), (label, k)
        for k in ("state1", "state2"):
            d = (a[k].cpu().int() - b[k].int()).abs()
            assert int(d.max()) <= 1, (label, k, int(d.max()))
            total += d.numel()
            off += int(d.sum())
    print(f"[{label}] {total} codes compared, {off} differ by one ({off / max(total, 1):.2e})", flush=True)
    assert off <= MAX_OFF_BY_ONE * total, (label, off, total)
    return total, off
