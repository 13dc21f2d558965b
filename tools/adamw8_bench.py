"""Optimizer step over the full-width UNet's parameter list (1 485 tensors, 1.413 B elements, synthetic gradients) on one GPU:
``t2v_adamw8_step`` (optim.AdamW8bit, 16 B / element) against (a) ``t2v_adamw_step`` on one flat fp32 buffer of the same size and
(b) ``torch.optim.AdamW(fused=True)`` on the same tensors (28 B / element each).  Event-timed, warmed, median and spread.

    python tools/adamw8_bench.py [--reps 20] [--out profiles/r07_adamw8_step.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_adamw8_step.json"))
    args = ap.parse_args()
    from bench import VC2_UNET
    from t2v_turbo_amd.native import shared_ops
    from t2v_turbo_amd.optim import AdamW8bit
    from t2v_turbo_amd.unet3d import UNetModel
    with torch.device("meta"):
        shapes = [tuple(p.shape) for p in UNetModel(**VC2_UNET).parameters()]
    dev = torch.device("cuda", 0)
    offs, total = [], 0
    for s in shapes:   # every tensor 16-byte aligned, as separate allocations are
        offs.append(total)
        total += (torch.Size(s).numel() + 3) // 4 * 4
    n_elem = sum(torch.Size(s).numel() for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)
    flat_p = torch.randn(total, device=dev, generator=gen) * 0.05
    flat_g = torch.randn(total, device=dev, generator=gen) * 0.01
    params = []
    for s, o in zip(shapes, offs):
        p = torch.nn.Parameter(flat_p[o:o + torch.Size(s).numel()].view(s))
        p.grad = flat_g[o:o + torch.Size(s).numel()].view(s)
        params.append(p)
    res = dict(device=torch.cuda.get_device_name(0), tensors=len(shapes), elements=n_elem, reps=args.reps)

    def rate(r, bytes_per_elem):
        r["GBps"] = n_elem * bytes_per_elem / (r["median_ms"] * 1e-3) / 1e9
        return r

    # 8-bit: the optimizer's step() as a trainer calls it, and the kernel launch alone
    opt = AdamW8bit(params, lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    opt.step()
    r8 = rate(timed(lambda: opt.step(), args.reps), 16)
    t, a = opt._table, opt._arena
    c1, c2 = opt._codes_on(dev)
    ops = shared_ops()
    (start, end, work, _), = t["launches"]
    k8 = rate(timed(lambda: ops.adamw8_step(t["dev"], end - start, work, a["s1"], a["s2"], a["a1"], a["a2"], a["f1"], a["f2"], c1, c2,
                                            0.9, 0.999, 1e-8, 100, 1.0), args.reps), 16)
    res["adamw8_step"] = dict(optimizer_step=r8, kernel_only=k8, state_bytes=opt.state_bytes(),
                              tensors_8bit=sum(1 for v in opt._layout.values() if v[0]),
                              tensors_fp32_state=sum(1 for v in opt._layout.values() if not v[0]))
    assert torch.isfinite(flat_p).all()
    del opt, t, a
    torch.cuda.empty_cache()

    # (a) the flat fp32 kernel on one buffer of the same size
    m, v = torch.zeros(total, device=dev), torch.zeros(total, device=dev)
    ra = rate(timed(lambda: ops.adamw_step(flat_p, flat_g, m, v, 1e-5, 0.9, 0.999, 1e-8, 1e-2, 100, 1.0), args.reps), 28)
    res["t2v_adamw_step_flat_fp32"] = dict(kernel_only=ra, state_bytes=2 * 4 * total)
    del m, v
    torch.cuda.empty_cache()

    # (b) torch's fused AdamW over the same tensor list
    ref = torch.optim.AdamW(params, lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, fused=True)
    rb = rate(timed(lambda: ref.step(), args.reps), 28)
    res["torch_adamw_fused"] = dict(optimizer_step=rb, state_bytes=2 * 4 * n_elem)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
