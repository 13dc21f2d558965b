"""The optimizer side of a training step — gradient clipping and AdamW — over the full-width UNet's parameter list (1 485 tensors,
1.413 G elements) and over the LoRA student's (1 150 tensors), synthetic gradients, one GPU:

    optim.AdamW.step() as a trainer calls it, and the t2v_adamw_multi launch alone
    optim.clip_grad_norm_ then step()                (three launches; the scaled gradients are written)
    optim.grad_clip_coef then step(grad_scale=coef)  (two launches; the coefficient stays on the device)
    torch.optim.AdamW, default foreach and fused=True; torch.nn.utils.clip_grad_norm_; the two together
    t2v_adamw_step on one flat buffer of the same size (the bandwidth yardstick); AdamW8bit.step()

All rows of a list are timed in ONE process, interleaved (one repetition of every row, then the next repetition), event-timed, warmed;
median, min, max and spread per row.  ``max_norm`` is far below the gradients' norm, so every clip really scales.

    python tools/adamw_bench.py [--reps 20] [--out profiles/r14_adamw_multi.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.set_num_threads(min(16, torch.get_num_threads()))

HYPER = dict(lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
MAX_NORM = 1.0


def shape_lists():
    from bench import VC2_UNET
    from t2v_turbo_amd import lora
    from t2v_turbo_amd.unet3d import UNetModel
    with torch.device("meta"):
        m = UNetModel(**VC2_UNET)
        full = [tuple(p.shape) for p in m.parameters()]
        m.requires_grad_(False)
        lora.inject_trainable_lora_extended(m, r=64)
        lo = [tuple(p.shape) for p in lora.lora_parameters(m)]
    return dict(full=full, lora=lo)


def make_params(shapes, dev, gen):
    """Parameters and gradients as views of two flat buffers, every tensor 16-byte aligned as separate allocations are."""
    offs, total = [], 0
    for s in shapes:
        offs.append(total)
        total += (torch.Size(s).numel() + 3) // 4 * 4
    flat_p = torch.randn(total, device=dev, generator=gen) * 0.05
    flat_g = torch.randn(total, device=dev, generator=gen) * 0.01
    params = []
    for s, o in zip(shapes, offs):
        p = torch.nn.Parameter(flat_p[o:o + torch.Size(s).numel()].view(s))
        p.grad = flat_g[o:o + torch.Size(s).numel()].view(s)
        params.append(p)
    return params, flat_p, flat_g


def interleaved(rows, reps, warmup=3):
    """rows: {name: callable}.  One repetition of every row, then the next: drift of the box lands on all rows alike."""
    for _ in range(warmup):
        for fn in rows.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(reps):
        for k, fn in rows.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), reps=reps) for k, v in ms.items()}


def bench_list(name, shapes, dev, reps):
    from t2v_turbo_amd import optim
    from t2v_turbo_amd.native import shared_ops
    from t2v_turbo_amd.optim import AdamW, AdamW8bit, clip_grad_norm_, grad_clip_coef
    gen = torch.Generator(device=dev).manual_seed(0)
    params, flat_p, flat_g = make_params(shapes, dev, gen)
    n_elem = sum(p.numel() for p in params)
    g0 = flat_g.clone()
    ops = shared_ops()

    ours = AdamW(params, **HYPER)
    ours.step()
    plan = ours._plan
    (start, end, work, _, _), = plan["launches"]
    t_foreach = torch.optim.AdamW(params, foreach=True, **HYPER)
    t_fused = torch.optim.AdamW(params, fused=True, **HYPER)
    o8 = AdamW8bit(params, **HYPER)
    fm, fv = torch.zeros_like(flat_p), torch.zeros_like(flat_p)
    hyper = [(HYPER["lr"], HYPER["weight_decay"], 0.9, 0.999, HYPER["eps"], 100)]

    def restore():   # the clipping rows scale the gradients in place: every repetition starts from the same ones (not timed apart:
        flat_g.copy_(g0)   # it is inside none of the rows below except where stated)

    def clip_step():
        clip_grad_norm_(params, MAX_NORM)
        ours.step()

    def coef_step():
        _, coef = grad_clip_coef(params, MAX_NORM)
        ours.step(grad_scale=coef)

    def torch_clip_fused():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        t_fused.step()

    rows = {
        "restore_gradients_copy": restore,
        "optim_AdamW_step": lambda: ours.step(),
        "t2v_adamw_multi_kernel_only": lambda: ops.adamw_multi(plan["table"], end - start, work, hyper, 1.0, None),
        "restore_1": restore,
        "optim_clip_grad_norm_then_step": clip_step,
        "restore_2": restore,
        "optim_grad_clip_coef_then_step_grad_scale": coef_step,
        "optim_clip_grad_norm_": lambda: clip_grad_norm_(params, MAX_NORM),
        "restore_3": restore,
        "torch_AdamW_foreach_step": lambda: t_foreach.step(),
        "torch_AdamW_fused_step": lambda: t_fused.step(),
        "torch_clip_grad_norm_": lambda: torch.nn.utils.clip_grad_norm_(params, MAX_NORM),
        "restore_4": restore,
        "torch_clip_grad_norm_then_fused_step": torch_clip_fused,
        "restore_5": restore,
        "t2v_adamw_step_flat_kernel_only": lambda: ops.adamw_step(flat_p, flat_g, fm, fv, HYPER["lr"], 0.9, 0.999, HYPER["eps"], HYPER["weight_decay"], 100, 1.0),
        "AdamW8bit_step": lambda: o8.step(),
    }
    res = interleaved(rows, reps)
    res = {k: v for k, v in res.items() if not k.startswith("restore_") or k == "restore_gradients_copy"}
    for k, bytes_per_elem in (("t2v_adamw_multi_kernel_only", 28), ("t2v_adamw_step_flat_kernel_only", 28), ("optim_AdamW_step", 28),
                              ("torch_AdamW_fused_step", 28), ("AdamW8bit_step", 16)):
        res[k]["GBps"] = n_elem * bytes_per_elem / (res[k]["median_ms"] * 1e-3) / 1e9
    a, b = res["optim_clip_grad_norm_then_step"], res["torch_clip_grad_norm_then_fused_step"]
    c = res["optim_grad_clip_coef_then_step_grad_scale"]
    verdict = dict(margin_ms=b["median_ms"] - a["median_ms"], larger_spread_ms=max(a["spread_ms"], b["spread_ms"]),
                   clip_then_step_faster_than_torch_clip_plus_fused=bool(b["median_ms"] - a["median_ms"] > max(a["spread_ms"], b["spread_ms"])),
                   folded_margin_ms=b["median_ms"] - c["median_ms"],
                   folded_faster_than_torch_clip_plus_fused=bool(b["median_ms"] - c["median_ms"] > max(c["spread_ms"], b["spread_ms"])))
    assert torch.isfinite(flat_p).all() and optim._CLIP_PLANS
    out = dict(tensors=len(shapes), elements=n_elem, work_blocks=work, table_uploads=ours.table_uploads, rows=res, verdict=verdict)
    del ours, t_foreach, t_fused, o8, fm, fv, params, flat_p, flat_g, g0
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lists", default="full,lora")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_adamw_multi.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    shapes = shape_lists()
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, max_norm=MAX_NORM, hyper=dict(HYPER, betas=list(HYPER["betas"])),
               method="one process, rows interleaved per repetition, event-timed, 3 warm-up rounds; spread = max - min")
    for name in args.lists.split(","):
        res[name] = bench_list(name, shapes[name], dev, args.reps)
        print(json.dumps({name: res[name]}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
