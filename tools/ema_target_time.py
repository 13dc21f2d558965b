#!/usr/bin/env python
"""The EMA target network of train_latent_t2v_turbo_v2.py --use_target_unet (:671-675, :1238-1245, :1272-1276) at the FULL VideoCrafter2
width and the bench latent (1,4,16,40,64) on the device: a frozen train-mode copy of the UNet, fp32 parameters, bf16 engine, called under
``no_grad`` through the module route; a student whose weights are perturbed every step; per step ONE ``update_ema`` of the target and
two target forwards — the first after the update, the second with no update in between (the floor).  One JSON line:

    ema_ms             per update_ema, until the device is done
    fwd_after_ema_ms   the first target forward after an update (a pack refresh + a replay, or packing + recording the network again)
    fwd_floor_ms       a target forward with nothing changed
    peak_mem_gb, counters (the engine's ``{"recorded", "refreshed"}``; None where the engine keeps none)

Runs unmodified on older trees (a same-box comparison needs both sides in one job): where ``optim.update_ema`` is absent it uses
``cd_math.update_ema``, where the engine has no ``counters`` it reports None.

    python tools/ema_target_time.py [--steps 4] [--variant NAME] [--graph 1]
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4, help="timed steps (after one untimed step that records the target's plan)")
    ap.add_argument("--variant", default="", help="a label for the JSON line")
    ap.add_argument("--graph", type=int, default=1, help="1: the target's launch list as a hipGraph once it has been replayed (T2V_HIP_GRAPH)")
    ap.add_argument("--rate", type=float, default=0.95)
    args = ap.parse_args()
    import bench
    from t2v_turbo_amd import cd_math, optim
    update_ema = getattr(optim, "update_ema", None)
    how = "optim.update_ema"
    if update_ema is None:
        update_ema, how = cd_math.update_ema, "cd_math.update_ema"
    dev = torch.device("cuda", 0)
    student = bench.build_model(dev, torch.float32)
    target = copy.deepcopy(student).requires_grad_(False).train()
    x, ctx, tc = bench.synth_inputs(dev, torch.float32)
    ts = torch.tensor([999], device=dev)
    s_params, t_params = list(student.parameters()), list(target.parameters())
    gen = torch.Generator(device=dev).manual_seed(0)

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    def forward():
        t0 = sync()
        with torch.no_grad():
            y = target(x, ts, context=ctx, fps=16, timestep_cond=tc)
        return (sync() - t0) * 1e3, y

    torch.cuda.reset_peak_memory_stats()
    record_ms, y = forward()
    eng = target._engine_box.engine
    assert eng is not None, "the target did not run on the inference engine"
    eng.use_graph = bool(args.graph)
    ema, after, floor = [], [], []
    finite = bool(torch.isfinite(y).all())
    for step in range(args.steps + 2):       # two untimed steps: the eager refresh, then its capture (and the plan's hipGraph)
        with torch.no_grad():
            for p in s_params:               # (the optimizer's part: the student moves)
                p.add_(torch.randn(p.shape, generator=gen, device=dev, dtype=p.dtype), alpha=1e-4)
        t0 = sync()
        update_ema(t_params, s_params, args.rate)
        t_ema = (sync() - t0) * 1e3
        t_after, y = forward()
        t_floor, y2 = forward()
        finite = finite and bool(torch.isfinite(y).all())
        if step >= 2:
            ema.append(t_ema), after.append(t_after), floor.append(t_floor)
    rnd = lambda v: [round(t, 2) for t in v]   # noqa: E731
    out = {"variant": args.variant, "update_ema": how, "rate": args.rate, "graph": bool(args.graph), "params_m": round(sum(p.numel() for p in t_params) / 1e6, 1),
           "tensors": len(t_params), "record_ms": round(record_ms, 1), "ema_ms": rnd(ema), "fwd_after_ema_ms": rnd(after), "fwd_floor_ms": rnd(floor),
           "ema_ms_min": round(min(ema), 2), "fwd_after_ema_ms_min": round(min(after), 2), "fwd_floor_ms_min": round(min(floor), 2),
           "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1), "counters": getattr(eng, "counters", None),
           "plans": len(eng.plans), "packs": len(eng.pk), "all_finite": finite}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
