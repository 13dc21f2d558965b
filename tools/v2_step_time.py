#!/usr/bin/env python
"""The v2 step (``distill.distill_step_v2``) and its consistency head (``cd_head``) on the device, at the bench latent (1,4,16,40,64):

    python tools/v2_step_time.py --leg head [--iters 200] [--rounds 5]
        the head alone — ``solver_step_v2`` + ``consistency_loss`` + ``loss.backward()`` on seeded bf16 records and fp32 predictions —
        native (csrc/train.hip) against ``T2V_NATIVE_CD_HEAD=0`` (the torch twin over ATen kernels), the two alternating in one
        process: per round and side, host time of the launching thread per head (a host clock around ``iters`` enqueues, the queue
        empty before), the device-event window around the same enqueues (the host's pace where the host is the slower side), and
        the device's own time per head (device events around ``iters`` heads enqueued behind a backlog).  One JSON line per side.
    python tools/v2_step_time.py --leg step --target {0,1} [--steps 4]
        the whole step at the FULL VideoCrafter2 width: full fine-tuning student in train mode, ``AdamW8bit``, with / without a frozen
        train-mode EMA target network; ms per step until the device is done, after two untimed steps.  One JSON line.
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
SHAPE = (1, 4, 16, 40, 64)


def _records(gen, dtype=torch.float16):
    c = torch.randn(SHAPE, generator=gen)
    return {"index": torch.tensor([37]), "z_t": torch.randn(SHAPE, generator=gen).to(dtype), "cond_teacher_out": c.to(dtype),
            "uncond_teacher_out": (c + 0.3 * torch.randn(SHAPE, generator=gen)).to(dtype),
            "score": (0.2 * torch.randn(SHAPE, generator=gen)).to(dtype), "use_motion_guide": torch.tensor([True]), "txt": ["a clip"]}


def head_leg(args):
    from t2v_turbo_amd import cd_head, cd_math
    from t2v_turbo_amd.scheduler import T2VTurboScheduler
    dev = torch.device("cuda", 0)
    sched = T2VTurboScheduler()
    acp = sched.alphas_cumprod
    solver = cd_math.DDIMSolver(acp.numpy(), ddim_timesteps=50)
    gen = torch.Generator().manual_seed(0)
    rec = _records(gen)
    z, c, u, score = (rec[k].to(dev).bfloat16() for k in ("z_t", "cond_teacher_out", "uncond_teacher_out", "score"))
    index, umg = rec["index"].to(dev), rec["use_motion_guide"].to(dev)
    w, mgs = torch.tensor([7.5], device=dev), torch.tensor([0.05], device=dev)
    noise_pred = torch.randn(SHAPE, generator=gen).to(dev).requires_grad_(True)
    target_noise_pred = torch.randn(SHAPE, generator=gen).to(dev)
    min_index = cd_head.motion_min_index(0.5, 50)

    def head():
        noise_pred.grad = None
        x_prev = cd_head.solver_step_v2(solver, acp, index, z, c, u, score, w, mgs, umg, min_index=min_index)
        loss, _ = cd_head.consistency_loss(solver, acp, index, noise_pred, target_noise_pred, z, x_prev, topk=5)
        loss.backward()
        return loss

    def window(n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(n):
            head()
        host = time.perf_counter() - t0
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3, host / n * 1e6      # us per head: device, host

    # A head is a handful of short launches: enqueued one by one the device waits for the host, and the event window above is the host's
    # time.  The device's own time is taken behind a backlog: enough large matrix products go first that every head of the window is in
    # the queue before the device reaches the first one; ``held`` says that it was (the start event had not completed when the host
    # finished enqueueing).
    a = torch.randn(8192, 8192, device=dev)
    torch.mm(a, a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        torch.mm(a, a)
    torch.cuda.synchronize()
    mm_s = (time.perf_counter() - t0) / 10

    def backlog_window(n, host_us):
        k = int(3.0 * n * host_us * 1e-6 / mm_s) + 2
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(k):
            torch.mm(a, a)
        e0.record()
        for _ in range(n):
            head()
        held = not e0.query()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / n * 1e3, 2), held

    out = {"1": [], "0": []}
    busy = {"1": [], "0": []}
    losses, grads = {}, {}
    for rnd in range(args.rounds + 1):           # round 0: warm-up of both sides, not kept
        for side in ("1", "0") if rnd % 2 == 0 else ("0", "1"):
            os.environ["T2V_NATIVE_CD_HEAD"] = side
            window(10)
            dev_us, host_us = window(args.iters)
            if rnd:
                out[side].append((round(dev_us, 2), round(host_us, 2)))
                busy[side].append(backlog_window(args.iters, host_us))
            losses[side], grads[side] = float(head().detach()), noise_pred.grad.clone()
    del os.environ["T2V_NATIVE_CD_HEAD"]
    diff = float((grads["1"] - grads["0"]).abs().max())
    for side in ("1", "0"):
        d, h = [a for a, _ in out[side]], [b for _, b in out[side]]
        print(json.dumps({"leg": "head", "T2V_NATIVE_CD_HEAD": int(side), "latent": list(SHAPE), "records": "bf16", "noise_pred": "fp32",
                          "iters": args.iters, "window_us_per_head": d, "host_us_per_head": h, "window_us_median": sorted(d)[len(d) // 2],
                          "host_us_median": sorted(h)[len(h) // 2], "device_us_per_head_behind_backlog": [b for b, _ in busy[side]],
                          "backlog_held": [k for _, k in busy[side]], "device_us_median": sorted(b for b, _ in busy[side])[len(busy[side]) // 2], "loss": losses[side], "max_abs_grad_diff_between_sides": diff,
                          "what": "tools/v2_step_time.py --leg head: solver_step_v2 + consistency_loss + loss.backward(), sides alternating in one process"}),
              flush=True)


def step_leg(args):
    import warnings
    import bench
    from t2v_turbo_amd import cd_math, optim
    from t2v_turbo_amd.distill import distill_step_v2
    from t2v_turbo_amd.scheduler import T2VTurboScheduler
    dev = torch.device("cuda", 0)
    student = bench.build_model(dev, torch.float32).requires_grad_(True).train()
    target = copy.deepcopy(student).requires_grad_(False).train() if args.target else None
    opt = optim.AdamW8bit(student.parameters(), lr=1e-6, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    sched = T2VTurboScheduler()
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=50)
    gen = torch.Generator().manual_seed(0)
    batch = _records(gen)
    batch["prompt_emb"] = torch.randn(1, 77, 1024, generator=gen).half()
    batch = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in batch.items()}
    times, losses, host = [], [], []
    torch.cuda.reset_peak_memory_stats()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)           # the composite UNet path must not be taken
        for step in range(args.steps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, info = distill_step_v2(student, solver, sched, batch, target_unet=target, optimizer=opt, weight_dtype=torch.bfloat16,
                                         rng=dict(w=torch.tensor([7.5])))
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            losses.append(float(loss.detach()))
            if step >= 2:
                times.append(round((t2 - t0) * 1e3, 1)), host.append(round((t1 - t0) * 1e3, 1))
    print(json.dumps({"leg": "step", "target_unet": bool(args.target), "T2V_NATIVE_CD_HEAD": int(os.environ.get("T2V_NATIVE_CD_HEAD", "1")),
                      "latent": list(SHAPE), "optimizer": "AdamW8bit", "params_m": round(sum(p.numel() for p in student.parameters()) / 1e6, 1),
                      "step_ms": times, "step_ms_min": min(times), "host_ms": host, "host_phases_ms_last": info["host_ms"], "losses": losses,
                      "all_finite": all(l == l and abs(l) != float("inf") for l in losses),
                      "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
                      "what": "tools/v2_step_time.py --leg step: distill_step_v2, full-width student (fp32 parameters, train mode, full "
                              "fine-tuning route), recorded bf16 teacher outputs"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["head", "step"], required=True)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--target", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    head_leg(args) if args.leg == "head" else step_leg(args)


if __name__ == "__main__":
    main()
