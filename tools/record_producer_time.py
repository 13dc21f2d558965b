#!/usr/bin/env python
"""``preprocess.make_latent_records`` at the FULL VideoCrafter2 width on the bench latent (1,4,16,40,64), 200-point solver, one clip per
call, for ``index`` 24 and 199 — the native path (csrc/train.hip between the forwards, one pack launch, one copy) against
``T2V_NATIVE_RECORD=0`` (the torch twin), the two alternating in one process:

    python tools/record_producer_time.py [--index 24 199] [--rounds 2] [--out profiles/r16_record_producer.jsonl]

Per side and index, one JSON line: wall ms per record until the records are on the host; the device-event window of the call minus the
windows of the UNet forwards (what the device spends, or idles, outside the forwards); the launching thread's time between the end of
one forward call and the start of the next; the number of forwards and of device-to-host copies.  Hooks on the module take the
timestamps: the producer itself is not changed."""
import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE, CTX_DIM, NUM_DDIM = (1, 4, 16, 40, 64), 1024, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", type=int, nargs="+", default=[24, 199])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bench
    from t2v_turbo_amd import cd_math, preprocess
    from t2v_turbo_amd.scheduler import T2VTurboScheduler
    from t2v_turbo_amd.unet3d import UNetModel
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with torch.device(dev):
        m = UNetModel(**dict(bench.VC2_UNET, record_attn_probs=True))
    with torch.no_grad():
        for p in m.parameters():
            if float(p.abs().max()) == 0:
                p.normal_(0.0, 0.02)
    m = m.to(torch.bfloat16).eval().requires_grad_(False)
    m.dtype = torch.bfloat16
    sched = T2VTurboScheduler()
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=NUM_DDIM)
    gen = torch.Generator().manual_seed(1)
    latents = torch.randn(SHAPE, generator=gen).to(dev)
    noise = torch.randn(SHAPE, generator=gen)
    ctx = torch.randn(1, 77, CTX_DIM, generator=gen).to(dev)
    unc = torch.randn(1, 77, CTX_DIM, generator=gen).to(dev)

    marks = []          # (host time at entry, host time at exit, event at entry, event at exit) per forward call

    def pre(mod, args, kwargs):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append([time.perf_counter(), None, e, None])

    def post(mod, args, kwargs, out):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks[-1][1], marks[-1][3] = time.perf_counter(), e

    m.register_forward_pre_hook(pre, with_kwargs=True)
    m.register_forward_hook(post, with_kwargs=True)

    def one(index, side):
        os.environ["T2V_NATIVE_RECORD"] = side
        del marks[:]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("error" if side == "1" else "default", RuntimeWarning)     # native: the composite UNet path must not be taken
            blobs, info = preprocess.make_latent_records(m, solver, sched, latents, ctx, unc, motion=True, fps=8, temp_loss_scale=100.0,
                                                         rng=dict(index=torch.tensor([index]), noise=noise))
        wall = time.perf_counter() - t0
        e1.record()
        torch.cuda.synchronize()
        fwd_ms = sum(s.elapsed_time(e) for _, _, s, e in marks)
        between = sum(b[0] - a[1] for a, b in zip(marks, marks[1:]))
        return dict(wall_ms=round(wall * 1e3, 1), device_window_ms=round(e0.elapsed_time(e1), 1), forwards=len(marks),
                    forward_windows_ms=round(fwd_ms, 1), outside_forwards_ms=round(e0.elapsed_time(e1) - fwd_ms, 2),
                    host_between_forwards_ms=round(between * 1e3, 2), device_to_host_copies=info["device_to_host_copies"],
                    record_bytes=len(blobs[0]))

    lines = []
    for index in a.index:
        runs = {"1": [], "0": []}
        for rnd in range(a.rounds + 1):          # round 0 records the engines' plans: not kept
            for side in ("1", "0") if rnd % 2 == 0 else ("0", "1"):
                r = one(index, side)
                print(f"index {index} round {rnd} T2V_NATIVE_RECORD={side}: {r}", file=sys.stderr, flush=True)
                if rnd:
                    runs[side].append(r)
        for side in ("1", "0"):
            best = min(runs[side], key=lambda r: r["wall_ms"])
            lines.append(dict(T2V_NATIVE_RECORD=int(side), index=index, latent=list(SHAPE), num_ddim_timesteps=NUM_DDIM, unet="bf16, full width",
                              rounds=a.rounds, best=best, all_wall_ms=[r["wall_ms"] for r in runs[side]],
                              all_outside_forwards_ms=[r["outside_forwards_ms"] for r in runs[side]],
                              all_host_between_forwards_ms=[r["host_between_forwards_ms"] for r in runs[side]],
                              what="tools/record_producer_time.py: make_latent_records(motion=True), one clip, sides alternating in one process; "
                                   "outside_forwards_ms = device-event window of the call minus the windows of the UNet forward calls"))
    os.environ.pop("T2V_NATIVE_RECORD", None)
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
