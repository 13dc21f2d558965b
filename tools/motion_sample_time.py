#!/usr/bin/env python
"""``motion_prior.motion_prior_sample`` at the FULL VideoCrafter2 width on the bench latent (1,4,16,40,64), 200-point solver,
``percentage=0.6`` — the native path (one ``t2v_mp_guided_step`` launch between the forwards of a step, fp32 state in place, one copy at
the end) against ``T2V_NATIVE_MP_SAMPLE=0`` (the torch twin), the two alternating in one process — and the uint8 tail
(``t2v_video_to_u8``) against the ATen chain on a decoded 16x320x512 clip:

    python tools/motion_sample_time.py [--steps 6] [--rounds 2] [--out profiles/r17_motion_sample.jsonl]

A window of ``--steps`` guided steps (from step 199 down) and one of ``--steps`` unguided steps (from step 40 down) stand for the 120 + 80
of a whole run: the steps of a kind do the same work.  Per side and kind, one JSON line: wall ms per step until the host has the
result; the launching thread's time between the end of one forward call and the start of the next, per step; the device-event window
minus the windows of the UNet forward calls, per step.  Hooks on the module take the timestamps: the sampler itself is not changed."""
import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE, CTX_DIM, NUM_DDIM, PERCENTAGE = (1, 4, 16, 40, 64), 1024, 200, 0.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bench
    from t2v_turbo_amd import cd_math
    from t2v_turbo_amd import motion_prior as mp
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
    example = torch.randn(SHAPE, generator=gen).to(dev)
    inverted = [example] * NUM_DDIM
    ctx = [{"context": torch.randn(1, 77, CTX_DIM, generator=gen).to(dev), "fps": 8} for _ in range(3)]
    guided = mp.guided_steps(PERCENTAGE, NUM_DDIM)
    windows = {"guided": (NUM_DDIM - 1, NUM_DDIM - a.steps), "unguided": (min(guided) - 41, min(guided) - 40 - a.steps)}
    assert windows["guided"][1] >= min(guided) and windows["unguided"][1] >= 0

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

    def one(kind, side):
        os.environ["T2V_NATIVE_MP_SAMPLE"] = side
        start, stop = windows[kind]
        del marks[:]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)          # the composite UNet path must not be taken
            out, info = mp.motion_prior_sample(m, solver, sched, latents, inverted, ctx[0], ctx[1], ctx[2], guidance_scale=7.5,
                                               percentage=PERCENTAGE, temp_loss_scale=100.0,
                                               rng=dict(noise=noise, start_latents=latents, start_step=start, stop_step=stop))
            float(out.flatten()[0])          # (the host has the result)
        wall = time.perf_counter() - t0
        e1.record()
        torch.cuda.synchronize()
        n = start - stop + 1
        fwd_ms = sum(s.elapsed_time(e) for _, _, s, e in marks)
        between = sum(b[0] - a_[1] for a_, b in zip(marks, marks[1:]))
        return dict(wall_ms_per_step=round(wall * 1e3 / n, 2), host_between_forwards_ms_per_step=round(between * 1e3 / n, 3),
                    outside_forwards_ms_per_step=round((e0.elapsed_time(e1) - fwd_ms) / n, 3), forwards=info["forwards"], steps=n,
                    device_to_host_copies=info["device_to_host_copies"])

    lines = []
    for kind in ("guided", "unguided"):
        runs = {"1": [], "0": []}
        for rnd in range(a.rounds + 1):          # round 0 records the engines' plans: not kept
            for side in ("1", "0") if rnd % 2 == 0 else ("0", "1"):
                r = one(kind, side)
                print(f"{kind} round {rnd} T2V_NATIVE_MP_SAMPLE={side}: {r}", file=sys.stderr, flush=True)
                if rnd:
                    runs[side].append(r)
        for side in ("1", "0"):
            best = min(runs[side], key=lambda r: r["wall_ms_per_step"])
            lines.append(dict(T2V_NATIVE_MP_SAMPLE=int(side), kind=kind, steps=list(windows[kind]), latent=list(SHAPE), num_ddim_timesteps=NUM_DDIM,
                              percentage=PERCENTAGE, unet="bf16, full width", rounds=a.rounds, best=best,
                              all_wall_ms_per_step=[r["wall_ms_per_step"] for r in runs[side]],
                              all_host_between_forwards_ms_per_step=[r["host_between_forwards_ms_per_step"] for r in runs[side]],
                              what="tools/motion_sample_time.py: motion_prior_sample over a window of steps, one clip, sides alternating in "
                                   "one process; outside_forwards = device-event window minus the windows of the UNet forward calls"))
    os.environ.pop("T2V_NATIVE_MP_SAMPLE", None)

    # the uint8 tail on a decoded clip: one launch against the ATen chain (clamp, +1, /2, *255, to(uint8), channels-last copy)
    video = torch.randn((1, 3, 16, 320, 512), generator=gen).to(dev, torch.bfloat16)

    def aten(v):
        return ((v.clamp(-1.0, 1.0) + 1.0) / 2.0 * 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()

    def timed(fn, iters=50):
        for _ in range(5):
            fn(video)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(iters):
            fn(video)
        e1.record()
        host = (time.perf_counter() - t0) / iters
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / iters * 1e3, 1), round(host * 1e6, 1)
    tail = {}
    for rnd in range(a.rounds):
        for name, fn in (("native", mp.video_to_uint8), ("aten", aten)) if rnd % 2 == 0 else (("aten", aten), ("native", mp.video_to_uint8)):
            tail.setdefault(name, []).append(timed(fn))
    lines.append(dict(kind="uint8 tail", video=list(video.shape), dtype="bf16",
                      native_us_device_host=min(tail["native"]), aten_us_device_host=min(tail["aten"]), all=tail,
                      what="t2v_video_to_u8 (one launch) against ((v.clamp(-1, 1) + 1) / 2 * 255).to(uint8).permute(0, 2, 3, 4, 1).contiguous() "
                           "in bf16 (six launches); us per call over 50 back-to-back calls: (device-event window, launching thread)"))
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
