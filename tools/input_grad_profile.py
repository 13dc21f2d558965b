#!/usr/bin/env python
"""Time ``motion_prior.get_motion_prior_score`` through the module call at full width (bf16, 1 x 4 x 16 x 40 x 64, synthetic weights):

    python tools/input_grad_profile.py --leg on   --out profile.jsonl     # native_input_grad on: engine route + fused loss kernel
    python tools/input_grad_profile.py --leg torchloss --out ...          # route on, the torch loss written out (reference pattern)
    python tools/input_grad_profile.py --leg kernel --out ...             # t2v_rank_loss alone on the nine recorded tensors
    python tools/input_grad_profile.py --leg off  --out ...               # the default: torch composite path + torch loss (run it last)

One leg per process (the peak memory is the process's); each appends one JSON line.  Times: host clock around calls that end in a
device synchronise; the kernel leg: device events around a run of calls."""
import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["on", "torchloss", "kernel", "off"], required=True)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiny", type=int, default=0, help="toy widths (plumbing check)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bench
    from t2v_turbo_amd import motion_prior as mp
    from t2v_turbo_amd.unet3d import UNetModel
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    cfg = dict(bench.VC2_UNET, record_attn_probs=True)
    shape, ctx_dim = (1, 4, 16, 40, 64), 1024
    if a.tiny:
        cfg.update(model_channels=64, context_dim=128)
        shape, ctx_dim = (1, 4, 4, 16, 16), 128
    torch.manual_seed(0)
    with torch.device(dev):
        m = UNetModel(**cfg)
    with torch.no_grad():
        for p in m.parameters():   # the zero-initialised output projections would leave most of the backward with zeros
            if float(p.abs().max()) == 0:
                p.normal_(0.0, 0.02)
    m = m.to(torch.bfloat16).eval().requires_grad_(False)
    m.dtype = torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(shape, device=dev, generator=gen).bfloat16()
    example = torch.randn(shape, device=dev, generator=gen).bfloat16()
    ts = torch.tensor([499], device=dev)
    ctx = {"context": torch.randn(1, 77, ctx_dim, device=dev, generator=gen).bfloat16(), "fps": 16,
           "timestep_cond": torch.randn(1, 256, device=dev, generator=gen).bfloat16()}
    m.native_input_grad = a.leg != "off"
    rec = {"leg": a.leg, "shape": list(shape), "dtype": "bf16", "steps": a.steps, "warmup": a.warmup,
           "cmd": "python tools/input_grad_profile.py --leg " + a.leg}

    def score_torchloss():
        """The body of ``get_motion_prior_score`` with the torch loss written out.  The example probabilities are cast to the dtype of
        the differentiated ones: the composite path's are bf16 here, the inference engine's fp32, and ``F.mse_loss`` refuses the mix in
        its backward — which is why the "off" leg cannot call ``get_motion_prior_score`` itself at bf16."""
        with torch.no_grad():
            _, ex = mp.get_temp_attn_prob(m, example, ts, ctx)
        lat = x.clone().requires_grad_(True)
        out, probs = mp.get_temp_attn_prob(m, lat, ts, ctx)
        ex = {k: v.to(probs[k].dtype) for k, v in ex.items()}
        return torch.autograd.grad(500.0 * mp.compute_temp_loss(probs, ex), lat)[0], out

    if a.leg == "kernel":
        from t2v_turbo_amd.native import HipOps
        ops = HipOps()
        with torch.no_grad():
            _, probs = mp.get_temp_attn_prob(m, x, ts, ctx)
            probs = [p.clone() for p in probs.values()]
            _, ex = mp.get_temp_attn_prob(m, example, ts, ctx)
        n = probs[0].shape[-1]
        problems = [(e, p, torch.empty_like(p)) for e, p in zip(ex.values(), probs)]
        ws = torch.empty(ops.rank_loss_ws_floats([p.numel() // n for p in probs], n), device=dev)
        loss = torch.empty(len(problems), device=dev)
        for _ in range(5):
            ops.rank_loss(problems, n, 1, 1.0, ws, loss)
        torch.cuda.synchronize()
        reps = 50
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.rank_loss(problems, n, 1, 1.0, ws, loss)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / reps
        nbytes = sum(3 * p.numel() * 4 for p in probs)
        rec.update(layers=len(probs), shapes=[list(p.shape) for p in probs], us_per_call=round(us, 2), bytes_moved=nbytes,
                   gb_per_s=round(nbytes / us / 1e3, 1), note="device events around 50 back-to-back calls (main + final launch each)")
    else:
        fn = score_torchloss if a.leg in ("torchloss", "off") else (lambda: mp.get_motion_prior_score(m, x.clone(), ts, example, ctx, ctx, 500.0))
        with warnings.catch_warnings():
            warnings.simplefilter("error" if a.leg != "off" else "ignore", RuntimeWarning)
            for _ in range(a.warmup):
                score, _ = fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            times = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                score, _ = fn()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
        assert torch.isfinite(score).all()
        times.sort()
        rec.update(ms_per_score_median=round(times[len(times) // 2], 2), ms_min=round(times[0], 2), ms_max=round(times[-1], 2),
                   peak_allocated_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                   peak_reserved_gb=round(torch.cuda.max_memory_reserved() / 2 ** 30, 2),
                   score_norm=float(score.float().norm()),
                   route="input_grad" if m._engine_box.input is not None else "composite")
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
