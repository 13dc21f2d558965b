#!/usr/bin/env python
"""Memory and step time of the full fine-tuning student with and without activation checkpointing, at the batch sizes of
train_t2v_turbo_v2.sh (``--train_batch_size 3 --use_motion_cond``, yaml ``use_checkpoint: true``): the FULL VideoCrafter2 width, train
mode, latent (B,4,16,40,64), forward + backward through the module route (``unet(...)``, ``loss.backward()``) with an SGD-style update of
every weight between steps, as bench.py's ``full_finetune_step`` leg.  One JSON line: the engine's activation pool (``pool.bytes``), the
peak of ``torch.cuda.max_memory_allocated`` (pool + packs + gradient arena and its hand-over copy + the fp32 parameters and their
``.grad`` — NOT the EMA target, the optimizer state or the reward branch), launches per list, and the median step time after the
recording step and the two pack-refresh steps (eager, then captured).

    python tools/full_finetune_memory.py --batch 3 --checkpoint 1 [--motion] [--steps 3]
    python tools/full_finetune_memory.py --sweep [--motion]      # B = 1, 2, 3 x checkpoint on / off, one child process each

A configuration that does not fit is a result: its line carries ``error`` and the sweep stops there."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(args):
    import torch
    import bench
    from t2v_turbo_amd.nn_util import guidance_embedding
    from t2v_turbo_amd.unet3d import UNetModel
    dev = torch.device("cuda", 0)
    B = args.batch
    out = {"batch": B, "checkpoint": bool(args.checkpoint), "motion_cond": bool(args.motion), "latent": [B, 4, 16, 40, 64], "train_mode": True}
    if args.motion:   # bench.build_model (its seed, device construction and the re-draw of zero-initialised tensors, line for line)
        # with the motion-guidance projections of the v2 student; bench.py is a yardstick and takes no configuration argument
        torch.manual_seed(1234)
        with torch.device(dev):
            m = UNetModel(**dict(bench.VC2_UNET, motion_cond_proj_dim=256))
        g = torch.Generator(device=dev).manual_seed(1234)
        with torch.no_grad():
            for p in m.parameters():
                if float(p.abs().max()) == 0.0:
                    p.normal_(0.0, 0.02, generator=g)
    else:
        m = bench.build_model(dev, torch.float32)
    m.requires_grad_(True)
    m.train()
    m.native_checkpoint = bool(args.checkpoint)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 4, 16, 40, 64, generator=gen).to(dev)
    ctx = torch.randn(B, 77, 1024, generator=gen).to(dev)
    tc = guidance_embedding(torch.linspace(5.0, 10.0, B), 256).to(dev)
    ts = torch.linspace(999, 399, B).long().to(dev)
    kw = {"motion_cond": torch.randn(B, 256, generator=gen).to(dev)} if args.motion else {}
    params = list(m.parameters())
    out["params_m"] = round(sum(p.numel() for p in params) / 1e6, 1)
    times = []
    torch.cuda.reset_peak_memory_stats()
    try:
        for step in range(args.steps + 3):   # 0 records the two launch lists, 1 re-makes the packs eagerly, 2 captures that refresh
            for p in params:
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("error")    # the torch-composite route warns: it must not be taken
                y = m(x, ts, context=ctx, fps=16, timestep_cond=tc, **kw)
            y.float().pow(2).mean().backward()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            with torch.no_grad():
                for p in params:
                    p.add_(p.grad, alpha=-1e-6)
        eng = m._engine_box.full
        assert eng.checkpoint_blocks is bool(args.checkpoint) and len(eng.plans) == 1
        plan = eng._last
        out.update(pool_bytes=eng.pool.bytes, pool_gb=round(eng.pool.bytes / 2 ** 30, 2),
                   max_memory_allocated=torch.cuda.max_memory_allocated(), peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                   launches={"forward": len(plan["rec"]), "backward": len(plan["rec_bwd"])},
                   ms_per_step_median=round(statistics.median(times[3:]), 1), ms_all=[round(t, 1) for t in times],
                   all_grads_finite=all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params))
    except (RuntimeError, MemoryError) as e:   # (torch.OutOfMemoryError is a RuntimeError)
        out.update(error=f"{type(e).__name__}: {str(e)[:300]}", at_step=len(times),
                   peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
        print(json.dumps(out), flush=True)
        return 1
    print(json.dumps(out), flush=True)
    return 0


def sweep(args):
    """Every configuration in a fresh child process under its own time limit; the first one that fails ends the sweep."""
    for batch in (1, 2, 3):
        for ck in (1, 0):
            cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(batch), "--checkpoint", str(ck), "--steps", str(args.steps)]
            cmd += ["--motion"] if args.motion else []
            child = subprocess.Popen(cmd)
            try:
                rc = child.wait(timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                child.terminate()            # let it close the device itself; kill only if it does not
                try:
                    child.wait(timeout=30)
                except subprocess.TimeoutExpired:
                    child.kill()
                    child.wait()
                print(json.dumps({"batch": batch, "checkpoint": bool(ck), "error": f"no result within {args.child_timeout} s"}), flush=True)
                return 1
            if rc != 0:
                return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--checkpoint", type=int, choices=(0, 1), default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed steps after the recording step and the two pack-refresh steps")
    ap.add_argument("--motion", action="store_true", help="pass motion_cond (the network gets motion_cond_proj / combine_proj)")
    ap.add_argument("--sweep", action="store_true", help="B = 1, 2, 3 with checkpointing on and off, one child process each")
    ap.add_argument("--child-timeout", type=int, default=600,
                    help="seconds per configuration of --sweep, from building the network to the last step")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    sys.exit(sweep(args) if args.sweep else run(args))


if __name__ == "__main__":
    main()
