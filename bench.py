#!/usr/bin/env python
"""Headline benchmark: VideoCrafter2 UNet denoise steps/s on a 16-frame 320x512 clip
(latent (1,4,16,40,64), bf16) — BASELINE.json configs[1] — on N MI355X (one process per GPU).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one UNet forward of the t2v-turbo sampling loop (timesteps cycle through the 4-step
LCM table [999,759,519,279]) on synthetic inputs already resident in HBM.  Multi-GPU = independent
replicas (inference shards by clip, no collective): weak scaling, value = N*K / max-over-ranks time.
Rank 0 prints ONE JSON line.  `--dump-outputs DIR` writes the UNet output of
the last timed step as DIR/unet_out.npy (float32); weights and inputs are seeded, so two builds compare output for output.

A plain run does only what the headline figure needs: set up, warm up, time the steps, dump, print.  `--full` adds the
legs that take runs of their own (see DESIGN.md §Measurement for their objects): the per-kernel breakdown and the in-graph
roofline, the 4-step and 16-step v2 clips with VAE decode, the CPU oracle baseline with its parity gate, the distillation
step with its parity gate and the full fine-tuning step.  `--breakdown`, `--clip`, `--cpu-baseline`, `--distill` and
`--full-finetune` switch one leg on or off either way.

`python bench.py --gpus N` without a torchrun environment re-executes itself under `torch.distributed.run`
(one rank per GPU, rendezvous on 127.0.0.1).  With `--full` at N > 1 the `distill_step` leg (BASELINE config C3) runs on
every rank with the real flat-buffer gradient all-reduce (RCCL) and reports global samples/s.
`--dry-run-cpu 1` runs the same control flow on CPU (tiny widths, gloo, the emulated op backend of the test
suite): a plumbing check of the multi-rank path for boxes without GPUs, labelled as such, never a measurement.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

T_START = time.time()
UNET_TFLOP_PER_STEP = 12.581   # BASELINE.md §2 (2*MAC, matmul+conv, B=1, 16x40x64)
MFMA_PEAK_TFLOPS = 2500.0      # MI355X dense bf16 (MI355X_MICROARCH.md)
VAE_DECODE_TFLOP_16F = 25.02   # 1.5635 TFLOP per 320x512 frame x 16

VC2_UNET = dict(
    in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1], num_res_blocks=2,
    channel_mult=[1, 2, 4, 4], num_head_channels=64, transformer_depth=1, context_dim=1024, use_linear=True,
    use_checkpoint=False, temporal_conv=True, temporal_attention=True, temporal_selfatt_only=True,
    use_relative_position=False, use_causal_attention=False, temporal_length=16, addition_attention=True,
    fps_cond=True, time_cond_proj_dim=256)


def build_model(device, dtype):
    from t2v_turbo_amd.unet3d import UNetModel
    torch.manual_seed(1234)  # same random-init weights in every process / on every rank
    with torch.device(device):
        m = UNetModel(**VC2_UNET)
    g = torch.Generator(device=device).manual_seed(1234)
    with torch.no_grad():
        for p in m.parameters():  # zero_module'd tensors would make the output identically 0
            if float(p.abs().max()) == 0.0:
                p.normal_(0.0, 0.02, generator=g)
    m = m.to(dtype).eval()
    m.dtype = dtype
    return m


def synth_inputs(device, dtype):
    from t2v_turbo_amd.nn_util import guidance_embedding
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 4, 16, 40, 64, generator=g).to(device, dtype)
    ctx = torch.randn(1, 77, 1024, generator=g).to(device, dtype)
    tc = guidance_embedding(torch.tensor([7.5]), 256).to(device, dtype)
    return x, ctx, tc


# workgroup tile (rows, columns) of every tile id of t2v-turbo_amd/csrc/gemm.hip (kCfg)
GEMM_TILES = {1: (128, 128), 2: (128, 64), 3: (256, 64), 4: (128, 128), 5: (128, 64), 6: (256, 128), 7: (256, 128),
              8: (64, 128), 9: (256, 64), 10: (128, 128), 11: (128, 256), 12: (256, 256), 13: (256, 128), 14: (128, 256),
              15: (256, 256), 16: (256, 128), 17: (128, 256), 18: (128, 128), 19: (256, 128), 20: (256, 256),
              21: (256, 256), 22: (160, 320), 23: (160, 320), 24: (256, 256), 25: (256, 128), 26: (128, 128),
              27: (256, 256), 28: (160, 320), 29: (128, 256), 30: (128, 128), 31: (128, 128), 32: (128, 128), 33: (128, 128)}


def gemm_operand_gbyte(d, k_total):
    """Bytes one t2v_gemm launch moves from L2 into LDS: every workgroup tile streams its (BM + BN) x K bf16 panel pair
    once.  None when the launch runs on the library heuristic (tile id not recorded in the descriptor)."""
    tile = GEMM_TILES.get(int(d.tile_cfg))
    if tile is None:
        return None
    bm, bn = tile
    tiles = -(-d.M // bm) * -(-d.N // bn) * max(d.batch, 1)
    return tiles * (bm + bn) * k_total * 2 / 1e9


def kernel_breakdown(engine, plan, rec=None):
    """Replay the recorded launches with an event pair around each one (same stream the kernels run on)
    and aggregate per C-ABI entry point; GEMM launches carry their algorithmic FLOPs (2*M*N*K*batch)."""
    from t2v_turbo_amd import native as nt
    ops = engine.ops
    rec = plan["rec"] if rec is None else rec
    stream = ops.stream()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(rec) + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for i, (fn, args, name) in enumerate(rec):
        fn(*args, stream)
        evs[i + 1].record()
    torch.cuda.synchronize()
    agg, shapes = {}, {}
    for i, (fn, args, name) in enumerate(rec):
        ms = evs[i].elapsed_time(evs[i + 1])
        a = agg.setdefault(name, {"launches": 0, "ms": 0.0, "tflop": 0.0, "gbyte": 0.0})
        a["launches"] += 1
        a["ms"] += ms
        if name in GEMM_FAMILY:
            d = args[0]._obj
            taps = {nt.GEMM_LINEAR: 1, nt.GEMM_TCONV3: 3}.get(d.mode, 9)
            tf = 2.0 * d.M * d.N * taps * (d.c0 + d.c1) * max(d.batch, 1) / 1e12
            a["tflop"] += tf
            try:
                og = gemm_operand_gbyte(d, taps * (d.c0 + d.c1)) if name == "t2v_gemm" else None
            except Exception:  # noqa: BLE001 - a derived figure must never cost the bench line
                og = None
            if og is not None:  # launches on a tuned tile id: operand traffic into LDS and the time it took
                a["operand_gbyte"] = a.get("operand_gbyte", 0.0) + og
                a["operand_ms"] = a.get("operand_ms", 0.0) + ms
            sh = shapes.setdefault((d.mode if name == "t2v_gemm" else "halo", d.M, d.N, taps * (d.c0 + d.c1), max(d.batch, 1), d.act, d.c1 > 0),
                                   {"n": 0, "ms": 0.0, "tflop": 0.0})
            sh["n"] += 1
            sh["ms"] += ms
            sh["tflop"] += tf
        elif name == "t2v_attn_spatial":
            n_img, seq_q, seq_kv, heads = args[9], args[10], args[11], args[12]
            a["tflop"] += 4.0 * n_img * heads * seq_q * seq_kv * 64 / 1e12
        elif name == "t2v_attn_temporal":
            clips, frames, hw, heads = args[8], args[9], args[10], args[11]
            a["tflop"] += 4.0 * clips * hw * heads * frames * frames * 64 / 1e12
            a["gbyte"] += 4 * 2.0 * clips * frames * hw * heads * 64 / 1e9  # q, k, v in + out, bf16
        elif name in ("t2v_gn_stats", "t2v_gn_apply", "t2v_group_norm"):
            # algorithmic HBM bytes (bf16): statistics read x once, apply reads x and writes y; t2v_group_norm is both
            rows, ch = args[6] * args[7], args[1] + args[4]
            a["gbyte"] += {"t2v_gn_stats": 1, "t2v_gn_apply": 2, "t2v_group_norm": 3}[name] * 2.0 * rows * ch / 1e9
        elif name == "t2v_group_norm_cs":
            # the apply pass reads x and writes y (bf16); the statistics come from the producers' column statistics (fp32 (sum, sumsq)
            # per 32-row slab and channel = 1/8 of the tensor's bytes) instead of a second read of x
            rows, ch = args[8] * args[9], args[3] + args[6]
            a["gbyte"] += (2 * 2.0 + 8.0 / 32) * rows * ch / 1e9
        elif name == "t2v_gn_stats_cs":
            a["gbyte"] += (8.0 / 32) * args[4] * args[5] * (args[1] + args[3]) / 1e9
        elif name == "t2v_layernorm":
            a["gbyte"] += 2 * 2.0 * args[2] * args[3] / 1e9
    report = os.environ.get("T2V_SHAPE_REPORT")
    if report:
        rows = [{"mode": k[0], "M": k[1], "N": k[2], "K": k[3], "batch": k[4], "act": k[5], "concat": k[6], "n": v["n"],
                 "ms": round(v["ms"], 3), "tflops": round(v["tflop"] / (v["ms"] / 1e3), 1)}
                for k, v in sorted(shapes.items(), key=lambda kv: -kv[1]["ms"])]
        with open(report, "w") as f:
            json.dump(rows, f, indent=0)
    return agg


GEMM_FAMILY = ("t2v_gemm", "t2v_conv_halo", "t2v_linear_pr")   # the implicit-GEMM convolutions / linears: one descriptor type, 2 M N K FLOP each


def family_ingraph(engine, rec, names, replays=5):
    """In-graph time (ms per step) of the launches of ``rec`` whose entry point is in ``names``: those launches, in recorded order, captured
    into ONE hipGraph on the stream they run on and replayed — device time without the host's per-launch dispatch that an event pair
    around every eager launch measures (rounds 4 and 5: that figure stopped responding to kernel changes).  Best of ``replays``."""
    ops = engine.ops
    sel = [(fn, args) for fn, args, name in rec if name in names]
    if not sel:
        return None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fn, args in sel[:4]:
            fn(*args, ops.stream())
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            st = ops.stream()
            for fn, args in sel:
                fn(*args, st)
        g.replay()
        torch.cuda.synchronize()
        best = None
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
    torch.cuda.current_stream().wait_stream(side)
    del g
    return best


def gemm_traffic():
    """HBM-side bytes per t2v_gemm launch from the committed PMC passes (profiles/r0N_gemm_traffic.json: rocprofv3
    --pmc FETCH_SIZE and WRITE_SIZE in separate runs of this same step, gfx950 FETCH_SIZE x2 correction;
    tools/pmc_traffic.py).  Counters cannot be read from inside the timed process, so this is the profile's number,
    labelled as such; null when the profile is absent."""
    here = os.path.dirname(os.path.abspath(__file__))
    for name in ("r06_gemm_traffic.json", "r05_gemm_traffic.json", "r04_gemm_traffic.json", "r03_gemm_traffic.json", "r02_gemm_traffic.json", "r01_gemm_traffic.json"):  # the newest committed PMC passes
        try:
            with open(os.path.join(here, "profiles", name)) as f:
                g = json.load(f)["gemm"]
            return {"traffic": round(g["hbm_bytes_per_launch"]), "traffic_unit": "bytes per launch (L2-miss side, incl. Infinity-Cache hits)",
                    "traffic_source": "profiles/" + name}
        except Exception:  # noqa: BLE001
            continue
    return {"traffic": None}


def log(msg):
    print(f"[bench +{time.time() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


class Watchdog:
    """SIGALRM guard: an optional leg that overruns is abandoned (recorded in the JSON) instead of
    eating the whole run."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        import signal

        def fire(*_):
            raise TimeoutError(f"{self.what} exceeded {self.seconds}s")

        self.old = signal.signal(signal.SIGALRM, fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        import signal
        signal.alarm(0)
        signal.signal(signal.SIGALRM, self.old)
        return False


PARITY_TOL = 3e-2   # bf16 device path vs the fp32 oracle, end to end (the reference's own bf16-vs-fp32 gap is 2.2e-2)


def cpu_baseline(model, x, ctx, tc, frames_req):
    """The oracle (CPU restatement of the reference forward, pinned to reference goldens; /root/reference does not exist on
    the GPU box, and tools/cpu_reference_time.py shows the two run at the same speed where it does:
    profiles/r02_cpu_reference_timing.json) timed on this host's cores, BASELINE.md 3 style: 1 warm-up + 3 runs, median.
    The warm-up is ONE fp32 forward of the whole 16-frame clip, which is also the parity check of the GPU output at the
    size the metric is quoted on; the timed runs are whole 16-frame forwards too."""
    import statistics
    from oracle import unet_oracle as uo
    cores = os.cpu_count() or 1
    threads = min(cores, 64)  # torch CPU ops stop scaling (and can thrash) far below 256 threads
    torch.set_num_threads(threads)
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    ts = torch.tensor([999])
    cpu = dict(context=ctx.float().cpu(), fps=16, timestep_cond=tc.float().cpu())

    def run(f):
        xs = x[:, :, :f].float().cpu()
        t0 = time.time()
        y = uo.unet_forward(sd, VC2_UNET, xs, ts, cpu["context"], fps=16, timestep_cond=cpu["timestep_cond"])
        return time.time() - t0, y

    full = frames_req or 16
    t_warm, y = run(full)
    log(f"cpu oracle warm-up / parity run: {full} frames {t_warm:.1f}s on {threads} threads")
    with torch.no_grad():
        y_gpu = model(x[:, :, :full].contiguous(), ts.to(x.device), context=ctx, fps=16, timestep_cond=tc)
    parity = float((y_gpu.float().cpu() - y).double().norm() / y.double().norm())
    # time what is named: whole 16-frame forwards (3 of them when they fit ~100 s of CPU time, else one more besides the
    # warm-up); the 4-frame slice of earlier rounds under-counted by 7 % and is gone
    n_timed = 3 if t_warm * 3 < 100 else 1
    times = []
    for _ in range(n_timed):
        dt, _y = run(full)
        times.append(dt)
    med = statistics.median(times)
    log(f"cpu oracle timed runs ({full} frames): {[round(t, 1) for t in times]} s")
    return {"value": round((full / 16.0) / med, 5), "unit": "UNet steps/s", "cores": threads, "kind": "port",
            "runs_s": [round(t, 2) for t in times], "warmup_s": round(t_warm, 2),
            "sample": f"fp32 forward of oracle.unet_oracle (restated reference UNetModel.forward) on the whole (1,4,{full},40,64) "
                      f"latent: 1 warm-up ({t_warm:.1f} s, also the parity run) + {n_timed} timed run(s), median {med:.1f} s, torch CPU "
                      f"{threads} threads of {cores} cores",
            "parity_rel_l2_vs_gpu": parity, "parity_frames": full, "parity_tol": PARITY_TOL}


DISTILL_PARITY = {"out": 3e-2, "dx": 6e-2, "cos_min": 0.98, "norm_ratio": 0.12}   # bf16 device engine vs fp32 CPU autograd


def _new_student(cfg, dev, rank_r, seed=4321):
    """LoRA-injected student (fp32 master weights; zero-init tensors and the zero lora_up factors re-drawn: same on every rank)."""
    from t2v_turbo_amd import lora
    from t2v_turbo_amd.unet3d import UNetModel
    torch.manual_seed(seed)             # the default initialisers draw from the global generators: the parity figures of the leg must
    if dev.type == "cuda":              # not depend on what ran before it
        torch.cuda.manual_seed_all(seed)
    with torch.device(dev):
        student = UNetModel(**cfg)
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for p in student.parameters():
            if float(p.abs().max()) == 0.0:
                p.normal_(0.0, 0.02, generator=g)
    student.requires_grad_(False)
    lora.inject_trainable_lora_extended(student, r=rank_r)
    params = lora.lora_parameters(student)
    with torch.no_grad():  # lora_up starts at zero: give the down-projection gradients something to do
        for p in params:
            if float(p.abs().max()) == 0.0:
                p.normal_(0.0, 0.01, generator=g)
    return student, params


def distill_parity(student, params, sync, make_ops, cfg, dev, frames=4):
    """Parity gate of the distillation leg (exit code 3 on failure, like the inference leg): the student's forward + backward on
    the device gradient engine against fp32 CPU autograd (oracle/lora_grad_oracle.py) at the FULL widths on a bounded
    ``frames``-frame latent (the 16-frame comparison is tests/test_gpu_train_parity.py: ~3 min of CPU), eval mode — the
    train-mode masks are checked by the GPU suite.  Every LoRA tensor's gradient by cosine and norm ratio."""
    import statistics
    from oracle.lora_grad_oracle import per_tensor_agreement, student_reference
    from t2v_turbo_amd.engine_unet_bwd import UNetGradEngine
    t0 = time.time()
    was_training = student.training
    student.eval()
    try:
        gen = torch.Generator().manual_seed(11)
        h, w = (40, 64) if cfg["model_channels"] >= 320 else (8, 8)
        x = torch.randn(1, 4, frames, h, w, generator=gen)
        ctx = torch.randn(1, 77, cfg["context_dim"], generator=gen)
        tc = torch.randn(1, 256, generator=gen)
        r_out = torch.randn(x.shape, generator=gen)
        ts = torch.tensor([519])
        eng = UNetGradEngine(student, make_ops())
        eng.bind_lora(params)
        emb_all = student.conditioning_emb_all(ts.to(dev), 16, tc.to(dev))
        y = eng.forward_tape(x.to(dev), ts.to(dev), ctx.to(dev), 16, tc.to(dev), None, emb_all=emb_all)
        flat = torch.zeros(eng.lora_numel, device=dev)
        dx = eng.backward(r_out.to(dev), flat_grad=flat, accumulate=False)
        sync.zero_()                              # the conditioning branch's 27 leaves stay with torch autograd:
        emb_all.backward(eng.d_emb_all)           # their gradients land in the flat buffer's own slots
        flat = (flat + sync.flat).cpu()
        sync.zero_()
        del eng
        rank_r = max(p.shape[0] for p in params[1::2])
        y_ref, dx_ref, g_ref = student_reference(student.state_dict(), cfg, rank_r, x, ts, ctx, 16, tc, r_out,
                                                 threads=min(os.cpu_count() or 1, 64))
        grads, off = [], 0
        for p in params:
            grads.append(flat[off:off + p.numel()].view(p.shape))
            off += p.numel()
        rows, zeros = per_tensor_agreement(grads, g_ref)

        def rel(a, b):
            return float((a.double().cpu() - b.double()).norm() / b.double().norm())

        cs, qs = [r[1] for r in rows], [abs(r[2] - 1.0) for r in rows]
        out = {"frames": frames, "out_rel_l2": rel(y, y_ref), "dx_rel_l2": rel(dx, dx_ref), "lora_tensors": len(rows),
               "lora_grad_cos_min": min(cs), "lora_grad_cos_median": statistics.median(cs), "lora_grad_norm_ratio_max_dev": max(qs),
               "zero_reference_gradients": len(zeros), "tol": DISTILL_PARITY, "seconds": round(time.time() - t0, 1),
               "reference": "fp32 CPU autograd through the torch module (oracle/lora_grad_oracle.py, pinned to the reference's own "
                            "LoRA gradients: tests/golden/unet_tiny_lora_grad.npz)"}
        out["ok"] = bool(out["out_rel_l2"] <= DISTILL_PARITY["out"] and out["dx_rel_l2"] <= DISTILL_PARITY["dx"] and
                         out["lora_grad_cos_min"] >= DISTILL_PARITY["cos_min"] and
                         out["lora_grad_norm_ratio_max_dev"] <= DISTILL_PARITY["norm_ratio"] and
                         all(float(grads[i].abs().max()) < 1e-6 for i in zeros))
        return out
    finally:
        student.train(was_training)


def full_finetune_leg(dev, steps=5):
    """The FULL fine-tuning student (train_latent_t2v_turbo_v2.py:669,798-816,1262: every UNet parameter trainable, no LoRA) at full width on
    the bench latent, train mode: `unet(...)` + `loss.backward()` through the module route on the native gradient engine (engine_full.py),
    an SGD-style update of every weight between steps so that the in-place pack refresh is inside the timed region.  Correctness of this
    path: tests/test_gpu_train_parity.py::test_full_fine_tuning_* (the reference's own gradients at two widths; fp32 CPU autograd at
    full width).  Step 0 records the two launch lists, step 1 re-makes the packs eagerly, step 2 captures that refresh as one hipGraph
    (a one-time ~ 0.2 s, visible in `ms_all`), steps 3+ are the steady state: `ms_per_step` is their minimum."""
    import warnings
    m = build_model(dev, torch.float32)
    m.requires_grad_(True)
    m.train()
    x, ctx, tc = synth_inputs(dev, torch.float32)
    ts = torch.tensor([999], device=dev)
    params = list(m.parameters())
    times = []
    torch.cuda.reset_peak_memory_stats()
    for step in range(steps + 1):   # step 0 records the two launch lists
        for p_ in params:
            p_.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("error")    # the torch-composite route warns: it must not be taken
            y = m(x, ts, context=ctx, fps=16, timestep_cond=tc)
        y.float().pow(2).mean().backward()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        with torch.no_grad():
            for p_ in params:
                p_.add_(p_.grad, alpha=-1e-6)
    eng = m._engine_box.full
    plan = next(iter(eng.plans.values()))
    finite = all(p_.grad is not None and bool(torch.isfinite(p_.grad).all()) for p_ in params)
    out = {"ms_per_step": round(min(times[1:]), 1), "ms_all": [round(t, 1) for t in times[1:]], "record_ms": round(times[0], 1),
           "params_m": round(sum(p_.numel() for p_ in params) / 1e6, 1), "all_grads_finite": finite,
           "launches": {"forward": len(plan["rec"]), "backward": len(plan["rec_bwd"])}, "plans": len(eng.plans),
           "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
           "what": "forward + backward of every UNet parameter (no LoRA), train mode, latent (1,4,16,40,64), weights updated between steps; "
                   "ms_all[1] contains the one-time capture of the pack refresh as a hipGraph"}
    del m, params, eng, plan
    torch.cuda.empty_cache()
    return out


def distill_step_leg(teacher, dev, world=1, dry=False, parity=True):
    """BASELINE config C3: the v1 consistency-distillation step (train_t2v_turbo_v1_lora.py:978-1196) at full size, per-rank
    B=1 — LoRA r=64 student (fp32 master weights, train mode, bf16 engine) forward + target forward + backward on the native
    gradient engine, the two frozen-teacher forwards on the inference engine, ONE flat-buffer gradient all-reduce (RCCL at
    world > 1: train_t2v_turbo_v1_lora.py:1190 through accelerate/DDP in the reference), flat-buffer clip + fused AdamW.
    Runs on every rank; the timed region is bracketed by barrier + synchronize and the max over ranks is reported."""
    import torch.distributed as dist
    from t2v_turbo_amd import cd_math, dist as tdist
    from t2v_turbo_amd.distill import distill_step
    from t2v_turbo_amd.engine_unet_bwd import UNetGradEngine
    from t2v_turbo_amd.optim import FlatAdamW
    from t2v_turbo_amd.scheduler import T2VTurboScheduler
    cfg = dict(VC2_UNET, model_channels=64, context_dim=128) if dry else VC2_UNET
    if dry:
        from tests.emu_ops import EmuOps   # CPU plumbing check only (--dry-run-cpu): the emulated op backend of the test suite

        def make_ops():
            return EmuOps(strict=True)
    else:
        from t2v_turbo_amd.native import HipOps as make_ops
    rank = int(os.environ.get("RANK", "0"))
    cuda = dev.type == "cuda"
    student, params = _new_student(cfg, dev, 16 if dry else 64)
    student.train()
    sync = tdist.FlatGradSync(params)
    opt = FlatAdamW(params, sync, lr=1e-5)
    eng = UNetGradEngine(student, make_ops())
    eng.flash_attn_bwd = eng.tn_wgrad = True
    eng.bind_lora(params)
    sched = T2VTurboScheduler()
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=50).to(dev)
    gen = torch.Generator().manual_seed(rank)       # every rank its own clip: data parallel, per-rank batch 1
    shape = (1, 4, 2, 8, 8) if dry else (1, 4, 16, 40, 64)
    lat = torch.randn(shape, generator=gen).to(dev) * 0.18215
    pe = torch.randn(1, 77, cfg["context_dim"], generator=gen).to(dev)
    ue = torch.randn(1, 77, cfg["context_dim"], generator=gen).to(dev)

    # T2V_BATCH_TEACHER=1: the teacher's cond / uncond forwards as ONE call on the 2-clip batch (distill_step(batch_teacher=True): same
    # numbers per clip, weights read once); default off = two calls, the order of operations the reference has
    batch_teacher = os.environ.get("T2V_BATCH_TEACHER", "0") == "1"

    def step():
        return distill_step(student, teacher, solver, sched, lat, pe, ue, optimizer=opt, grad_sync=sync,
                            autocast_dtype=torch.bfloat16 if cuda else None, student_engine=eng, batch_teacher=batch_teacher)

    def fence():
        if world > 1:
            dist.barrier()
        if cuda:
            torch.cuda.synchronize()

    # Two ways of issuing the same launch lists: plain replay (a Python / ctypes loop over ~8 800 C-ABI calls per step: the step is
    # then as fast as the HOST can issue, 232-262 ms across the boxes of the pool) and hipGraph replay of the teacher's list and of
    # the student's forward / backward lists (the host is idle, the step is what the GPU needs).  Both are timed; ms_per_step is the
    # better one and says which.  At N > 1 the graphs keep the gradient exchange as one all-reduce after the backward (a captured
    # list cannot carry the host-side markers of the overlapped exchange).
    t_eng = None if dry else teacher.native_engine()
    modes = [("plain replay", False)] + ([] if dry else [("hipGraph replay", True)])
    timings = {}
    t_graph = None if t_eng is None else t_eng.use_graph
    # The reference never puts the v1 teacher in eval mode (train_t2v_turbo_v1_lora.py:621-626; forwards at :1105-1134), so its
    # TemporalConvBlock dropouts are live: the timed step runs the teacher in TRAIN mode, as the reference does (the inference
    # engine applies those dropouts as counter-based masks); the eval-mode figure of earlier rounds is reported beside it.
    teacher_was_training = teacher.training
    teacher.train()
    try:
        for label, graph in modes:
            if t_eng is not None:
                t_eng.use_graph = graph
            eng.use_graph = graph
            for _ in range(1 if dry else (3 if graph else 2)):   # (a list is captured on its second plain replay)
                loss, info = step()
            fence()
            t0 = time.perf_counter()
            n = 2 if dry else 5
            for _ in range(n):
                loss, info = step()
            fence()
            timings[label] = (time.perf_counter() - t0, info, len(getattr(eng, "_handles", None) or []))
        # the same step with an eval-mode teacher (what rounds 1-3 timed), in the better issue mode
        best_graph = dict(modes)[min(timings, key=lambda k: timings[k][0])]
        teacher.eval()
        if t_eng is not None:
            t_eng.use_graph = best_graph
        eng.use_graph = best_graph
        for _ in range(1 if dry else 3):
            step()
        fence()
        t0 = time.perf_counter()
        for _ in range(2 if dry else 5):
            step()
        fence()
        ms_eval_teacher = (time.perf_counter() - t0) / (2 if dry else 5) * 1e3
    finally:
        teacher.train(teacher_was_training)
        if t_eng is not None:
            t_eng.use_graph = t_graph
        eng.use_graph = False
    best = min(timings, key=lambda k: timings[k][0])
    dt, info, n_segments = timings[best]
    if world > 1:
        tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    ms = dt / n * 1e3
    # the exchange by itself: the same all-reduce of the flat gradient buffer, timed in isolation (it is inside ms_per_step too)
    ar_ms = None
    if world > 1:
        fence()
        t0 = time.perf_counter()
        for _ in range(3):
            sync.all_reduce_mean()
        fence()
        ar_ms = (time.perf_counter() - t0) / 3 * 1e3
        sync.zero_()
    plan = eng._last
    out = {"ms_per_step": round(ms, 1), "issue": best,
           "ms_per_step_by_issue": {k: round(v[0] / n * 1e3, 1) for k, v in timings.items()},
           "samples_per_s": round(world * 1e3 / ms, 3), "n_gpus": world, "per_rank_batch": 1,
           "loss": float(loss.detach()),
           "finite": bool(torch.isfinite(sync.flat).all() and torch.isfinite(opt.flat_param).all()),
           "lora_params_m": round(sync.numel / 1e6, 1), "student": "native gradient engine (flash attention backward, token-contracted "
           "weight gradients), train mode",
           "teacher": ("1 forward of the [cond | uncond] 2-clip batch" if batch_teacher else "2 forwards") +
                      " on the inference engine, TRAIN mode (TemporalConvBlock dropouts live, as the reference runs its teacher)",
           "ms_per_step_eval_teacher": round(ms_eval_teacher, 1),
           "grad_exchange": ("gradient arena all-reduced in %d segments from inside the backward (%.1f MB fp32, backend %s) + the "
                             "conditioning branch's tensors after it; allreduce_ms = ONE blocking all-reduce of the whole flat "
                             "buffer, timed separately, for scale" % (n_segments, eng.e_used * 4 / 2 ** 20, dist.get_backend())
                             if n_segments else
                             "one all-reduce(mean) of the flat fp32 LoRA gradient buffer, %.1f MB, backend %s"
                             % (sync.numel * 4 / 2 ** 20, dist.get_backend())) if world > 1 else "none (1 rank)",
           "allreduce_ms": None if ar_ms is None else round(ar_ms, 3),
           "launches": {"student_forward": len(plan["rec"]), "student_backward": len(plan["rec_bwd"])} if "rec" in plan else None,
           "host_ms_last_step": info.get("host_ms"),
           "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1) if cuda else None}
    if rank != 0:
        return out
    if cuda:
        try:
            with torch.no_grad():
                fwd = kernel_breakdown(eng, plan, plan["rec"])
                plan["static"]["dout"].normal_()
                bwd = kernel_breakdown(eng, plan, plan["rec_bwd"])
            for tag, agg in (("forward", fwd), ("backward", bwd)):
                out[tag + "_ms"] = round(sum(v["ms"] for v in agg.values()), 2)
                out[tag + "_gemm_tflop"] = round(agg.get("t2v_gemm", {}).get("tflop", 0.0), 2)
                out[tag + "_kernel_ms"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 2)}
                                           for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])[:12]}
        except Exception as e:  # noqa: BLE001 - a derived table must not cost the measured number
            out["breakdown_error"] = repr(e)
    if parity and world == 1:
        del eng, plan
        try:
            out["parity"] = distill_parity(student, params, sync, make_ops, cfg, dev)
        except Exception as e:  # noqa: BLE001 - an unverifiable step is reported as a parity failure, not as a number
            out["parity"] = {"ok": False, "error": repr(e)}
    return out


def dump_outputs(out_dir, arrays):
    """--dump-outputs: what the timed path returned in its last step, as float32 .npy files.  Weights and inputs come from fixed
    seeds, so two builds run with the same arguments can be compared output for output."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())
    log(f"outputs of the last timed step written to {out_dir}: {sorted(arrays)}")


def self_spawn(n):
    """`python bench.py --gpus N` from a plain shell: re-execute under torch.distributed.run, one rank per GPU."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("self-spawn: " + " ".join(cmd))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this driver
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graph", type=int, default=1, help="replay the recorded forward as one hipGraph")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg below whose switch is not given: breakdown, clips, CPU baseline, distillation, full fine-tuning")
    ap.add_argument("--cpu-baseline", type=int, default=None, help="time the CPU oracle and gate on its parity (N = 1; default: --full)")
    ap.add_argument("--cpu-frames", type=int, default=0, help="frames in the CPU sample (0 = the whole 16-frame clip)")
    ap.add_argument("--clip", type=int, default=None, help="also time the 4-step clip and the 16-step v2 clip incl. VAE decode (default: --full)")
    ap.add_argument("--breakdown", type=int, default=None, help="per-kernel times and the GEMM-family roofline (default: --full)")
    ap.add_argument("--distill", type=int, default=None,
                    help="also time the v1 distillation step (config C3; on every rank at N > 1; default: --full)")
    ap.add_argument("--distill-parity", type=int, default=1, help="gate the distillation leg on its gradient parity check (N = 1)")
    ap.add_argument("--full-finetune", type=int, default=None,
                    help="also time the full fine-tuning student step (v2 script's call pattern; rank 0, N = 1; default: --full)")
    ap.add_argument("--dry-run-cpu", type=int, default=0, help="plumbing check on CPU: tiny widths, gloo, emulated kernels (not a measurement)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the UNet output of the last timed step as DIR/unet_out.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    for leg in ("breakdown", "clip", "cpu_baseline", "distill", "full_finetune"):
        if getattr(args, leg) is None:
            setattr(args, leg, int(args.full))

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:   # plain `python bench.py --gpus N`: become N ranks
        sys.exit(self_spawn(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dry = bool(args.dry_run_cpu)
    import torch.distributed as dist
    if dry:
        torch.set_num_threads(max(1, (os.cpu_count() or 2) // max(world, 1) // 2))
        if world > 1:
            dist.init_process_group("gloo")
        dev, dtype = torch.device("cpu"), torch.float32
    else:
        assert torch.cuda.is_available(), "bench.py needs a GPU (MI355X); --dry-run-cpu 1 only checks the plumbing"
        if world > 1:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        torch.cuda.set_device(local)
        dev, dtype = torch.device("cuda", local), torch.bfloat16

    log("building model")
    if dry:
        from t2v_turbo_amd.unet3d import UNetModel
        torch.manual_seed(1234)
        model = UNetModel(**dict(VC2_UNET, model_channels=64, context_dim=128)).eval()
        with torch.no_grad():
            for p in model.parameters():
                if float(p.abs().max()) == 0.0:
                    p.normal_(0.0, 0.02)
        g0 = torch.Generator().manual_seed(0)
        x, ctx = torch.randn(1, 4, 2, 8, 8, generator=g0), torch.randn(1, 77, 128, generator=g0)
        from t2v_turbo_amd.nn_util import guidance_embedding
        tc = guidance_embedding(torch.tensor([7.5]), 256)
    else:
        model = build_model(dev, dtype)
        x, ctx, tc = synth_inputs(dev, dtype)
    log("model built")
    eng = None if dry else model.native_engine()
    if eng is not None:
        eng.use_graph = bool(args.graph)
    table = [999, 759, 519, 279]
    ts = [torch.tensor([t], device=dev, dtype=torch.long) for t in table]

    def step(i):
        return model(x, ts[i % 4], context=ctx, fps=16, timestep_cond=tc)

    def barrier():
        if world > 1:
            dist.barrier()
        if not dry:
            torch.cuda.synchronize()

    with torch.no_grad():
        step(0)  # recording pass (also packs weights)
        log("plan recorded")
        for i in range(max(args.warmup, 2)):  # >= 2: the second call captures the graph
            step(i)
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            y = step(i)
        barrier()
        elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"unet_out": y})
    del y
    ms_per_step = elapsed / args.steps * 1e3
    value = world * args.steps / elapsed

    result = {
        "metric": "UNet denoise steps/sec (16f 320x512 latent)", "value": round(value, 4), "unit": "steps/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": "VideoCrafter2 UNet forward, B=1 per GPU, latent (1,4,16,40,64), ctx (1,77,1024), "
                               "4-step LCM timestep table, random-init weights (zero-init tensors re-drawn)",
                   "parallelism": f"replicas x{world}", "hip_graph": bool(args.graph)},
        "tflops_per_gpu": round(UNET_TFLOP_PER_STEP / (ms_per_step / 1e3), 2),
    }
    if dry:
        result.update(dtype="f32", data="CPU DRY RUN of the launch path (tiny widths, latent (1,4,2,8,8), gloo, emulated kernels): "
                                        "plumbing only, NOT a measurement", tflops_per_gpu=None)
        result["config"]["workload"] = "dry run: tiny UNet forward on CPU"
    if rank == 0 and not dry:
        plan = next(iter(eng.plans.values()))
        result["config"]["graph_captured"] = plan.get("graph") is not None
        result["config"]["launches_per_step"] = len(plan["rec"])
        result["config"]["workspace_gb"] = round(plan["pool_bytes"] / 2 ** 30, 3)
        if args.breakdown:
            with torch.no_grad():
                agg = kernel_breakdown(eng, plan)
            zero = {"ms": 0.0, "tflop": 0.0, "launches": 0}
            g0, h0, l0 = agg.get("t2v_gemm", zero), agg.get("t2v_conv_halo", zero), agg.get("t2v_linear_pr", zero)
            # the dominant kernel FAMILY: the implicit-GEMM convolutions / linears — t2v_gemm, t2v_conv_halo (3x3 convs of the three upper
            # levels since round 4) and t2v_linear_pr (short-K GEGLU / q|k|v launches since round 6): algorithmic FLOPs of all three over
            # their IN-GRAPH time (the family's launches captured into one hipGraph and replayed: family_ingraph); the per-launch
            # event times of the eager replay stay in by_kernel / kernel_ms as `ms_eager`
            gm = dict(g0, tflop=g0["tflop"] + h0["tflop"] + l0["tflop"], launches=g0["launches"] + h0["launches"] + l0["launches"],
                      ms_eager=g0["ms"] + h0["ms"] + l0["ms"])
            try:   # (a derived figure must never cost the bench line: a failed capture falls back to the eager event times, labelled)
                with torch.no_grad():
                    fam_ms = family_ingraph(eng, plan["rec"], GEMM_FAMILY)
                    one_ms = {n: family_ingraph(eng, plan["rec"], (n,)) for n in GEMM_FAMILY}
            except Exception as e:  # noqa: BLE001
                log(f"in-graph family timing failed ({e!r}): roofline from the eager per-launch events")
                fam_ms, one_ms = None, {}
            gm["ms"] = fam_ms if fam_ms else gm["ms_eager"]
            ach = gm["tflop"] / (gm["ms"] / 1e3) if gm["ms"] > 0 else 0.0

            def one(n, a):
                ms = one_ms.get(n)
                return {"launches": a["launches"], "ms": None if ms is None else round(ms, 3), "ms_eager": round(a["ms"], 3),
                        "tflops": round(a["tflop"] / (ms / 1e3), 1) if ms else None}
            result["roofline"] = {
                "kernel": "gemm_kernel + conv_halo_kernel + linear_pr_kernel (implicit-GEMM conv / linear: v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16)",
                "bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(ach / MFMA_PEAK_TFLOPS, 4), **gemm_traffic(),
                "timing": ("in-graph: the family's launches of one step captured into one hipGraph on their stream, best of 5 replays (HIP events)"
                           if fam_ms else "eager replay, one HIP event pair per launch (the in-graph capture failed on this box)"),
                "launches": gm["launches"], "tflop_per_step": round(gm["tflop"], 3), "ms_per_step": round(gm["ms"], 3),
                "ms_per_step_eager_events": round(gm["ms_eager"], 3),
                "whole_step_frac": round(UNET_TFLOP_PER_STEP / (ms_per_step / 1e3) / MFMA_PEAK_TFLOPS, 4),
                "by_kernel": {"t2v_gemm": one("t2v_gemm", g0), "t2v_conv_halo": one("t2v_conv_halo", h0), "t2v_linear_pr": one("t2v_linear_pr", l0)},
            }
            if gm.get("operand_ms"):  # the rate the kernel is actually bound by
                result["roofline"]["operand_delivery"] = {
                    "gbyte_per_step": round(gm["operand_gbyte"], 2), "ms": round(gm["operand_ms"], 3),
                    "tb_per_s": round(gm["operand_gbyte"] / gm["operand_ms"], 2),
                    "what": "tile panels streamed L2 -> LDS: sum over launches of tiles x (BM + BN) x K x 2 bytes / their time; "
                            "the fill path itself delivers 13.9-17 TB/s by LDS-DMA and 18-29 TB/s register-staged on an L2-resident "
                            "window (profiles/r02_fill_rate.txt): not the bound"}
            result["kernel_ms"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3), "tflop": round(v["tflop"], 3),
                                       **({"gbyte": round(v["gbyte"], 3), "gb_per_s": round(v["gbyte"] / (v["ms"] / 1e3), 1)}
                                          if v.get("gbyte") else {})}
                                   for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])}
        log(f"timed region done: {ms_per_step:.2f} ms/step")
        if args.clip and world == 1:
            try:
                with Watchdog(150, "4-step clip leg"):
                    result["clip_4step"] = clip_wallclock(model, dev, dtype)
            except Exception as e:  # noqa: BLE001 - optional leg, reported not fatal
                result["clip_4step"] = {"error": repr(e)}
            log(f"clip leg: {result['clip_4step']}")
            try:
                with Watchdog(150, "16-step v2 clip leg"):
                    result["clip_16step_v2"] = clip_v2_wallclock(dev, dtype)
            except Exception as e:  # noqa: BLE001
                result["clip_16step_v2"] = {"error": repr(e)}
            log(f"v2 clip leg: {result['clip_16step_v2']}")
        if args.cpu_baseline and world == 1:
            try:
                with Watchdog(300, "cpu baseline leg"):
                    result["cpu_baseline"] = cpu_baseline(model, x, ctx, tc, args.cpu_frames)
            except Exception as e:  # noqa: BLE001
                result["cpu_baseline"] = {"error": repr(e)}
            log(f"cpu baseline leg: {result['cpu_baseline']}")
    # the distillation step (config C3) runs on EVERY rank: at N > 1 it carries the real gradient all-reduce
    if args.distill:
        try:
            with Watchdog(420, "distillation step leg"):
                d = distill_step_leg(model, dev, world=world, dry=dry, parity=bool(args.distill_parity))
        except Exception as e:  # noqa: BLE001
            if world > 1:
                raise   # a rank that drops out of a collective leg must not leave the others waiting silently
            d = {"error": repr(e)}
        if rank == 0:
            result["distill_step"] = d
            log(f"distill leg: {d}")
    if args.full_finetune and rank == 0 and world == 1 and not dry:
        try:
            with Watchdog(240, "full fine-tuning leg"):
                result["full_finetune_step"] = full_finetune_leg(dev)
        except Exception as e:  # noqa: BLE001 - optional leg, reported not fatal
            result["full_finetune_step"] = {"error": repr(e)}
        log(f"full fine-tuning leg: {result['full_finetune_step']}")
    rc = 0
    if rank == 0:
        print(json.dumps(result), flush=True)
        par = result.get("cpu_baseline", {}).get("parity_rel_l2_vs_gpu")
        if par is not None and not par <= PARITY_TOL:  # a fast wrong answer is not a result
            log(f"PARITY FAILURE: rel-L2 {par:.3e} vs the oracle exceeds {PARITY_TOL}")
            rc = 3
        dpar = result.get("distill_step", {}).get("parity")
        if dpar is not None and not dpar.get("ok", False):
            log(f"PARITY FAILURE (distillation leg: student forward / backward vs fp32 CPU autograd): {dpar}")
            rc = 3
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    sys.exit(rc)


def clip_v2_wallclock(dev, dtype):
    """BASELINE config C4: T2V-Turbo-v2 sampling — 16 steps on the 200-step grid with the motion-guidance embedding (`unet_mg`:
    motion_cond_proj_dim = 256, switched off below the percentage threshold: pipeline/t2v_turbo_vc2_pipeline.py:190-204) +
    16-frame VAE decode -> (1,3,16,320,512).  Full-width parity of the motion-conditioned forward: tests/test_gpu_engine.py."""
    from t2v_turbo_amd.pipeline import T2VTurboVC2Pipeline, make_synthetic_t2v
    from t2v_turbo_amd.unet3d import UNetModel
    cfg = dict(VC2_UNET, motion_cond_proj_dim=256)
    torch.manual_seed(1234)
    with torch.device(dev):
        unet = UNetModel(**cfg)
    g = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for p_ in unet.parameters():
            if float(p_.abs().max()) == 0.0:
                p_.normal_(0.0, 0.02, generator=g)
    unet = unet.to(dtype).eval()
    unet.dtype = dtype
    unet.native_engine().use_graph = True
    pipe = T2VTurboVC2Pipeline(make_synthetic_t2v(unet, dev, dtype), None, {"params": {"unet_config": {"params": cfg}}})
    pe = torch.randn(1, 77, 1024, generator=torch.Generator().manual_seed(0)).to(dev, dtype)
    times = []
    for it in range(4):
        gen = torch.Generator(device=dev).manual_seed(42)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vid = pipe(prompt=None, height=320, width=512, frames=16, fps=16, guidance_scale=7.5, motion_gs=0.1, use_motion_cond=True,
                   percentage=0.3, num_inference_steps=16, lcm_origin_steps=200, prompt_embeds=pe, generator=gen, output_type="pt")
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(min(times[1:]), 2), "ms_all": [round(t, 2) for t in times], "unet_steps": 16, "video_shape": list(vid.shape),
            "finite": bool(torch.isfinite(vid.float()).all()),
            "workload": "16 UNet steps (motion_cond on for t >= 700) + fused scheduler steps + 16-frame VAE decode"}


def clip_wallclock(model, dev, dtype):
    """4 UNet steps + scheduler + 16-frame VAE decode -> (1,3,16,320,512), prompt embeds given."""
    try:
        from t2v_turbo_amd.pipeline import T2VTurboVC2Pipeline, make_synthetic_t2v
    except Exception as e:  # pipeline not built yet in this revision
        return {"error": f"pipeline unavailable: {e}"}
    t2v = make_synthetic_t2v(model, dev, dtype)
    pipe = T2VTurboVC2Pipeline(t2v, None, {"params": {"unet_config": {"params": VC2_UNET}}})
    g = torch.Generator().manual_seed(0)
    pe = torch.randn(1, 77, 1024, generator=g).to(dev, dtype)
    times = []
    log("clip leg: VAE built")
    for it in range(3):
        gen = torch.Generator(device=dev).manual_seed(42)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vid = pipe(prompt=None, height=320, width=512, frames=16, fps=16, guidance_scale=7.5, num_inference_steps=4,
                   lcm_origin_steps=50, prompt_embeds=pe, generator=gen, output_type="pt")
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        log(f"clip leg: iteration {it} {times[-1]:.1f} ms")
    out = {"ms": round(min(times), 2), "ms_all": [round(t, 2) for t in times], "video_shape": list(vid.shape),
           "finite": bool(torch.isfinite(vid.float()).all())}
    # parity of the decode at the size it is timed on: one frame of latents at the scale the sampler hands over, device engine
    # (bf16) against the fp32 oracle on the same random-init VAE (oracle.vae_oracle; ~4 s of CPU) — not inside the timed region
    try:
        from oracle import vae_oracle as vo
        vae = t2v.first_stage_model
        gz = torch.Generator().manual_seed(5)
        z = torch.randn(1, 4, 1, 40, 64, generator=gz) * 0.18215 * 4.0
        sd = {k: v.detach().float().cpu() for k, v in vae.state_dict().items()}
        dd = dict(double_z=True, z_channels=4, resolution=512, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
                  attn_resolutions=[], dropout=0.0)
        ref = vo.decode_first_stage_2dae(sd, dd, z)
        with torch.no_grad():
            v = vae.decode_video(z.to(dev, dtype))
        out["parity_rel_l2"] = float((v.float().cpu() - ref).double().norm() / ref.double().norm())
        out["parity_what"] = "VAE decode of one (1,4,1,40,64) latent frame, device engine (bf16) vs oracle.vae_oracle (fp32), same weights"
        out["parity_tol"] = PARITY_TOL
        # roofline of the decode by itself: 25.02 TFLOP for 16 frames, HIP-event time of one 16-frame decode
        zs = torch.randn(1, 4, 16, 40, 64, generator=gz).to(dev, dtype) * 0.18215 * 4.0
        with torch.no_grad():
            vae.decode_video(zs)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                vae.decode_video(zs)
            e1.record()
        torch.cuda.synchronize()
        dec_ms = e0.elapsed_time(e1) / 3
        out["vae_decode_roofline"] = {"bound": "mfma", "tflop": VAE_DECODE_TFLOP_16F, "ms": round(dec_ms, 2),
                                      "achieved": round(VAE_DECODE_TFLOP_16F / (dec_ms / 1e3), 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                      "frac": round(VAE_DECODE_TFLOP_16F / (dec_ms / 1e3) / MFMA_PEAK_TFLOPS, 4)}
    except Exception as e:  # noqa: BLE001 - a derived figure must not cost the measured number
        out["parity_error"] = repr(e)
    return out


if __name__ == "__main__":
    main()
