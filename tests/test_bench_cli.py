"""`python bench.py --gpus N` from a plain shell must become N ranks (self-spawn under torch.distributed.run) and, with `--full`,
run the distillation leg on every rank with the real flat-buffer all-reduce.  Checked here on CPU with the bench's own dry-run mode
(tiny widths, gloo, emulated kernels): the launch / rendezvous / collective plumbing of the path the driver takes on an 8-GPU node."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus_2_self_spawns_two_ranks_and_all_reduces():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-cpu", "1", "--full", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "rank 0 prints exactly ONE JSON line"
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["scaling"] == "weak" and "DRY RUN" in out["data"]
    d = out["distill_step"]
    assert d["n_gpus"] == 2 and d["finite"] and d["allreduce_ms"] > 0 and "gloo" in d["grad_exchange"]
    assert abs(d["samples_per_s"] - 2e3 / d["ms_per_step"]) < 1e-2 * d["samples_per_s"] + 1e-3   # global = ranks x per-rank


def test_bench_steps_and_dump_outputs_are_reproducible(tmp_path):
    """`--steps K` sets the number of timed steps reported in the line next to `ms_per_step`, and `--dump-outputs DIR` writes the
    last timed step's UNet output as float32; two runs with the same arguments dump the same array (seeded weights and inputs).
    A plain run (no `--full`) runs none of the extra legs."""
    import numpy as np
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-run-cpu", "1",
                            "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        assert not {"distill_step", "full_finetune_step", "roofline", "kernel_ms", "clip_4step", "cpu_baseline"} & set(out)
        assert abs(out["value"] - 1e3 / out["ms_per_step"]) < 1e-2 * out["value"]
        assert sorted(p.name for p in d.iterdir()) == ["unet_out.npy"]
        y = np.load(d / "unet_out.npy")
        assert y.dtype == np.float32 and y.shape == (1, 4, 2, 8, 8) and np.isfinite(y).all() and np.abs(y).max() > 0
        dumps.append(y)
    assert np.array_equal(dumps[0], dumps[1])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run-cpu", "1", "--steps", "0"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--steps" in r.stderr
