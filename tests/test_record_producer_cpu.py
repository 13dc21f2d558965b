"""``preprocess.make_latent_records`` on the CPU (the torch twin, fp32) against the record the REFERENCE computed
(tests/golden/record_tiny.npz, tests/golden/make_golden_record.py), and the records' way to ``LatentRecordDataset``.

Bound against the fixture: per element |record - ref| <= ulp_fp16(ref) / 2 + 1e-5 * max |ref| — the twin is fp32 math on the CPU followed
by one fp16 rounding; the second term is for the other operation order of fp32 sums in two implementations of the same network."""
import os

import pytest
import torch

from oracle.synth import synth_state_dict
from t2v_turbo_amd import cd_head, cd_math, latent_io, preprocess
from t2v_turbo_amd.scheduler import T2VTurboScheduler
from tests.cd_head_cases import ulp
from tests.util import load, manifest, tiny_unet_params

TENSORS = preprocess.RECORD_TENSORS


def golden_inputs(dev="cpu", dtype=torch.float32):
    g = load("record_tiny")
    B = g["latents"].shape[0]
    return g, dict(latents=g["latents"].to(dev, dtype), prompt_embeds=g["prompt_emb"].to(dev, dtype),
                   uncond_prompt_embeds=g["uncond_prompt_embeds"].repeat(B, 1, 1).to(dev, dtype))


def check_against_fixture(name, got, ref):
    """The bound of the module docstring; ``got`` fp16, ``ref`` fp32."""
    err = (got.double() - ref.double()).abs()
    slack = err - (ulp(ref, torch.float16) / 2 + 1e-5 * float(ref.abs().max()))
    print(f"{name}: max err {float(err.max()):.3e}, worst excess over the bound {float(slack.max()):.3e} (max|ref| {float(ref.abs().max()):.3e})")
    assert float(slack.max()) <= 0.0, (name, float(slack.max()))


@pytest.fixture(scope="module")
def setup():
    from t2v_turbo_amd.unet3d import UNetModel
    m = UNetModel(**tiny_unet_params(record_attn_probs=True)).eval()
    m.load_state_dict(synth_state_dict(manifest("unet_tiny")), strict=True)
    m.requires_grad_(False)
    sched = T2VTurboScheduler(linear_start=0.00085, linear_end=0.012)
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=50)
    g, inputs = golden_inputs()
    return m, sched, solver, g, inputs


@pytest.fixture(scope="module")
def produced(setup):
    m, sched, solver, g, inputs = setup
    rng = dict(index=g["index"], noise=g["noise"])
    out = {}
    for motion in (True, False):
        out[motion] = preprocess.make_latent_records(m, solver, sched, **inputs, motion=motion, fps=int(g["fps"]),
                                                     temp_loss_scale=float(g["temp_loss_scale"]), text=["a cat", "a dog"], rng=rng)
    return out


@pytest.mark.parametrize("motion", [True, False])
def test_twin_reproduces_the_reference_record(setup, produced, motion):
    g = setup[3]
    blobs, info = produced[motion]
    assert len(blobs) == 2 and info["native"] is False and torch.equal(info["index"], g["index"])
    zero_keys = () if motion else ("score", "z_example", "z_example_prev")
    for b, blob in enumerate(blobs):
        rec = latent_io.unpack_latent_record(blob)
        assert set(latent_io.RECORD_KEYS) <= set(rec) and (("text" in rec) == (not motion))
        if not motion:
            assert rec["text"] == ["a cat", "a dog"][b]
        idx = rec["index"]
        assert isinstance(idx, torch.Tensor) and idx.dim() == 0 and idx.dtype == torch.int64 and int(idx) == int(g["index"][b])
        cd_head.check_index(idx.reshape(1), 50)
        for k in TENSORS:
            t = rec[k]
            assert t.dtype == torch.float16 and t.device.type == "cpu" and t.shape == g[k][b].shape, k
            if k in zero_keys:
                assert not bool(t.any()), k
            else:
                check_against_fixture(f"{k}[{b}] motion={motion}", t, g[k][b])
        # a per-clip view pickled as it is would carry the whole batch's storage
        numel = sum(rec[k].numel() for k in TENSORS)
        assert len(blob) <= 2 * numel + 8192, (len(blob), numel)
    # clip 1 has index 0: its z_example_prev is the original latent
    if motion:
        rec = latent_io.unpack_latent_record(blobs[1])
        assert torch.equal(rec["z_example_prev"], g["latents"][1].half())


def test_drawn_index_is_in_the_scripts_range_and_valid(setup):
    m, sched, solver, g, inputs = setup
    gen = torch.Generator().manual_seed(5)
    for motion, lo, hi in ((True, 25, 50), (False, 0, 25)):
        for _ in range(20):
            index, noise = preprocess._draw(solver, inputs["latents"], motion, 0.5, {}, gen)
            assert index.dtype == torch.int64 and index.shape == (2,) and noise.shape == inputs["latents"].shape
            assert lo <= int(index.min()) and int(index.max()) < hi
            cd_head.check_index(index, 50)
    with pytest.raises(ValueError):
        preprocess._draw(solver, inputs["latents"], True, 0.5, {"index": torch.tensor([3, 50])}, gen)


def test_a_teacher_that_is_not_frozen_is_refused(setup):
    m, sched, solver, g, inputs = setup
    m.train()
    try:
        with pytest.raises(ValueError):
            preprocess.make_latent_records(m, solver, sched, **inputs)
    finally:
        m.eval()


@pytest.mark.parametrize("motion", [True, False])
def test_written_records_come_back_through_the_dataset(tmp_path, produced, motion):
    blobs, _ = produced[motion]
    texts = ["a cat", "a dog"]
    relpaths = ["clips/a/0001.pkl", "clips/b/0002.pkl"]
    csv_path = os.path.join(tmp_path, "latents.csv")
    preprocess.write_latent_records(str(tmp_path), "latent_root", relpaths, blobs, texts, csv_path)
    ds = latent_io.LatentRecordDataset(csv_path, latent_root="latent_root", root_dir=str(tmp_path))
    ds.MAX_RETRIES = 1          # (a fault must surface, not be resampled away)
    assert len(ds) == 2
    for i, blob in enumerate(blobs):
        rec, sample = latent_io.unpack_latent_record(blob), ds[i]
        assert sample["txt"] == texts[i] and sample["use_motion_guide"] is True
        assert torch.equal(sample["index"], rec["index"])
        for k in TENSORS:
            assert torch.equal(sample[k], rec[k]), k


def test_kernel_twins_in_float64_are_the_schedulers_own_functions(setup):
    """The ``*_torch`` twins the kernel tests use as yardstick, against ``scheduler.add_noise`` and ``DDIMSolver.ddim_reverse_step``."""
    m, sched, solver, g, inputs = setup
    x, noise, index = g["latents"].double(), g["noise"].double(), g["index"]
    want = sched.add_noise(x, noise, solver.ddim_timesteps[index])
    assert torch.allclose(preprocess.add_noise_torch(solver, sched.alphas_cumprod, index, x, noise), want, rtol=1e-12, atol=0)
    import copy
    s64 = copy.copy(solver).to("cpu", torch.float64)
    ts = solver.ddim_timesteps[torch.tensor([0])]
    got, prev = preprocess.ddim_reverse_step_torch(solver, sched.alphas_cumprod, index, 0, x, noise, torch.zeros_like(x))
    assert torch.allclose(got, s64.ddim_reverse_step(x, noise, ts), rtol=1e-12, atol=0)
    assert torch.equal(prev[1], x[1]) and not bool(prev[0].any())          # index [3, 0]: step 0 is clip 1's last
    got1, _ = preprocess.ddim_reverse_step_torch(solver, sched.alphas_cumprod, index, 1, x, noise)
    assert torch.equal(got1[1], x[1]) and not torch.equal(got1[0], x[0])
