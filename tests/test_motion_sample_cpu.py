"""``motion_prior.motion_prior_sample`` on the CPU (the torch twin, fp32) against the run the REFERENCE computed
(tests/golden/motion_sample_tiny.npz, tests/golden/make_golden_motion_sample.py; its inputs are those of record_tiny.npz).

Bounds, none taken from what the code gives:
  * the head twin in float64 on the fixture's own tensors: 1e-5 * max |ref| (both sides are fp32 arithmetic on the same inputs; the
    figure at which the oracle is pinned to its fixtures);
  * the twin sampler restarted in front of a step: a step is linear in the two network outputs and the score,
        x' = (sqrt(ap) / a) x + Bg ((1 + w) cond - w uncond) - sqrt(1 - ap) sqrt(1 - a) score,   Bg = sqrt(1 - ap) - sqrt(ap) sg / a,
    so with d(t) = 1e-5 * max |t| per tensor — the term tests/test_record_producer_cpu.py allows two fp32 implementations of the same
    network on the teacher outputs and the score (its other term is the record's fp16 rounding, which is not made here) —
        |x' - ref| <= |Bg| ((1 + w) d(cond) + w d(uncond)) + sqrt(1 - ap) sqrt(1 - a) d(score) + 1e-5 max |ref|;
    max |t| is read from the tensors of the run (they differ from the reference's by that same 1e-5);
  * a cached ``motion_intermediate``: a guided step that runs on a cached entry does not read the state at all, so after the last
    guided step the latent differs from the producing run's by the fp16 rounding of the entry's five tensors through the same
    coefficients (half an fp16 ulp each) plus fp32 rounding."""
import os
import pickle

import numpy as np
import pytest
import torch
import yaml

from oracle.synth import synth_state_dict
from t2v_turbo_amd import cd_math
from t2v_turbo_amd import motion_prior as mp
from t2v_turbo_amd.scheduler import T2VTurboScheduler
from tests.cd_head_cases import ulp
from tests.util import VAE_TINY_DD, load, manifest, rel_l2, tiny_unet_params


def golden(dev="cpu", dtype=torch.float32):
    """(fixture, keyword-free inputs of ``motion_prior_sample`` for both clips)."""
    g, r = load("motion_sample_tiny"), load("record_tiny")
    sums = [float(r[k].double().sum()) for k in ("latents", "prompt_emb", "uncond_prompt_embeds", "noise")]
    assert np.allclose(sums, g["input_sums"].numpy(), rtol=1e-12), "record_tiny.npz is not the one the fixture was made from"
    fps = int(g["fps"])
    prompts, B = r["prompt_emb"].to(dev, dtype), r["latents"].shape[0]
    ctx = dict(inference={"context": prompts.flip(0), "fps": fps}, original={"context": prompts, "fps": fps},
               uncond={"context": r["uncond_prompt_embeds"].repeat(B, 1, 1).to(dev, dtype), "fps": fps})
    n = int(g["num_ddim"])
    inverted = [None] * n
    for j, i in enumerate((5, 6, 7)):
        inverted[i] = g["inverted_567"][j].to(dev, dtype)
    for i in range(5):          # (the unguided steps never read theirs)
        inverted[i] = torch.zeros_like(inverted[7])
    kw = dict(guidance_scale=float(g["guidance_scale"]), percentage=float(g["percentage"]), temp_loss_scale=float(g["temp_loss_scale"]))
    return g, dict(latents=r["latents"].to(dev, dtype), noise=r["noise"], inverted=inverted, ctx=ctx, kw=kw, n=n)


def clip(inp, b):
    """The inputs of clip ``b`` alone."""
    ctx = {k: {"context": v["context"][b:b + 1], "fps": v["fps"]} for k, v in inp["ctx"].items()}
    return dict(inp, latents=inp["latents"][b:b + 1], noise=inp["noise"][b:b + 1], inverted=[t[b:b + 1] for t in inp["inverted"]], ctx=ctx)


def sample(m, sched, solver, inp, rng=None, **over):
    rng = dict(rng or {}, noise=inp["noise"])
    return mp.motion_prior_sample(m, solver, sched, inp["latents"], inp["inverted"], inp["ctx"]["inference"], inp["ctx"]["original"],
                                  inp["ctx"]["uncond"], rng=rng, **dict(inp["kw"], **over))


def coefficients(sched, solver, i, w):
    """(|Bg|, sqrt(1 - ap) sqrt(1 - a)) of step i from the schedule, in float64."""
    acp = float(sched.alphas_cumprod[int(solver.ddim_timesteps[i])])
    ap = float(solver.ddim_alpha_cumprods_prev[i])
    a, sg = acp ** 0.5, (1 - acp) ** 0.5
    return abs((1 - ap) ** 0.5 - ap ** 0.5 * sg / a), (1 - ap) ** 0.5 * (1 - a) ** 0.5, ap ** 0.5


@pytest.fixture(scope="module")
def setup():
    from t2v_turbo_amd.unet3d import UNetModel
    m = UNetModel(**tiny_unet_params(record_attn_probs=True)).eval()
    m.load_state_dict(synth_state_dict(manifest("unet_tiny")), strict=True)
    m.requires_grad_(False)
    sched = T2VTurboScheduler(linear_start=0.00085, linear_end=0.012)
    g, inp = golden()
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=inp["n"])
    assert solver.ddim_timesteps.tolist() == [124, 249, 374, 499, 624, 749, 874, 999] and mp.guided_steps(0.5, 8) == [5, 6, 7]
    return m, sched, solver, g, inp


def state_before(sched, solver, g, inp, i):
    """The fixture's latent of clip 0 in front of step i."""
    if i == inp["n"] - 1:
        return sched.add_noise(inp["latents"][:1], inp["noise"][:1], solver.ddim_timesteps[-1:])
    return g["latents_after_clip0"][i + 1:i + 2]


@pytest.mark.parametrize("i", [7, 4])
def test_head_twin_in_float64_reproduces_the_fixtures_step(setup, i):
    m, sched, solver, g, inp = setup
    x = state_before(sched, solver, g, inp, i)
    score = g["score_7"].double() if i == 7 else None
    out = mp.mp_guided_step_torch(solver, sched.alphas_cumprod, i, inp["kw"]["guidance_scale"], x.double(), g[f"cond_{i}"].double(),
                                  g[f"uncond_{i}"].double(), score)
    for name, got, ref in (("next latent", out["x"], g["latents_after_clip0"][i:i + 1]), ("pred_x_0", out["pred_x0"], g[f"pred_x_0_{i}"])):
        err, bound = float((got - ref.double()).abs().max()), 1e-5 * float(ref.abs().max())
        print(f"step {i} {name}: max err {err:.3e}, bound {bound:.3e} (max|ref| {float(ref.abs().max()):.3e})")
        assert err <= bound, (name, err, bound)
    # without the motion term the step is another one: the term cannot be dropped unnoticed
    if i == 7:
        plain = mp.mp_guided_step_torch(solver, sched.alphas_cumprod, i, inp["kw"]["guidance_scale"], x.double(), g["cond_7"].double(),
                                        g["uncond_7"].double(), None)
        assert rel_l2(plain["x"], g["latents_after_clip0"][7:8]) > 0.1


@pytest.mark.parametrize("i", list(range(7, -1, -1)))
def test_twin_sampler_restarted_in_front_of_every_step(setup, monkeypatch, i):
    m, sched, solver, g, inp = setup
    w, n = inp["kw"]["guidance_scale"], inp["n"]
    seen = {}
    real = mp.mp_guided_step_torch

    def spy(solver_, acp, i_, w_, x, cond, uncond, score=None, x0c=None, x0u=None):
        seen.update(cond=cond, uncond=uncond, score=score)
        return real(solver_, acp, i_, w_, x, cond, uncond, score, x0c, x0u)
    monkeypatch.setattr(mp, "mp_guided_step_torch", spy)
    if i == n - 1:          # both clips from the noise: the score clip by clip
        one, refs = inp, torch.cat([g["latents_after_clip0"][7:8], g["latents_after_clip1_740"][0:1]])
        rng = dict(stop_step=i)
    else:
        one, refs = clip(inp, 0), g["latents_after_clip0"][i:i + 1]
        rng = dict(start_latents=state_before(sched, solver, g, inp, i), start_step=i, stop_step=i)
    got, info = sample(m, sched, solver, one, rng=rng)
    guided = i in mp.guided_steps(inp["kw"]["percentage"], n)
    assert info["native"] is False and got.shape == refs.shape and (seen["score"] is not None) == guided
    assert len(info["motion_intermediate"]) == (1 if guided else 0)
    bg, cm, _ = coefficients(sched, solver, i, w)
    d = lambda t: 0.0 if t is None else 1e-5 * float(t.abs().max())   # noqa: E731
    bound = bg * ((1 + w) * d(seen["cond"]) + w * d(seen["uncond"])) + cm * d(seen["score"]) + 1e-5 * float(refs.abs().max())
    err = float((got.double() - refs.double()).abs().max())
    print(f"step {i}: max err {err:.3e}, bound {bound:.3e} (|Bg| {bg:.4f}, motion coefficient {cm:.4f}, max|ref| {float(refs.abs().max()):.3e}, "
          f"rel-L2 {rel_l2(got, refs):.3e})")
    assert err <= bound, (i, err, bound)


@pytest.fixture(scope="module")
def full_run(setup):
    m, sched, solver, g, inp = setup
    return sample(m, sched, solver, inp, return_sampled=True)


def test_whole_loop_follows_the_fixture_and_reports_its_work(setup, full_run):
    """The bookkeeping of a whole run; the distance to the reference's trajectory is printed (eight steps through the network, each
    amplifying what the one before left: the bound is step-wise, in the test above)."""
    m, sched, solver, g, inp = setup
    latents, info = full_run
    assert latents.dtype == torch.float32 and bool(torch.isfinite(latents).all())
    assert info["forwards"] == 3 * (2 * 2 + 1) + 5 * 2 and info["native"] is False
    assert len(info["motion_intermediate"]) == 3 and len(info["sampled_latents"]) == 8
    for e in info["motion_intermediate"]:
        assert tuple(e) == mp.MOTION_INTERMEDIATE_KEYS
        assert all(t.dtype == torch.float16 and t.device.type == "cpu" and t.shape == latents.shape for t in e.values())
    ref = torch.cat([g["latents_after_clip0"][0:1], g["latents_after_clip1_740"][2:3]])
    print(f"final latents: rel-L2 against the fixture {rel_l2(latents, ref):.3e}; pred_x_0 at step 7 {rel_l2(info['sampled_latents'][0][:1], g['pred_x_0_7']):.3e}, "
          f"at step 4 {rel_l2(info['sampled_latents'][3][:1], g['pred_x_0_4']):.3e}")


def test_a_cached_motion_intermediate_gives_the_same_latents(setup, full_run):
    m, sched, solver, g, inp = setup
    w = inp["kw"]["guidance_scale"]
    _, info = full_run
    cached = info["motion_intermediate"]
    want, _ = sample(m, sched, solver, inp, rng=dict(stop_step=5))
    got, info5 = sample(m, sched, solver, inp, rng=dict(stop_step=5), motion_intermediate=cached)
    assert info5["forwards"] == 0 and all(a is b for a, b in zip(info5["motion_intermediate"], cached)) and len(info5["motion_intermediate"]) == 3
    bg, cm, sap = coefficients(sched, solver, 5, w)
    s1ap = (1 - sap ** 2) ** 0.5
    e = {k: ulp(v, torch.float16) / 2 for k, v in cached[2].items()}
    bound = (sap * ((1 + w) * e["cond_pred_x_0"] + w * e["uncond_pred_x_0"]) + s1ap * ((1 + w) * e["cond_pred_noise"] + w * e["uncond_pred_noise"])
             + cm * e["score"] + 1e-5 * float(want.abs().max()))
    err = (got.double() - want.double()).abs()
    print(f"after step 5 on cached entries: max err {float(err.max()):.3e}, largest bound {float(bound.max()):.3e}")
    assert float((err - bound).max()) <= 0.0
    # the whole loop on the cache: only the five unguided steps run the network
    full, info_full = sample(m, sched, solver, inp, motion_intermediate=cached)
    assert info_full["forwards"] == 5 * 2 and bool(torch.isfinite(full).all()) and len(info_full["motion_intermediate"]) == 3


def _vae():
    from t2v_turbo_amd.vae import AutoencoderKL
    ae = AutoencoderKL(ddconfig=VAE_TINY_DD, embed_dim=4).eval()
    ae.load_state_dict(synth_state_dict(manifest("vae_tiny")))
    return ae.requires_grad_(False)


def toy_reward(imgs, text):
    """A differentiable stand-in for a reward model: a fixed pattern over the pixels, one value per image."""
    wgt = torch.linspace(-1.0, 1.0, imgs[0].numel(), device=imgs.device, dtype=imgs.dtype).reshape(imgs[0].shape)
    return (imgs * wgt).sum(dim=(1, 2, 3)) / 100.0


def test_reward_guidance_equals_a_plain_autograd_restatement(setup, monkeypatch):
    m, sched, solver, g, inp = setup
    one, w, i, scale, frames = clip(inp, 0), inp["kw"]["guidance_scale"], 7, 30.0, torch.tensor([0, 2, 3])
    vae = _vae()
    seen = []
    real = mp.mp_guided_step_torch
    monkeypatch.setattr(mp, "mp_guided_step_torch", lambda s, acp, i_, w_, x, c, u, sc=None, a=None, b=None:
                        (seen.append((x, c, u, sc)), real(s, acp, i_, w_, x, c, u, sc, a, b))[1])
    plain, _ = sample(m, sched, solver, one, rng=dict(stop_step=i))
    guided, info = sample(m, sched, solver, one, rng=dict(stop_step=i, reward_frames=frames), vae=vae, reward_fn=toy_reward, reward_scale=scale,
                          reward_batch_size=3, text=["a cat"])
    (x, cond, uncond, motion_score), (_, _, _, total_score) = seen
    acp = float(sched.alphas_cumprod[999])
    lat = x.detach().clone().requires_grad_(True)          # motion_prior_sample.py:231-255, restated
    pred_x_0 = (lat - (1 - acp) ** 0.5 * (cond + w * (cond - uncond))) / acp ** 0.5
    sel = (pred_x_0[:, :, frames] / 0.18215).permute(0, 2, 1, 3, 4).reshape(3, 4, 16, 16)
    imgs = (vae.decoder(vae.post_quant_conv(sel)) / 2 + 0.5).clamp(0, 1)
    (want,) = torch.autograd.grad(-toy_reward(imgs, None).mean() * scale, lat)
    got = total_score - motion_score
    print(f"reward gradient: max |want| {float(want.abs().max()):.3e}, max err {float((got - want).abs().max()):.3e}, "
          f"motion score max {float(motion_score.abs().max()):.3e}")
    assert float(want.abs().max()) > 1e-3 * float(motion_score.abs().max()) > 0
    assert float((got - want).abs().max()) <= 1e-5 * float(total_score.abs().max())
    assert not torch.equal(plain, guided)
    # the stored entry holds the motion score alone, as the script appends it before the reward gradient is added
    assert torch.equal(info["motion_intermediate"][0]["score"], motion_score.to(torch.float16))


def test_refusals(setup):
    m, sched, solver, g, inp = setup
    from t2v_turbo_amd.unet3d import UNetModel
    m.train()
    try:
        with pytest.raises(ValueError):
            sample(m, sched, solver, inp)
    finally:
        m.eval()
    no_probs = UNetModel(**tiny_unet_params()).eval().requires_grad_(False)
    with pytest.raises(ValueError):
        sample(no_probs, sched, solver, inp)
    with pytest.raises(ValueError):
        sample(m, sched, cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=8, use_scale=True), inp)
    with pytest.raises(ValueError):
        sample(m, sched, solver, dict(inp, inverted=inp["inverted"][:7]))
    with pytest.raises(ValueError):
        sample(m, sched, solver, inp, reward_fn=toy_reward, reward_scale=1.0)


def test_video_to_uint8_on_the_cpu_is_the_torch_expression():
    g = torch.Generator().manual_seed(3)
    v = 0.8 * torch.randn((2, 3, 3, 5, 7), generator=g)
    v[0, 1, 2, 3, 4] = float("nan")
    out = mp.video_to_uint8(v)
    want = ((v.clamp(-1, 1) + 1.0) / 2.0 * 255).to(torch.uint8).permute(0, 2, 3, 4, 1)
    assert out.dtype == torch.uint8 and out.shape == (2, 3, 5, 7, 3) and out.is_contiguous()
    keep = ~torch.isnan(v).permute(0, 2, 3, 4, 1)
    assert torch.equal(out[keep], want[keep]) and int(out[0, 2, 3, 4, 1]) == 0
    assert torch.equal(mp.video_to_uint8(v.bfloat16()), mp.video_to_uint8(v.bfloat16().float()))


def test_command_line_writes_frames_and_the_motion_intermediate(tmp_path):
    from tools import motion_prior_sample as cli
    cfg = {"model": {"params": {"linear_start": 0.00085, "linear_end": 0.012, "scale_factor": 0.18215,
                                "unet_config": {"params": tiny_unet_params()},
                                "first_stage_config": {"params": {"ddconfig": VAE_TINY_DD, "embed_dim": 4}}}}}
    p = lambda name: os.path.join(tmp_path, name)   # noqa: E731
    yaml.safe_dump(cfg, open(p("cfg.yaml"), "w"))
    torch.save(synth_state_dict(manifest("unet_tiny")), p("unet.pt"))
    torch.save(synth_state_dict(manifest("vae_tiny")), p("vae.pt"))
    gen = torch.Generator().manual_seed(4)
    np.save(p("clip.npy"), torch.randint(0, 256, (1, 2, 64, 64, 3), generator=gen, dtype=torch.uint8).numpy())
    for name in ("new", "ref", "uncond"):
        np.save(p(name + ".npy"), torch.randn(1, 77, 128, generator=gen).numpy())
    args = ["--unet", p("unet.pt"), "--vae", p("vae.pt"), "--config", p("cfg.yaml"), "--clip", p("clip.npy"), "--inference-embeds", p("new.npy"),
            "--ref-embeds", p("ref.npy"), "--uncond-embeds", p("uncond.npy"), "--num-ddim-timesteps", "4", "--percentage", "0.5",
            "--guidance-scale", "2.0", "--device", "cpu", "--dtype", "fp32"]
    cli.main(args + ["--out-dir", p("out")])
    frames = np.load(p("out/frames.npy"))
    entries = pickle.load(open(p("out/motion_intermediate.pkl"), "rb"))
    assert frames.dtype == np.uint8 and frames.shape == (2, 64, 64, 3) and frames.min() < frames.max()
    assert len(entries) == 1 and all(t.dtype == torch.float16 and t.shape == (1, 4, 2, 8, 8) for t in entries[0].values())          # step 3 of 4
    # given again, the guided step runs on the stored entry
    cli.main(args + ["--out-dir", p("out2"), "--motion-intermediate", p("out/motion_intermediate.pkl")])
    again = np.load(p("out2/frames.npy"))
    assert again.shape == frames.shape and again.dtype == np.uint8
    assert len(pickle.load(open(p("out2/motion_intermediate.pkl"), "rb"))) == 1
