"""-m gpu: the motion-prior sampler's kernels on the device — the case table and bounds of tests/mp_sample_cases.py (shared with the
host-simulator test) — and ``motion_prior.motion_prior_sample`` on the tiny bf16 UNet against the run the REFERENCE computed in fp32
(tests/golden/motion_sample_tiny.npz).

Bound of the sampler against the fixture: ``e_native <= 1.1 * e_twin + 2^-9``, both the rel-L2 of the final latents against the
fixture, e_twin from ``T2V_NATIVE_MP_SAMPLE=0`` on the same inputs in this test — the form of tests/test_gpu_record.py with fp16's 2^-11
replaced by bf16's 2^-9 (the rounding of the UNet's input): keeping the state in fp32 is no further from the reference than rounding
it after every step.  No absolute figure is fixed; the engine's own error against fp32 is the existing engine tests' subject."""
import os
import warnings

import pytest
import torch

from oracle.synth import synth_state_dict
from t2v_turbo_amd import cd_math
from t2v_turbo_amd import motion_prior as mp
from t2v_turbo_amd import native as nt
from t2v_turbo_amd.scheduler import T2VTurboScheduler
from tests import cd_head_cases as cc
from tests import mp_sample_cases as mc
from tests.test_motion_sample_cpu import clip, golden, sample, toy_reward
from tests.util import VAE_TINY_DD, manifest, rel_l2, tiny_unet_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return nt.HipOps()


# --------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("geom,i,dtype,with_score,with_x0,outs,lp,pd", mc.HEAD_PARAMS)
def test_guided_step_on_the_case_table(ops, geom, i, dtype, with_score, with_x0, outs, lp, pd):
    case = mc.head_case(geom, i, dtype, with_score, with_x0)
    first = mc.run_head(ops, "cuda", case, outs, cc.DTYPES[lp], cc.DTYPES[pd])
    mc.check_head(case, first)
    again = mc.run_head(ops, "cuda", case, outs, cc.DTYPES[lp], cc.DTYPES[pd])
    assert all(first[k] is None or mc.same_bits(first[k], again[k]) for k in first)


@pytest.mark.parametrize("dtype", list(cc.DTYPES))
@pytest.mark.parametrize("with_x0", [False, True])
def test_bases_off_a_16_byte_boundary_take_the_scalar_path(ops, dtype, with_x0):
    case = mc.head_case("misaligned", 24, dtype, True, with_x0)
    got = mc.run_head(ops, "cuda", case, "lpr", torch.bfloat16, cc.DTYPES[dtype], misalign=True)
    mc.check_head(case, got, " (unaligned)")
    aligned = mc.run_head(ops, "cuda", case, "lpr", torch.bfloat16, cc.DTYPES[dtype])
    assert all(mc.same_bits(got[k], aligned[k]) for k in got)


def test_guided_step_refusals_return_the_error_codes_before_any_launch(ops):
    mc.check_head_refusals(ops, "cuda")
    sched, tabs = mc._sched(ops, "cuda")
    x = torch.randn(2, 40, device="cuda")
    for call in (lambda: ops.mp_guided_step(sched, 50, 2.0, x.clone(), x, x),                               # step outside the grid
                 lambda: ops.mp_guided_step(sched, 1, 2.0, x.clone(), x.double(), x.double()),              # dtype code
                 lambda: ops.mp_guided_step(sched, 1, 2.0, x.clone(), x, x, x0_cond=x)):                    # one x0 alone
        with pytest.raises(nt.NativeError):
            call()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_uint8_equals_the_torch_expression_on_every_16_bit_pattern(ops, dtype):
    video = mc.u8_patterns(dtype)
    out = mc.run_u8(ops, "cuda", video)
    mc.check_u8(video, out, dtype)
    nan = torch.isnan(video.float()).permute(0, 2, 3, 4, 1)
    assert bool(nan.any()) and not bool(out.cpu()[nan].any()), "NaN gives 0"
    assert mc.same_bits(out, mc.run_u8(ops, "cuda", video))


def test_uint8_on_the_fp32_boundary_values(ops):
    video = mc.u8_boundaries()
    mc.check_u8(video, mc.run_u8(ops, "cuda", video), "boundaries")


@pytest.mark.parametrize("dtype", list(cc.DTYPES))
def test_uint8_batch_frame_and_channel_addressing_and_a_misaligned_base(ops, dtype):
    video = mc.u8_batch(dtype)
    mc.check_u8(video, mc.run_u8(ops, "cuda", video), dtype)
    mc.check_u8(video, mc.run_u8(ops, "cuda", video, misalign=True), dtype + " (unaligned)")
    wide = video[..., :4].contiguous()
    mc.check_u8(wide, mc.run_u8(ops, "cuda", wide), dtype + " (vector)")
    mc.check_u8(wide, mc.run_u8(ops, "cuda", wide, misalign=True), dtype + " (vector shape, unaligned)")


def test_uint8_refusals(ops):
    mc.check_u8_refusals(ops, "cuda")


# --------------------------------------------------------------------------------------------------------------- the sampler
def shared_ops():
    return nt.shared_ops()


@pytest.fixture(scope="module")
def model():
    from tests.test_gpu_engine import _unet
    m = _unet(tiny_unet_params(record_attn_probs=True), "unet_tiny", torch.bfloat16)
    m.dtype = torch.bfloat16
    m.requires_grad_(False)
    sched = T2VTurboScheduler(linear_start=0.00085, linear_end=0.012)
    g, inp = golden("cuda")
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=inp["n"])
    return m, sched, solver, g, inp


@pytest.fixture(scope="module")
def sampled(model):
    """(fixture, (latents, info) of the native path and of T2V_NATIVE_MP_SAMPLE=0, launches counted on the shared ops)."""
    m, sched, solver, g, inp = model
    ops = shared_ops()
    calls = {"mp_guided_step": 0, "cd_add_noise": 0}
    real = {name: getattr(ops, name) for name in calls}
    for name in calls:
        setattr(ops, name, (lambda nm: lambda *a, **k: (calls.__setitem__(nm, calls[nm] + 1), real[nm](*a, **k))[1])(name))
    out = {}
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)          # the composite UNet path must not be taken
            out["native"] = sample(m, sched, solver, inp)
            native_calls = dict(calls)
            os.environ["T2V_NATIVE_MP_SAMPLE"] = "0"
            try:
                out["twin"] = sample(m, sched, solver, inp)
            finally:
                del os.environ["T2V_NATIVE_MP_SAMPLE"]
        assert calls == native_calls, "T2V_NATIVE_MP_SAMPLE=0 launched a sampler kernel"
    finally:
        for name in calls:
            delattr(ops, name)
    torch.cuda.synchronize()
    return g, out, native_calls


def test_sampler_on_the_device_against_the_reference_run(model, sampled):
    """Measured on MI355X (this test prints the figures): final latents against the fixture e_native 1.0170e-1, e_twin
    (``T2V_NATIVE_MP_SAMPLE=0``) 1.0335e-1, bound 1.1564e-1 — eight steps through the tiny bf16 UNet at ``temp_loss_scale`` 500, each
    amplifying what the one before left; the stored scores of the two paths differ by 5.6e-2 / 1.3e-1 / 1.1e-1 (steps 7 / 6 / 5)."""
    g, out, native_calls = sampled
    (lat_n, info_n), (lat_t, info_t) = out["native"], out["twin"]
    assert info_n["native"] is True and info_t["native"] is False
    # eight steps, one launch each; three guided steps of three forwards, five of two; one copy brings the three entries back
    assert native_calls == {"mp_guided_step": 8, "cd_add_noise": 1}, native_calls
    assert info_n["forwards"] == 3 * 3 + 5 * 2 and info_n["device_to_host_copies"] == 1
    assert lat_n.dtype == torch.float32 and lat_t.dtype == torch.bfloat16
    for info in (info_n, info_t):
        assert len(info["motion_intermediate"]) == 3
        for e in info["motion_intermediate"]:
            assert tuple(e) == mp.MOTION_INTERMEDIATE_KEYS
            assert all(t.dtype == torch.float16 and t.device.type == "cpu" and t.shape == lat_n.shape and bool(torch.isfinite(t).all())
                       for t in e.values())
    ref = torch.cat([g["latents_after_clip0"][0:1], g["latents_after_clip1_740"][2:3]])
    e_native, e_twin = rel_l2(lat_n.float().cpu(), ref), rel_l2(lat_t.float().cpu(), ref)
    print(f"final latents against the fixture: e_native {e_native:.4e}, e_twin (T2V_NATIVE_MP_SAMPLE=0) {e_twin:.4e}, "
          f"bound {1.1 * e_twin + 2.0 ** -9:.4e}")
    for k in range(3):
        print(f"  entry {k}: score rel-L2 native vs twin {rel_l2(info_n['motion_intermediate'][k]['score'].float(), info_t['motion_intermediate'][k]['score'].float()):.3e}")
    assert e_native <= 1.1 * e_twin + 2.0 ** -9, (e_native, e_twin)


def _vae(dtype=torch.bfloat16):
    from t2v_turbo_amd.vae import AutoencoderKL
    ae = AutoencoderKL(ddconfig=VAE_TINY_DD, embed_dim=4).eval()
    ae.load_state_dict(synth_state_dict(manifest("vae_tiny")))
    return ae.requires_grad_(False)


def test_video_to_uint8_of_a_decode_and_the_pipelines_uint8_output(model):
    from t2v_turbo_amd.latent_diffusion import LatentDiffusion
    from t2v_turbo_amd.pipeline import T2VTurboVC2Pipeline
    from t2v_turbo_amd.unet3d import UNetModel
    from tests.util import load
    ae = _vae().cuda()
    z = torch.randn(1, 4, 3, 8, 8, generator=torch.Generator().manual_seed(11)).cuda()
    with torch.no_grad():
        video = ae.decode_video(z)
    frames = mp.video_to_uint8(video)
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.shape == (1, 3, 64, 64, 3)
    assert torch.equal(frames.cpu(), mc.u8_expected(video)) and int(frames.min()) < int(frames.max())
    p = tiny_unet_params()
    unet = UNetModel(**p).eval()
    unet.load_state_dict(synth_state_dict(manifest("unet_tiny")), strict=True)
    pipe = T2VTurboVC2Pipeline(LatentDiffusion(unet, _vae()).cuda(), T2VTurboScheduler(), {"params": {"unet_config": {"params": p}}})
    kw = dict(prompt=None, height=64, width=64, frames=4, fps=16, guidance_scale=7.5, num_inference_steps=4, lcm_origin_steps=50,
              prompt_embeds=load("pipeline_tiny")["prompt_embeds"].cuda())
    vid = pipe(generator=torch.Generator().manual_seed(42), output_type="pt", **kw)
    u8 = pipe(generator=torch.Generator().manual_seed(42), output_type="uint8", **kw)
    assert u8.dtype == torch.uint8 and u8.shape == (1, 4, 64, 64, 3) and torch.equal(u8.cpu(), mc.u8_expected(vid))


def test_reward_guidance_runs_on_the_native_decode_gradient(model):
    """The reward gradient of a guided step on the device (bf16 VAE, native decode-gradient engine) against plain autograd through the
    same VAE in fp32 on the CPU: rel-L2 < 5e-2, the bound of ``test_vae_decode_backward_native_vs_oracle_autograd``."""
    m, sched, solver, g, inp = model
    one, w, frames = clip(inp, 0), inp["kw"]["guidance_scale"], torch.tensor([0, 2, 3])
    ae = _vae().cuda().bfloat16()
    gen = torch.Generator().manual_seed(21)
    x = (3.0 * torch.randn(1, 4, 4, 16, 16, generator=gen)).bfloat16()
    cond = torch.randn(x.shape, generator=gen).bfloat16()
    uncond = (cond.float() + 0.3 * torch.randn(x.shape, generator=gen)).bfloat16()
    kw = dict(vae_scale_factor=0.18215, reward_fn=toy_reward, reward_scale=30.0, reward_batch_size=3, text=None, rng=dict(reward_frames=frames),
              generator=None)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = mp._reward_score(x.cuda(), cond.cuda(), uncond.cuda(), 7, w, solver, sched.alphas_cumprod, vae=ae, **kw)
        assert ae._engine_box.grad is not None and ae._engine_box.grad.ops.is_native
        want = mp._reward_score(x, cond, uncond, 7, w, solver, sched.alphas_cumprod, vae=_vae(), **kw)
        err = rel_l2(got.float().cpu(), want)
        print(f"reward gradient on the device against fp32 autograd: rel-L2 {err:.3e} (bound 5e-2), max |want| {float(want.abs().max()):.3e}")
        assert float(want.abs().max()) > 0 and err < 5e-2
        # and inside the sampler: one guided step with the reward term, on the native routes
        lat, info = sample(m, sched, solver, one, rng=dict(stop_step=7, reward_frames=frames), vae=ae, reward_fn=toy_reward, reward_scale=30.0,
                           reward_batch_size=3)
        plain, info_p = sample(m, sched, solver, one, rng=dict(stop_step=7))
    assert info["native"] and bool(torch.isfinite(lat).all()) and not torch.equal(lat, plain)
    # the stored entry holds the motion score alone: the same kernels on the same inputs as the plain run (had it held the sum, the
    # distance would be the reward term's share of the score, about 1e-1 here)
    d = rel_l2(info["motion_intermediate"][0]["score"].float(), info_p["motion_intermediate"][0]["score"].float())
    print(f"stored score with and without the reward term: rel-L2 {d:.3e}")
    assert d < 1e-3
