#!/usr/bin/env python
"""The motion-clone sampler (``motion_prior.motion_prior_sample``, reference ``motion_prior_sample.py``) from ``.npy`` files — a thin command
line; there is no text encoder and no video file I/O here: prompts come as embeddings, the clip as an array.

    python tools/motion_prior_sample.py --unet unet.pt --vae vae.pt --config inference_t2v_512_v2.0.yaml \\
        (--clip clip.npy | --latents latents.npy) --inference-embeds new_prompt.npy --ref-embeds ref_prompt.npy --uncond-embeds uncond.npy \\
        --out-dir out [--num-ddim-timesteps 200] [--percentage 0.6] [--guidance-scale 7.5] [--temp-loss-scale 100] [--motion-intermediate m.pkl]

``clip.npy``: uint8 (1,T,H,W,C) or float (1,T,C,H,W) in [-1, 1]; ``latents.npy``: scaled latents (1,4,T,h,w); the three embeddings:
(1,77,D).  ``unet.pt`` / ``vae.pt``: state dicts of the ``model.diffusion_model`` and ``first_stage_model`` of the checkpoint; the YAML is
the reference's model config.  Runs encode -> DDIM inversion under the reference prompt -> guided sampling under the new prompt ->
decode -> uint8, and writes ``<out-dir>/frames.npy`` (T,H,W,3) uint8 and ``<out-dir>/motion_intermediate.pkl`` (the list the script
pickles; given again with ``--motion-intermediate``, its guided steps run no forward)."""
import argparse
import copy
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--unet", required=True)
    ap.add_argument("--vae", required=True)
    ap.add_argument("--config", required=True)
    ap.add_argument("--clip")
    ap.add_argument("--latents")
    ap.add_argument("--inference-embeds", required=True)
    ap.add_argument("--ref-embeds", required=True)
    ap.add_argument("--uncond-embeds", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--motion-intermediate")
    ap.add_argument("--fps", type=int, default=8)
    ap.add_argument("--num-ddim-timesteps", type=int, default=200)
    ap.add_argument("--percentage", type=float, default=0.6)
    ap.add_argument("--guidance-scale", type=float, default=7.5)
    ap.add_argument("--temp-loss-scale", type=float, default=100.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    a = ap.parse_args(argv)
    if (a.clip is None) == (a.latents is None):
        ap.error("give exactly one of --clip and --latents")
    import yaml
    from t2v_turbo_amd import cd_math, motion_prior, preprocess
    from t2v_turbo_amd.scheduler import T2VTurboScheduler
    from t2v_turbo_amd.unet3d import UNetModel
    from t2v_turbo_amd.vae import AutoencoderKL
    params = yaml.safe_load(open(a.config))["model"]["params"]
    dev, dtype = torch.device(a.device), {"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    scale = params.get("scale_factor", 0.18215)
    unet = UNetModel(**dict(params["unet_config"]["params"], use_checkpoint=False, record_attn_probs=True)).eval()
    unet.load_state_dict(torch.load(a.unet, map_location="cpu"), strict=True)
    unet = unet.to(dev, dtype).requires_grad_(False)
    unet.dtype = dtype
    vae = AutoencoderKL(**params["first_stage_config"]["params"]).eval()
    vae.load_state_dict(torch.load(a.vae, map_location="cpu"), strict=True)
    vae = vae.to(dev, dtype).requires_grad_(False)
    sched = T2VTurboScheduler(linear_start=params.get("linear_start", 0.00085), linear_end=params.get("linear_end", 0.012))
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=a.num_ddim_timesteps)
    gen = torch.Generator().manual_seed(a.seed)
    if a.latents is not None:
        latents = torch.from_numpy(np.load(a.latents)).to(dev, dtype)
    else:
        latents = preprocess.encode_clips(vae, torch.from_numpy(np.load(a.clip)), scale, generator=gen).to(dev, dtype)
    ctx = {k: {"context": torch.from_numpy(np.load(p)).to(dev, dtype), "fps": a.fps}
           for k, p in (("inference", a.inference_embeds), ("ref", a.ref_embeds), ("uncond", a.uncond_embeds))}
    n = a.num_ddim_timesteps
    inverted = motion_prior.reverse_ddim_loop(latents, unet, ctx["ref"], copy.copy(solver).to(dev), n, dev)
    print(f"inverted {n} steps", flush=True)
    cached = pickle.load(open(a.motion_intermediate, "rb")) if a.motion_intermediate else None
    out, info = motion_prior.motion_prior_sample(unet, solver, sched, latents, inverted, ctx["inference"], ctx["ref"], ctx["uncond"],
                                                 guidance_scale=a.guidance_scale, percentage=a.percentage, temp_loss_scale=a.temp_loss_scale,
                                                 motion_intermediate=cached, generator=gen)
    print(f"sampled: {info['forwards']} forwards, native {info['native']}, {info['device_to_host_copies']} device-to-host copies", flush=True)
    with torch.no_grad():
        frames = motion_prior.video_to_uint8(vae.decode_video(out.to(dtype), scale))
    os.makedirs(a.out_dir, exist_ok=True)
    np.save(os.path.join(a.out_dir, "frames.npy"), frames[0].cpu().numpy())
    with open(os.path.join(a.out_dir, "motion_intermediate.pkl"), "wb") as f:
        pickle.dump(info["motion_intermediate"], f)
    print(f"wrote {tuple(frames[0].shape)} uint8 frames and {len(info['motion_intermediate'])} motion_intermediate entries under {a.out_dir}")


if __name__ == "__main__":
    main()
