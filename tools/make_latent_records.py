#!/usr/bin/env python
"""Make v2 latent records (``preprocess.make_latent_records``) from ``.npy`` files — a thin command line; there is no text encoder and no
video decoder here: prompts come as embeddings, clips as arrays.

    python tools/make_latent_records.py --unet unet.pt --config inference_t2v_512_v2.0.yaml \\
        (--clips clips.npy --vae vae.pt | --latents latents.npy) --prompt-embeds prompts.npy --uncond-embeds uncond.npy \\
        --texts captions.txt --out-root data --latent-root latents --csv data/latents.csv [--no-motion] [--batch 1]

``clips.npy``: uint8 (N,T,H,W,C) or float (N,T,C,H,W) in [-1, 1]; ``latents.npy``: scaled latents (N,4,T,h,w); ``prompts.npy``: (N,77,D);
``uncond.npy``: (1,77,D) or (N,77,D); ``captions.txt``: one caption per line.  ``unet.pt`` / ``vae.pt``: state dicts of the
``model.diffusion_model`` and ``first_stage_model`` of the teacher's checkpoint; the YAML is the reference's model config
(``unet_config`` / ``first_stage_config`` / ``scale_factor`` / ``linear_start`` / ``linear_end`` under ``model.params``).  Writes
``<out-root>/<latent-root>/<i>.pkl`` and the CSV that ``latent_io.LatentRecordDataset`` opens."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--unet", required=True)
    ap.add_argument("--config", required=True)
    ap.add_argument("--vae")
    ap.add_argument("--clips")
    ap.add_argument("--latents")
    ap.add_argument("--prompt-embeds", required=True)
    ap.add_argument("--uncond-embeds", required=True)
    ap.add_argument("--texts", required=True)
    ap.add_argument("--out-root", required=True)
    ap.add_argument("--latent-root", default="latent_root")
    ap.add_argument("--csv", required=True)
    ap.add_argument("--no-motion", action="store_true")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--fps", type=int, default=8)
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--num-ddim-timesteps", type=int, default=200)
    ap.add_argument("--max-percentage", type=float, default=0.5)
    ap.add_argument("--temp-loss-scale", type=float, default=100.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    a = ap.parse_args(argv)
    if (a.clips is None) == (a.latents is None):
        ap.error("give exactly one of --clips (with --vae) and --latents")
    if a.clips is not None and a.vae is None:
        ap.error("--clips needs --vae")
    import yaml
    from t2v_turbo_amd import cd_math, preprocess
    from t2v_turbo_amd.scheduler import T2VTurboScheduler
    from t2v_turbo_amd.unet3d import UNetModel
    params = yaml.safe_load(open(a.config))["model"]["params"]
    dev, dtype = torch.device(a.device), {"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    ucfg = dict(params["unet_config"]["params"], use_checkpoint=False, record_attn_probs=not a.no_motion)
    unet = UNetModel(**ucfg).eval()
    unet.load_state_dict(torch.load(a.unet, map_location="cpu"), strict=True)
    unet = unet.to(dev, dtype).requires_grad_(False)
    unet.dtype = dtype
    sched = T2VTurboScheduler(linear_start=params.get("linear_start", 0.00085), linear_end=params.get("linear_end", 0.012))
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=a.num_ddim_timesteps)
    prompts = torch.from_numpy(np.load(a.prompt_embeds))
    uncond = torch.from_numpy(np.load(a.uncond_embeds))
    texts = [ln.rstrip("\n") for ln in open(a.texts)]
    n = prompts.shape[0]
    assert len(texts) == n, "one caption per clip"
    gen = torch.Generator().manual_seed(a.seed)
    if a.latents is not None:
        latents = torch.from_numpy(np.load(a.latents))
    else:
        from t2v_turbo_amd.vae import AutoencoderKL
        vae = AutoencoderKL(**params["first_stage_config"]["params"]).eval()
        vae.load_state_dict(torch.load(a.vae, map_location="cpu"), strict=True)
        vae = vae.to(dev, dtype).requires_grad_(False)
        clips = torch.from_numpy(np.load(a.clips))
        latents = torch.cat([preprocess.encode_clips(vae, clips[i:i + a.batch], params.get("scale_factor", 0.18215), generator=gen).float().cpu()
                             for i in range(0, n, a.batch)])
    assert latents.shape[0] == n
    relpaths, blobs = [], []
    for i in range(0, n, a.batch):
        j = min(i + a.batch, n)
        unc = (uncond if uncond.shape[0] == n else uncond.expand(n, -1, -1))[i:j]
        out, info = preprocess.make_latent_records(unet, solver, sched, latents[i:j].to(dev), prompts[i:j].to(dev), unc.to(dev),
                                                   motion=not a.no_motion, fps=a.fps, topk=a.topk, max_percentage=a.max_percentage,
                                                   temp_loss_scale=a.temp_loss_scale, text=texts[i:j], generator=gen)
        blobs += out
        relpaths += [f"{k:08d}.pkl" for k in range(i, j)]
        print(f"clips {i}..{j - 1}: index {info['index'].tolist()} native {info['native']}", flush=True)
    preprocess.write_latent_records(a.out_root, a.latent_root, relpaths, blobs, texts, a.csv)
    print(f"wrote {n} records under {os.path.join(a.out_root, a.latent_root)} and {a.csv}")


if __name__ == "__main__":
    main()
