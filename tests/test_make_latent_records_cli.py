"""tools/make_latent_records.py in-process on the CPU at toy size: ``.npy`` clips through the VAE encoder (uint8 frames), prompt embeddings,
tiny UNet and VAE state dicts -> record files and a CSV that ``LatentRecordDataset`` reads back; and ``encode_clips`` on both video
layouts against the VAE's own ``encode``."""
import os

import numpy as np
import torch
import yaml

from oracle.synth import synth_state_dict
from t2v_turbo_amd import latent_io, preprocess
from tests.util import VAE_TINY_DD, manifest, tiny_unet_params


def _vae():
    from t2v_turbo_amd.vae import AutoencoderKL
    ae = AutoencoderKL(ddconfig=VAE_TINY_DD, embed_dim=4).eval()
    ae.load_state_dict(synth_state_dict(manifest("vae_tiny")))
    return ae.requires_grad_(False)


def test_encode_clips_matches_the_vaes_encode_on_both_layouts():
    ae = _vae()
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (1, 2, 64, 64, 3), generator=g, dtype=torch.uint8)
    as_float = frames.permute(0, 1, 4, 2, 3).float() / 127.5 - 1.0
    a = preprocess.encode_clips(ae, frames, 0.18215, generator=torch.Generator().manual_seed(9))
    b = preprocess.encode_clips(ae, as_float, 0.18215, generator=torch.Generator().manual_seed(9))
    assert a.shape == (1, 4, 2, 8, 8) and torch.equal(a, b)
    noise = torch.randn(1, 4, 2, 8, 8, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        want = torch.stack([ae.encode(as_float[:, t]).sample(noise[:, :, t]) for t in range(2)], dim=2) * 0.18215
    assert torch.allclose(a, want, rtol=1e-5, atol=1e-6)


def test_command_line_writes_records_the_dataset_reads(tmp_path):
    from tools import make_latent_records as cli
    cfg = {"model": {"params": {"linear_start": 0.00085, "linear_end": 0.012, "scale_factor": 0.18215,
                                "unet_config": {"params": tiny_unet_params()},
                                "first_stage_config": {"params": {"ddconfig": VAE_TINY_DD, "embed_dim": 4}}}}}
    p = lambda name: os.path.join(tmp_path, name)   # noqa: E731
    yaml.safe_dump(cfg, open(p("cfg.yaml"), "w"))
    torch.save(synth_state_dict(manifest("unet_tiny")), p("unet.pt"))
    torch.save(synth_state_dict(manifest("vae_tiny")), p("vae.pt"))
    g = torch.Generator().manual_seed(4)
    np.save(p("clips.npy"), torch.randint(0, 256, (2, 2, 64, 64, 3), generator=g, dtype=torch.uint8).numpy())
    np.save(p("prompts.npy"), torch.randn(2, 77, 128, generator=g).numpy())
    np.save(p("uncond.npy"), torch.randn(1, 77, 128, generator=g).numpy())
    open(p("captions.txt"), "w").write("a cat\na dog\n")
    cli.main(["--unet", p("unet.pt"), "--config", p("cfg.yaml"), "--vae", p("vae.pt"), "--clips", p("clips.npy"), "--prompt-embeds",
              p("prompts.npy"), "--uncond-embeds", p("uncond.npy"), "--texts", p("captions.txt"), "--out-root", p("data"), "--csv",
              p("latents.csv"), "--num-ddim-timesteps", "50", "--device", "cpu", "--dtype", "fp32", "--batch", "2"])
    ds = latent_io.LatentRecordDataset(p("latents.csv"), root_dir=p("data"))
    ds.MAX_RETRIES = 1
    assert len(ds) == 2
    for i, text in enumerate(["a cat", "a dog"]):
        s = ds[i]
        assert s["txt"] == text and 25 <= int(s["index"]) < 50
        for k in preprocess.RECORD_TENSORS:
            assert s[k].dtype == torch.float16 and bool(torch.isfinite(s[k]).all()), k
        assert s["z_t"].shape == (4, 2, 8, 8) and s["prompt_emb"].shape == (77, 128) and bool(s["score"].any())
