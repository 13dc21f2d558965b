#!/usr/bin/env python
"""A golden v2 latent record from THE REFERENCE ITSELF (CPU, fp32; needs the reference checkout that make_golden.py names):

    python tests/golden/make_golden_record.py        -> tests/golden/record_tiny.npz

What ``preprocess.make_latent_records`` must reproduce: the seven tensors ``preprocess_scripts/preprocess_with_motion_prior.py:328-409``
stores per clip, computed by the reference's ``T2VTurboScheduler.add_noise``, ``DDIMSolver.ddim_reverse_step`` (inside the inversion loop of
``motion_prior_sample.py:27-37``), ``UNetModel`` and ``compute_temp_loss`` (inside the score of ``motion_prior_sample.py:59-84``).  Two clips
on the tiny UNet with ``record_attn_probs=True`` (weights from ``oracle/synth.py``): clip 0 is the input of ``unet_tiny.npz``, clip 1 is
seeded here; a 50-point solver, ``index = [3, 0]`` (four inversion steps; clip 1 stops after one and keeps the original latent as
``z_example_prev``), a pinned ``noise``, fps 8, ``temp_loss_scale`` 500.  The script runs one clip per call (``index.item()``): so does
this file."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

INDEX, FPS, TEMP_LOSS_SCALE, NUM_DDIM = [3, 0], 8, 500.0, 50


def main():
    import make_golden as mg
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    from oracle.synth import manifest_of, synth_state_dict
    from lvdm.modules.networks.openaimodel3d import UNetModel
    from ode_solver.ddim_solver import DDIMSolver
    from scheduler.t2v_turbo_scheduler import T2VTurboScheduler
    from utils.common_utils import compute_temp_loss

    z = np.load(os.path.join(HERE, "unet_tiny.npz"))
    g = torch.Generator().manual_seed(31)
    x0, ctx0 = torch.from_numpy(z["x"]), torch.from_numpy(z["ctx"])
    latents = torch.cat([x0, torch.randn(x0.shape, generator=g)])
    prompt_embeds = torch.cat([ctx0, torch.randn(ctx0.shape, generator=g)])
    uncond = torch.randn(ctx0.shape, generator=g)
    noise = torch.randn(latents.shape, generator=g)
    index = torch.tensor(INDEX)

    m = UNetModel(**mg.tiny_unet_params(record_attn_probs=True)).eval()
    m.load_state_dict(synth_state_dict(manifest_of(m)), strict=True)
    m.requires_grad_(False)
    sch = T2VTurboScheduler(linear_start=0.00085, linear_end=0.012)
    solver = DDIMSolver(sch.alphas_cumprod.numpy(), ddim_timesteps=NUM_DDIM, use_scale=False)

    def probs_of(model):  # motion_prior_sample.py:40-56
        blocks = tuple(f"output_blocks.{i}.2" for i in range(3, 12))
        return {n: mod.attention_probs for n, mod in model.named_modules() if n.startswith(blocks) and n.endswith("blocks.0.attn1")}

    out = {k: [] for k in ("z_t", "cond_teacher_out", "uncond_teacher_out", "score", "z_example", "z_example_prev")}
    for b in range(latents.shape[0]):
        lat, idx = latents[b:b + 1], index[b:b + 1]
        ctx = {"context": prompt_embeds[b:b + 1], "fps": FPS}
        start = solver.ddim_timesteps[idx]
        with torch.no_grad():
            z_t = sch.add_noise(lat, noise[b:b + 1], start)
            inter, cur = [], lat
            for i in range(int(idx) + 1):  # motion_prior_sample.py:27-37
                ts = solver.ddim_timesteps[torch.full((1,), i, dtype=torch.long)].long()
                cur = solver.ddim_reverse_step(cur, m(cur, ts, **ctx), ts)
                inter.append(cur)
            z_example = inter[-1]
            z_example_prev = inter[-2] if int(idx) > 0 else lat
            uncond_out = m(z_t, start, context=uncond, fps=FPS)
            m(z_example, start, **ctx)  # motion_prior_sample.py:59-84
            ref_probs = dict(probs_of(m))
        zg = z_t.clone().requires_grad_(True)
        cond_out = m(zg, start, **ctx)
        loss = TEMP_LOSS_SCALE * compute_temp_loss(probs_of(m), ref_probs)
        (score,) = torch.autograd.grad(loss, zg)
        assert len(ref_probs) == 9 and float(score.abs().max()) > 0
        for k, v in (("z_t", z_t), ("cond_teacher_out", cond_out), ("uncond_teacher_out", uncond_out), ("score", score),
                     ("z_example", z_example), ("z_example_prev", z_example_prev)):
            out[k].append(v.detach())
        print(f"clip {b}: index {int(idx)} loss {float(loss.detach()):.6f} score std {float(score.std()):.4e} z_example std {float(z_example.std()):.4f}")
    arrays = {k: torch.cat(v).numpy() for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "record_tiny.npz"), latents=latents.numpy(), prompt_emb=prompt_embeds.numpy(),
                        uncond_prompt_embeds=uncond.numpy(), noise=noise.numpy(), index=index.numpy(), fps=np.int64(FPS),
                        temp_loss_scale=np.float32(TEMP_LOSS_SCALE), **arrays)
    print("wrote record_tiny.npz", {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
