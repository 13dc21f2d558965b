#!/usr/bin/env python
"""A golden run of the motion-prior guided sampler from THE REFERENCE ITSELF (CPU, fp32; needs the reference checkout that make_golden.py
names):

    python tests/golden/make_golden_motion_sample.py        -> tests/golden/motion_sample_tiny.npz

What ``motion_prior.motion_prior_sample`` must reproduce: the loop of ``motion_prior_sample.py:146-297`` computed with the reference's
``UNetModel`` (tiny, ``record_attn_probs=True``, weights from ``oracle/synth.py``), ``T2VTurboScheduler.add_noise``, ``DDIMSolver``
(``ddim_reverse_step`` for the inversion, ``ddim_step`` for the sampling), ``get_predicted_original_sample``, ``extract_into_tensor`` and
``compute_temp_loss``.  Two clips: the two latents and prompts of ``record_tiny.npz``, each sampled under the OTHER clip's prompt (its own
prompt is the original context), one clip per call as the script runs.  An 8-point solver (timesteps 124 ... 999), ``percentage`` 0.5
(steps 7, 6, 5 are guided, 4 ... 0 are not), ``guidance_scale`` 2.0, ``temp_loss_scale`` 500, fps 8, the noise of ``record_tiny.npz``.
The inputs stay in ``record_tiny.npz`` (this file stores their sums); stored are the inversion latents at steps 7, 6, 5, the latent
after every step for clip 0 and after steps 7, 4, 0 for clip 1, and for clip 0 at steps 7 and 4 ``cond``, ``uncond``, ``pred_x_0`` (and the
score at step 7).

The motion term must matter: the file asserts that ``sqrt(1 - a) score`` has at least 0.1 of the standard deviation of the CFG noise
estimate at every guided step, and prints the ratio."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

NUM_DDIM, PERCENTAGE, GUIDANCE_SCALE, TEMP_LOSS_SCALE, FPS = 8, 0.5, 2.0, 500.0, 8
KEPT_STEPS = (7, 4)          # clip 0: cond / uncond / pred_x_0 (and the score at step 7) are stored for these steps


def main():
    import make_golden as mg
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    from oracle.synth import manifest_of, synth_state_dict
    from lvdm.modules.networks.openaimodel3d import UNetModel
    from ode_solver.ddim_solver import DDIMSolver
    from scheduler.t2v_turbo_scheduler import T2VTurboScheduler
    from utils.common_utils import compute_temp_loss, extract_into_tensor, get_predicted_original_sample

    rec = np.load(os.path.join(HERE, "record_tiny.npz"))
    latents_all, prompts = torch.from_numpy(rec["latents"]), torch.from_numpy(rec["prompt_emb"])
    uncond, noise_all = torch.from_numpy(rec["uncond_prompt_embeds"]), torch.from_numpy(rec["noise"])

    m = UNetModel(**mg.tiny_unet_params(record_attn_probs=True)).eval()
    m.load_state_dict(synth_state_dict(manifest_of(m)), strict=True)
    m.requires_grad_(False)
    sch = T2VTurboScheduler(linear_start=0.00085, linear_end=0.012)
    solver = DDIMSolver(sch.alphas_cumprod.numpy(), ddim_timesteps=NUM_DDIM, use_scale=False)
    alpha_schedule, sigma_schedule = torch.sqrt(sch.alphas_cumprod), torch.sqrt(1 - sch.alphas_cumprod)
    n = len(solver.ddim_timesteps)
    assert solver.ddim_timesteps.tolist() == [124, 249, 374, 499, 624, 749, 874, 999]

    def probs_of(model):  # motion_prior_sample.py:40-56
        blocks = tuple(f"output_blocks.{i}.2" for i in range(3, 12))
        return {nm: mod.attention_probs for nm, mod in model.named_modules() if nm.startswith(blocks) and nm.endswith("blocks.0.attn1")}

    out = {"after": [], "inverted": []}
    kept = {}
    for b in range(latents_all.shape[0]):
        original_latents = latents_all[b:b + 1]
        inference_context = {"context": prompts[1 - b:2 - b], "fps": FPS}
        original_context = {"context": prompts[b:b + 1], "fps": FPS}
        uncond_context = {"context": uncond, "fps": FPS}
        with torch.no_grad():
            intermediate_latents, cur = [], original_latents
            for i in range(n):  # motion_prior_sample.py:27-37
                ts = solver.ddim_timesteps[torch.full((1,), i, dtype=torch.long)].long()
                cur = solver.ddim_reverse_step(cur, m(cur, ts, **original_context), ts)
                intermediate_latents.append(cur)
            latents = sch.add_noise(original_latents, noise_all[b:b + 1], solver.ddim_timesteps[-1])
        after = []
        for i in range(n - 1, -1, -1):  # motion_prior_sample.py:157-294
            index = torch.full((1,), i, dtype=torch.long)
            ts = solver.ddim_timesteps[index]
            guided = i > n - PERCENTAGE * n
            if guided:
                with torch.no_grad():  # motion_prior_sample.py:59-84
                    m(intermediate_latents[i], ts, **original_context)
                    ref_probs = dict(probs_of(m))
                zg = latents.detach().clone().requires_grad_(True)
                cond_pred_noise = m(zg, ts, **inference_context)
                loss = TEMP_LOSS_SCALE * compute_temp_loss(probs_of(m), ref_probs)
                score = torch.autograd.grad(loss, zg)[0].detach()
                cond_pred_noise = cond_pred_noise.detach()
            with torch.no_grad():
                if not guided:
                    cond_pred_noise = m(latents, ts, **inference_context)
                    score = torch.zeros_like(latents)
                uncond_pred_noise = m(latents, ts, **uncond_context)
                cond_pred_x_0 = get_predicted_original_sample(cond_pred_noise, ts, latents, "epsilon", alpha_schedule, sigma_schedule)
                uncond_pred_x_0 = get_predicted_original_sample(uncond_pred_noise, ts, latents, "epsilon", alpha_schedule, sigma_schedule)
                pred_x_0 = cond_pred_x_0 + GUIDANCE_SCALE * (cond_pred_x_0 - uncond_pred_x_0)
                pred_noise = cond_pred_noise + GUIDANCE_SCALE * (cond_pred_noise - uncond_pred_noise)
                alphas = extract_into_tensor(alpha_schedule, ts, score.shape)
                term = (1 - alphas) ** (0.5) * score
                if guided:
                    ratio = float(term.std() / pred_noise.std())
                    print(f"clip {b} step {i}: loss {float(loss.detach()):.5f}  std(motion term) / std(CFG noise estimate) = {ratio:.3f}")
                    assert ratio >= 0.1, (b, i, ratio)
                pred_noise = pred_noise - term
                if b == 0 and i in KEPT_STEPS:
                    kept.update({f"cond_{i}": cond_pred_noise, f"uncond_{i}": uncond_pred_noise, f"pred_x_0_{i}": pred_x_0})
                    if guided:
                        kept[f"score_{i}"] = score
                latents = solver.ddim_step(pred_x_0, pred_noise, index).to(torch.float32)
            assert bool(torch.isfinite(latents).all())
            after.append(latents)
        out["after"].append(torch.cat(after[::-1]))          # [n] in step order: after[i] = the latent after step i
        out["inverted"].append(torch.cat([intermediate_latents[i] for i in (5, 6, 7)]))
        print(f"clip {b}: final latent std {float(latents.std()):.4f}")
    # (sizes: the inputs are record_tiny.npz's and are not stored twice — their float64 sums are, so that a test can tell a regenerated
    # record_tiny.npz from the one this run read; clip 1 keeps its latents after steps 7, 4 and 0 only)
    arrays = {"latents_after_clip0": out["after"][0].numpy(),                 # [n, 4, F, h, w]: after[i] = the latent after step i
              "latents_after_clip1_740": out["after"][1][[7, 4, 0]].numpy(),   # [3, 4, F, h, w]
              "inverted_567": torch.stack(out["inverted"], 1).numpy()}        # [3, B, 4, F, h, w]: the inversion latents at steps 5, 6, 7
    arrays.update({k: v.numpy() for k, v in kept.items()})
    sums = np.asarray([float(t.double().sum()) for t in (latents_all, prompts, uncond, noise_all)])
    np.savez_compressed(os.path.join(HERE, "motion_sample_tiny.npz"), input_sums=sums, num_ddim=np.int64(NUM_DDIM),
                        percentage=np.float32(PERCENTAGE), guidance_scale=np.float32(GUIDANCE_SCALE),
                        temp_loss_scale=np.float32(TEMP_LOSS_SCALE), fps=np.int64(FPS), **arrays)
    print("wrote motion_sample_tiny.npz", {k: v.shape for k, v in arrays.items()},
          os.path.getsize(os.path.join(HERE, "motion_sample_tiny.npz")), "bytes")


if __name__ == "__main__":
    main()
