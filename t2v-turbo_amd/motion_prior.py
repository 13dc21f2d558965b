"""Motion-prior preprocessing around the denoiser: DDIM inversion — a pure consumer of the
native UNet forward, ``len(solver.ddim_timesteps)`` sequential calls — temporal attention-probability capture and the
motion-prior score (``motion_prior_sample.py:27-84``, ``utils/common_utils.py:446-478``) — and the sampler that consumes them,
``motion_prior_sample`` (``motion_prior_sample.py:146-297``): DDIM sampling with CFG from a reference clip's inverted latents, the noise
estimate of the first ``percentage`` of the steps steered by the motion-prior score (and optionally by an image-reward gradient), with
``video_to_uint8`` for the frames at the end.

CUDA tensors take one HIP launch between the forwards of a sampling step (``t2v_mp_guided_step``, csrc/train.hip: the latent stays fp32
in place, no host synchronisation before the single copy that brings the new ``motion_intermediate`` entries to the host) and one launch
for the uint8 frames (``t2v_video_to_u8``, csrc/elementwise.hip).  CPU tensors and ``T2V_NATIVE_MP_SAMPLE=0`` take the torch twin, the
script's own sequence written with ``cd_math``; ``mp_guided_step_torch`` is also the specification the kernel is tested against
(evaluated in float64 when given float64 tensors)."""
import os
import types

import torch
import torch.nn.functional as F

from . import cd_head, cd_math
from .native import RANK_LOSS_MAX, shared_ops

MOTION_INTERMEDIATE_KEYS = ("cond_pred_x_0", "uncond_pred_x_0", "cond_pred_noise", "uncond_pred_noise", "score")

ATTN_PROB_BLOCKS = tuple(f"output_blocks.{i}.2" for i in range(3, 12))


@torch.no_grad()
def reverse_ddim_loop(latents, unet, context, solver, num_inference_steps, device):
    """motion_prior_sample.py:27-37: x_{t_i} from x_{t_{i-1}} with the model's own noise prediction (no grad: every call
    runs on the native engine when the UNet is on a GPU)."""
    intermediate_latents = []
    for i in range(num_inference_steps):
        index = torch.full((1,), i, device=device, dtype=torch.long)
        ts = solver.ddim_timesteps[index].long()
        pred_noise = unet(latents, ts, **context)
        latents = solver.ddim_reverse_step(latents, pred_noise, ts)
        intermediate_latents.append(latents)
    return intermediate_latents


def get_temp_attn_prob(unet, latent, ts, context):
    """motion_prior_sample.py:40-57: forward + the temporal attn1 probabilities of output_blocks 3..11 (the UNet must have
    been built with ``record_attn_probs=True``)."""
    model_output = unet(latent, ts, **context)
    attention_prob = {}
    for name, module in unet.named_modules():
        if name.startswith(ATTN_PROB_BLOCKS) and name.endswith("blocks.0.attn1"):
            attention_prob[name] = module.attention_probs
    return model_output, attention_prob


def calculate_motion_rank_new(tensor_ref, tensor_gen, rank_k=1):
    """utils/common_utils.py:446-461: MSE on the top-``rank_k`` entries (by reference value) of each probability row."""
    if rank_k == 0:
        return torch.tensor(0.0, device=tensor_ref.device)
    if rank_k > tensor_ref.shape[-1]:
        raise ValueError("The value of rank_k cannot be larger than the number of frames")
    _, sorted_indices = torch.sort(tensor_ref, dim=-1)
    mask = torch.zeros_like(tensor_ref, dtype=torch.bool)
    mask.scatter_(-1, sorted_indices[..., -rank_k:], True)
    return F.mse_loss(tensor_ref[mask].detach(), tensor_gen[mask])


def compute_temp_loss(attention_prob, attention_prob_example):
    """utils/common_utils.py:464-478."""
    losses = [calculate_motion_rank_new(attention_prob_example[name].detach(), attention_prob[name], rank_k=1)
              for name in attention_prob.keys()]
    return (torch.stack(losses) * 100).mean()


def _selection(ref, rank_k):
    """The entries of each row that ``calculate_motion_rank_new`` compares: the last ``rank_k`` places of a stable ascending sort."""
    idx = torch.sort(ref, dim=-1, stable=True).indices[..., -rank_k:]
    return torch.zeros_like(ref, dtype=torch.bool).scatter_(-1, idx, True)


def compute_temp_loss_fused(attention_prob, attention_prob_example, rank_k=1, scale=1.0):
    """``scale * compute_temp_loss`` (for any ``rank_k`` >= 1) together with its gradient, without autograd:
    -> (loss, 0-d tensor; {name: d(loss) / d(attention_prob[name])}).  With P layers of rows_p rows,
        loss = scale * mean_p(100 * loss_p),  loss_p = sum over the selected entries of (gen - ref)^2 / (rows_p * rank_k),
        d(loss) / d(gen_p) = scale * 100 / P * 2 / (rows_p * rank_k) * (gen - ref) on the selected entries, 0 elsewhere.
    CUDA tensors: ONE ``t2v_rank_loss`` call for all layers (per width of the last dimension, 16 layers at a time), instead of a
    sort, a scatter, a boolean gather and an MSE through autograd per layer; CPU tensors: the closed form above in torch."""
    names = list(attention_prob.keys())
    if rank_k < 1 or any(rank_k > attention_prob[nm].shape[-1] for nm in names):
        raise ValueError("rank_k must be between 1 and the number of frames")
    P = len(names)
    alpha = float(scale) * 100.0 / P
    gens = {nm: attention_prob[nm].detach() for nm in names}
    refs = {nm: attention_prob_example[nm].detach() for nm in names}
    grads = {}
    if not gens[names[0]].is_cuda:
        loss = 0.0
        for nm in names:
            gen, ref = gens[nm].float(), refs[nm].float()
            sel = _selection(ref, rank_k)
            count = ref.numel() // ref.shape[-1] * rank_k
            d = torch.where(sel, gen - ref, torch.zeros_like(gen))
            loss = loss + (d * d).sum() / count
            grads[nm] = (alpha * 2.0 / count * d).to(gens[nm].dtype)
        return alpha * loss, grads
    ops = shared_ops()
    dev = gens[names[0]].device
    loss_p = torch.empty(P, dtype=torch.float32, device=dev)
    by_n = {}
    for i, nm in enumerate(names):
        by_n.setdefault(gens[nm].shape[-1], []).append(i)
    with torch.cuda.device(dev):
        for n, members in by_n.items():
            for c in range(0, len(members), RANK_LOSS_MAX):
                chunk = members[c:c + RANK_LOSS_MAX]
                problems = []
                for i in chunk:
                    gen, ref = gens[names[i]].float().contiguous(), refs[names[i]].float().contiguous()
                    problems.append((ref, gen, torch.empty_like(gen)))
                ws = torch.empty(ops.rank_loss_ws_floats([g.numel() // n for _, g, _ in problems], n), dtype=torch.float32, device=dev)
                out = torch.empty(len(chunk), dtype=torch.float32, device=dev)
                ops.rank_loss(problems, n, rank_k, alpha, ws, out)
                for j, i in enumerate(chunk):
                    grads[names[i]] = problems[j][2].to(gens[names[i]].dtype)
                if len(chunk) == P:
                    loss_p = out
                else:
                    loss_p[torch.tensor(chunk, device=dev)] = out
    return loss_p.sum() * alpha, grads


def get_motion_prior_score(unet, latents, ts, example_latent, original_context, inference_context, temp_loss_scale):
    """motion_prior_sample.py:59-84: d(temp loss)/d(latents).  The example pass needs no gradient (native engine).  The
    differentiated pass is the module call: the torch composite path by default, the data-gradient engine with
    ``unet.native_input_grad`` on (unet3d.UNetModel, route "input_grad").  With that route on and CUDA tensors the loss between the
    probabilities is the fused kernel (``compute_temp_loss_fused``) and its gradients enter ``autograd.grad`` as ``grad_outputs``:
    two engine passes with one launch pair in between."""
    with torch.no_grad():
        _, attention_prob_example = get_temp_attn_prob(unet, example_latent, ts, original_context)
    with torch.set_grad_enabled(True):
        latents.requires_grad_(True)
        cond_teacher_output, attention_prob = get_temp_attn_prob(unet, latents, ts, inference_context)
        route_on = getattr(unet, "input_grad_route_on", None)
        if latents.is_cuda and route_on is not None and route_on():
            names = list(attention_prob.keys())
            _, grads = compute_temp_loss_fused(attention_prob, attention_prob_example, rank_k=1, scale=temp_loss_scale)
            score = torch.autograd.grad([attention_prob[nm] for nm in names], latents,
                                        grad_outputs=[grads[nm] for nm in names])[0].detach()
        else:
            loss = temp_loss_scale * compute_temp_loss(attention_prob, attention_prob_example)
            score = torch.autograd.grad(loss, latents)[0].detach()
    return score, cond_teacher_output


def get_motion_prior_score_native(grad_engine, unet, latents, ts, example_latent, original_context, inference_context,
                                  temp_loss_scale):
    """Same result as ``get_motion_prior_score`` with the differentiated pass on the UNet data-gradient engine
    (``engine_unet_bwd.UNetGradEngine``): forward with tape, the (tiny) loss on the recorded probabilities differentiated by
    autograd w.r.t. those probabilities only, and the engine's backward from there to the latents."""
    with torch.no_grad():
        _, attention_prob_example = get_temp_attn_prob(unet, example_latent, ts, original_context)
        attention_prob_example = {k: v.clone() for k, v in attention_prob_example.items()}  # the next forward reuses the buffers
    ctx = dict(inference_context)
    out = grad_engine.forward_tape(latents.detach(), ts, ctx["context"], ctx.get("fps", 16), ctx.get("timestep_cond"),
                                   ctx.get("motion_cond"))
    modules = dict(unet.named_modules())
    names = [n for n in attention_prob_example if n in modules]
    leaves = {n: modules[n].attention_probs.detach().clone().requires_grad_(True) for n in names}
    with torch.set_grad_enabled(True):
        loss = temp_loss_scale * compute_temp_loss(leaves, attention_prob_example)
        grads = torch.autograd.grad(loss, [leaves[n] for n in names])
    score = grad_engine.backward(None, {modules[n]: g for n, g in zip(names, grads)})
    return score.detach(), out



# --------------------------------------------------------------------------------------------------------------- uint8 frames
def video_to_uint8(videos):
    """Decoded video (B,3,T,H,W) in [-1, 1] (``decode_first_stage_2DAE``) -> frames (B,T,H,W,3) uint8: the tail of every entry point of the
    reference (``predict.py:129-137``, ``motion_prior_sample.py:299-301``), ``((v.float().clamp(-1, 1) + 1.0) / 2.0 * 255).to(uint8)``
    with the channels last; NaN gives 0.  CUDA: one launch (``t2v_video_to_u8``), the same bytes."""
    assert videos.dim() == 5 and videos.shape[1] == 3, "video_to_uint8: (B,3,T,H,W)"
    if videos.is_cuda:
        v = videos.detach()
        if v.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            v = v.float()
        v = v.contiguous()
        B, _, T, H, W = v.shape
        out = torch.empty((B, T, H, W, 3), dtype=torch.uint8, device=v.device)
        with torch.cuda.device(v.device):
            shared_ops().video_to_u8(v, out)
        return out
    v = torch.nan_to_num(videos.detach().float(), nan=-1.0)
    return ((v.clamp(-1.0, 1.0) + 1.0) / 2.0 * 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()


# --------------------------------------------------------------------------------------------------------------- the sampler
def native_sample_enabled():
    """``T2V_NATIVE_MP_SAMPLE`` (default 1), read at every call."""
    return os.environ.get("T2V_NATIVE_MP_SAMPLE", "1") != "0"


def guided_steps(percentage, num_inference_steps):
    """The steps whose noise estimate is steered: ``i > n - percentage * n`` (motion_prior_sample.py:160), evaluated as the script does."""
    n = num_inference_steps
    return [i for i in range(n) if i > n - percentage * n]


@torch.no_grad()
def mp_guided_step_torch(solver, alphas_cumprod, i, guidance_scale, x, cond, uncond, score=None, x0_cond=None, x0_uncond=None):
    """The head of sampling step ``i`` (motion_prior_sample.py:180-196, 283-292 with ``use_scale = False``), in fp32 (float64 for a
    float64 ``x``), out of place -> dict(x, pred_x0, x0_cond, x0_uncond).  Every clip is at step ``i``; ``x0_cond`` / ``x0_uncond``:
    both None (formed from ``x``) or both given (a cached ``motion_intermediate`` entry); ``score`` None: no motion term."""
    assert (x0_cond is None) == (x0_uncond is None)
    cdt, dev, bsz = cd_head._compute_dtype(x), x.device, x.shape[0]
    alpha_schedule, sigma_schedule = cd_head._schedules(alphas_cumprod, dev, cdt)
    index = torch.full((bsz,), int(i), device=dev, dtype=torch.long)
    ts = cd_head._table(solver.ddim_timesteps, dev, torch.int64)[index]
    xx, c, u = x.to(cdt), cond.to(cdt), uncond.to(cdt)
    if x0_cond is None:
        x0c = cd_math.get_predicted_original_sample(c, ts, xx, "epsilon", alpha_schedule, sigma_schedule)
        x0u = cd_math.get_predicted_original_sample(u, ts, xx, "epsilon", alpha_schedule, sigma_schedule)
    else:
        x0c, x0u = x0_cond.to(cdt), x0_uncond.to(cdt)
    pred_x0 = x0c + guidance_scale * (x0c - x0u)
    pred_noise = c + guidance_scale * (c - u)
    if score is not None:
        alphas = cd_math.extract_into_tensor(alpha_schedule, ts, xx.shape)
        pred_noise = pred_noise - (1 - alphas) ** 0.5 * score.to(cdt)
    view = types.SimpleNamespace(ddim_alpha_cumprods_prev=cd_head._table(solver.ddim_alpha_cumprods_prev, dev, torch.float32).to(cdt),
                                 use_scale=False)
    return dict(x=cd_math.DDIMSolver.ddim_step(view, pred_x0, pred_noise, index), pred_x0=pred_x0, x0_cond=x0c, x0_uncond=x0u)


def _rows(ctx, b):
    """Clip ``b`` of a context dict (tensors with a batch dimension are sliced, everything else passes)."""
    return {k: (v[b:b + 1] if torch.is_tensor(v) and v.dim() > 0 else v) for k, v in ctx.items()}


def _ctx_to(ctx, dev, dtype):
    return {k: (v.to(dev, dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in ctx.items()}


def _reward_score(latents, cond, uncond, i, guidance_scale, solver, alphas_cumprod, vae, vae_scale_factor, reward_fn, reward_scale,
                  reward_batch_size, text, rng, generator):
    """motion_prior_sample.py:231-255, clip by clip: d(-reward.mean() * reward_scale) / d(latents) through
    ``pred_x_0 = (latents - sg eps_cfg) / a`` on ``reward_batch_size`` random frames, ``vae.decode`` (on the GPU: the native decode
    gradient) and the caller's ``reward_fn(images in [0, 1], text)``.  The elementwise ops around the decode stay with autograd."""
    dev = latents.device
    alpha_schedule, sigma_schedule = cd_head._schedules(alphas_cumprod, dev, torch.float32)
    t = int(solver.ddim_timesteps[int(i)])          # (a CPU table: no device synchronisation)
    a, sg = alpha_schedule[t], sigma_schedule[t]
    vdt = next(vae.parameters()).dtype
    pred_noise = (cond.float() + guidance_scale * (cond.float() - uncond.float())).detach()
    grads = []
    for b in range(latents.shape[0]):
        idx = rng["reward_frames"] if "reward_frames" in rng else torch.randint(0, latents.shape[2], (reward_batch_size,), generator=generator)
        idx = idx.to(dev)
        with torch.enable_grad():
            lat = latents[b:b + 1].detach().float().clone().requires_grad_(True)
            pred_x_0 = (lat - sg * pred_noise[b:b + 1]) / a
            sel = pred_x_0[:, :, idx].to(vdt) / vae_scale_factor
            sel = sel.permute(0, 2, 1, 3, 4)
            sel = sel.reshape(idx.numel(), *sel.shape[2:])
            imgs = (vae.decode(sel) / 2 + 0.5).clamp(0, 1)
            rewards = reward_fn(imgs, None if text is None else (text[b] if isinstance(text, (list, tuple)) else text))
            loss = -rewards.mean() * reward_scale
            grads.append(torch.autograd.grad(loss, lat)[0].detach())
    return torch.cat(grads)


def _entry_to(entry, dev, dtype=None):
    return [entry[k].to(dev) if dtype is None else entry[k].to(dev, dtype) for k in MOTION_INTERMEDIATE_KEYS]


def _sample_torch(unet, solver, noise_scheduler, original_latents, intermediate_latents, inference_context, original_context,
                  uncond_context, noise, guidance_scale, guided, temp_loss_scale, cached, return_sampled, reward, span):
    """The twin: the script's own sequence; the state is cast to the UNet's dtype after each step, the score clip by clip (the loss
    is a mean over the rows of a call)."""
    dev, pdt = original_latents.device, next(unet.parameters()).dtype
    n, B = solver.ddim_timesteps.numel(), original_latents.shape[0]
    acp = noise_scheduler.alphas_cumprod
    inf_ctx, org_ctx, unc_ctx = (_ctx_to(c, dev, pdt) for c in (inference_context, original_context, uncond_context))
    ts_table = cd_head._table(solver.ddim_timesteps, dev, torch.int64)
    with torch.no_grad():
        latents = noise_scheduler.add_noise(original_latents.to(pdt), noise.to(dev, pdt), ts_table[n - 1].expand(B)).to(pdt)
    start_latents, start, stop = span
    if start_latents is not None:
        latents = start_latents.to(dev, pdt)
    entries, sampled, forwards, copies = [], [], 0, 0
    for i in range(start, stop - 1, -1):
        ts = ts_table[i].expand(B).contiguous()
        k = n - 1 - i
        x0c = x0u = score = None
        if i in guided and k < len(cached):
            x0c, x0u, cond, uncond, score = _entry_to(cached[k], dev, pdt)
            entries.append(cached[k])
        elif i in guided:
            scores, conds = [], []
            for b in range(B):
                s_b, c_b = get_motion_prior_score(unet, latents[b:b + 1].detach().clone(), ts[b:b + 1], intermediate_latents[i][b:b + 1].to(dev, pdt),
                                                  _rows(org_ctx, b), _rows(inf_ctx, b), temp_loss_scale)
                scores.append(s_b.detach())
                conds.append(c_b.detach())
            score, cond = torch.cat(scores), torch.cat(conds)
            with torch.no_grad():
                uncond = unet(latents, ts, **unc_ctx)
            forwards += 2 * B + 1
        else:
            with torch.no_grad():
                cond, uncond = unet(latents, ts, **inf_ctx), unet(latents, ts, **unc_ctx)
            forwards += 2
        entry_score = score
        if i in guided and reward is not None:
            score = score.float() + _reward_score(latents, cond, uncond, i, guidance_scale, solver, acp, **reward)
        out = mp_guided_step_torch(solver, acp, i, guidance_scale, latents, cond, uncond, score, x0c, x0u)
        if i in guided and k >= len(cached):
            vals = (out["x0_cond"], out["x0_uncond"], cond, uncond, entry_score)
            entries.append({key: v.detach().to(torch.float16).cpu() for key, v in zip(MOTION_INTERMEDIATE_KEYS, vals)})
            copies += len(vals)
        latents = out["x"].to(pdt)
        if return_sampled:
            sampled.append(out["pred_x0"])
    return latents, entries, sampled, forwards, copies


def _sample_native(ops, unet, solver, noise_scheduler, original_latents, intermediate_latents, inference_context, original_context,
                   uncond_context, noise, guidance_scale, guided, temp_loss_scale, cached, return_sampled, reward, span):
    from .distill import _to_device_async
    dev, pdt = original_latents.device, next(unet.parameters()).dtype
    lp = pdt if pdt in (torch.bfloat16, torch.float16) else None          # the UNet's input: a rounded copy, or the fp32 state itself
    n, B = solver.ddim_timesteps.numel(), original_latents.shape[0]
    acp = noise_scheduler.alphas_cumprod
    inf_ctx, org_ctx, unc_ctx = (_ctx_to(c, dev, pdt) for c in (inference_context, original_context, uncond_context))
    tabs = (cd_head._table(acp, dev, torch.float32), cd_head._table(solver.ddim_timesteps, dev, torch.int64),
            cd_head._table(solver.ddim_alpha_cumprods_prev, dev, torch.float32))
    last = torch.full((B,), n - 1, dtype=torch.int64, device=dev)
    sched = ops.cd_sched(*tabs, last, 0, 1.0)          # (index: read by the forward-diffusion sample only)
    lat = original_latents.detach().to(pdt).contiguous()          # (the script diffuses the latents in the UNet's dtype)
    noise = _to_device_async(noise, dev).to(pdt).contiguous()
    x = torch.empty(lat.shape, dtype=torch.float32, device=dev)
    x_lp = torch.empty(lat.shape, dtype=lp, device=dev) if lp is not None else None
    ops.cd_add_noise(sched, lat, noise, x, x_lp)
    start_latents, start, stop = span
    if start_latents is not None:
        x.copy_(start_latents)
        if x_lp is not None:
            x_lp.copy_(x)
    x_in = x if x_lp is None else x_lp
    ts_grid = tabs[1][:, None].expand(n, B).contiguous()
    new = [i for i in sorted(guided, reverse=True) if n - 1 - i >= len(cached) and stop <= i <= start]
    examples = {i: _to_device_async(intermediate_latents[i].detach(), dev).to(pdt) for i in new}
    rec = torch.empty((len(new), B, 5) + tuple(lat.shape[1:]), dtype=torch.float16, device=dev) if new else None
    sampled = [torch.empty(lat.shape, dtype=torch.float32, device=dev) for _ in range(start - stop + 1)] if return_sampled else []
    entries, forwards, n_new = [], 0, 0
    for i in range(start, stop - 1, -1):
        ts = ts_grid[i]
        k = n - 1 - i
        x0c = x0u = score = rec_i = None
        if i in guided and k < len(cached):
            # a cached entry: no forward; its five tensors go to the kernel as they are
            x0c, x0u, cond, uncond, score = (t.contiguous() for t in _entry_to(cached[k], dev))
            if cond.dtype != uncond.dtype or x0c.dtype != x0u.dtype:
                x0c, x0u, cond, uncond = (t.float() for t in (x0c, x0u, cond, uncond))
            entries.append(cached[k])
        elif i in guided:
            # score and conditional output on the input-gradient route: the loss is a mean over the rows of the call and the clips do
            # not mix, so one batched call at B times the scale gives every clip the score of its own call
            score, cond = get_motion_prior_score(unet, x_in.detach(), ts, examples.pop(i), org_ctx, inf_ctx, temp_loss_scale * B)
            cond = cond.detach()
            with torch.no_grad():
                uncond = unet(x_in, ts, **unc_ctx)
            forwards += 3
            rec_i = rec[n_new]
            n_new += 1
            entries.append(None)
        else:
            with torch.no_grad():
                cond, uncond = unet(x_in, ts, **inf_ctx), unet(x_in, ts, **unc_ctx)
            forwards += 2
        if cond.dtype != uncond.dtype or cond.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            cond, uncond = cond.float(), uncond.float()
        if score is not None and score.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            score = score.float()
        step_score = score
        if i in guided and reward is not None:
            step_score = score.float() + _reward_score(x_in, cond, uncond, i, guidance_scale, solver, acp, **reward)
        with torch.no_grad():
            ops.mp_guided_step(sched, i, guidance_scale, x, cond.contiguous(), uncond.contiguous(), x0c, x0u,
                               None if step_score is None else step_score.contiguous(), x_lp, sampled[start - i] if return_sampled else None, rec_i)
            if rec_i is not None and step_score is not score:
                # the entry holds the motion score alone (the script appends it before the reward gradient is added)
                per = x[0].numel()
                ops.pack_f16_multi([(score.contiguous(), 4 * per, B, 5 * per)], rec_i.view(-1))
    copies = 0
    if new:
        # one copy into pinned memory, allocated once: this is where the host first waits for the device
        host = torch.empty(rec.shape, dtype=torch.float16, pin_memory=True)
        host.copy_(rec, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        copies = 1
        j = 0
        for e in range(len(entries)):
            if entries[e] is None:
                entries[e] = {key: host[j, :, slot].clone() for slot, key in enumerate(MOTION_INTERMEDIATE_KEYS)}          # (a pickled view carries its whole storage)
                j += 1
    return x, entries, sampled, forwards, copies


def motion_prior_sample(unet, solver, noise_scheduler, original_latents, intermediate_latents, inference_context, original_context,
                        uncond_context, *, guidance_scale=7.5, percentage=0.6, temp_loss_scale=100.0, motion_intermediate=None,
                        return_sampled=False, vae=None, vae_scale_factor=0.18215, reward_fn=None, reward_scale=0.0, reward_batch_size=12,
                        text=None, rng=None, generator=None):
    """The motion-clone sampler (``motion_prior_sample.py:146-297``) for one process and B >= 1 clips -> (latents, info).

    ``original_latents``: the reference clips' scaled VAE latents (B,4,F,h,w); ``intermediate_latents``: their DDIM inversion, one
    (B,4,F,h,w) tensor per solver step (``reverse_ddim_loop`` under ``original_context``); the three contexts: dicts of ``context``
    (B,77,D) and ``fps``.  ``latents = add_noise(original_latents, noise, ddim_timesteps[-1])``, then the steps i = n-1 ... 0: while
    ``i > n - percentage * n`` the CFG noise estimate is steered by ``sqrt(1 - a) score`` with the motion-prior score of the temporal
    attention maps against ``intermediate_latents[i]`` (three forwards), afterwards plain CFG (two forwards).  ``motion_intermediate``: a
    list of earlier entries, in step order; a guided step that finds its entry there runs no forward.  ``reward_fn(images, text)``
    with ``vae`` and ``reward_scale > 0``: the score of a guided step additionally gets d(-reward.mean() reward_scale) / d(latents)
    through ``reward_batch_size`` random frames of the predicted x0.  ``rng`` may pin ``noise`` and ``reward_frames``; ``generator``: a
    CPU generator for both.

    On CUDA tensors the state stays fp32, in place, between the steps (the returned latents are that fp32 state) and one launch
    follows the forwards of a step; a batch takes ONE score call at ``B x temp_loss_scale``; the new ``motion_intermediate`` entries come
    to the host in one copy, which is where the host first waits for the device.  ``T2V_NATIVE_MP_SAMPLE=0`` and CPU tensors take the
    torch twin (the state rounded to the UNet's dtype after each step, as the script does; the score clip by clip).

    ``info``: ``motion_intermediate`` (a list of dicts of CPU fp16 tensors under the script's keys), ``sampled_latents`` (the predicted
    x0 of every step, with ``return_sampled``), ``forwards``, ``device_to_host_copies``, ``native``."""
    rng = rng or {}
    if unet.training or any(p.requires_grad for p in unet.parameters()):
        raise ValueError("motion_prior_sample: the UNet must be frozen and in eval mode")
    if not any(getattr(m, "record_attn_probs", False) for m in unet.modules()):
        raise ValueError("motion_prior_sample: the UNet must be built with record_attn_probs=True")
    if getattr(solver, "use_scale", False):
        raise ValueError("motion_prior_sample: use_scale = True is out of scope")
    n = solver.ddim_timesteps.numel()
    if len(intermediate_latents) < n:
        raise ValueError(f"motion_prior_sample: {len(intermediate_latents)} inverted latents for a grid of {n} steps")
    if reward_fn is not None and vae is None:
        raise ValueError("motion_prior_sample: reward_fn needs the vae")
    cached = list(motion_intermediate or [])
    guided = set(guided_steps(percentage, n))
    noise = rng["noise"] if "noise" in rng else torch.randn(original_latents.shape, generator=generator)
    reward = None
    if reward_fn is not None and reward_scale > 0.0:
        reward = dict(vae=vae, vae_scale_factor=vae_scale_factor, reward_fn=reward_fn, reward_scale=reward_scale,
                      reward_batch_size=reward_batch_size, text=text, rng=rng, generator=generator)
    native = original_latents.is_cuda and native_sample_enabled()
    route = unet.native_input_grad if hasattr(type(unet), "native_input_grad") else None
    switch = original_latents.is_cuda and route is None and hasattr(type(unet), "native_input_grad")
    if switch:
        unet.native_input_grad = True          # the score's differentiated pass on the data-gradient engine
    # (for tests: ``rng`` may also restart the loop — ``start_latents`` is the state in front of step ``start_step`` — and end it after
    # step ``stop_step``; a cached entry keeps its place, n - 1 - i, in ``motion_intermediate``)
    span = (rng.get("start_latents"), int(rng.get("start_step", n - 1)), int(rng.get("stop_step", 0)))
    if not 0 <= span[2] <= span[1] < n:
        raise ValueError("motion_prior_sample: 0 <= stop_step <= start_step < n")
    args = (unet, solver, noise_scheduler, original_latents, intermediate_latents, inference_context, original_context, uncond_context,
            noise, float(guidance_scale), guided, temp_loss_scale, cached, return_sampled, reward, span)
    try:
        if native:
            with torch.cuda.device(original_latents.device):
                latents, entries, sampled, forwards, copies = _sample_native(shared_ops(), *args)
        else:
            latents, entries, sampled, forwards, copies = _sample_torch(*args)
    finally:
        if switch:
            unet.native_input_grad = None
    info = dict(motion_intermediate=entries, forwards=forwards, device_to_host_copies=copies, native=native)
    if return_sampled:
        info["sampled_latents"] = sampled
    return latents, info
