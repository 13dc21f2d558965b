"""Producer of the v2 latent records (reference ``preprocess_scripts/preprocess_with_motion_prior.py:310-409``,
``preprocess_no_motion_mp4.py:326-376``): what ``latent_io.LatentRecordDataset`` reads and ``distill.distill_step_v2`` trains on —

* ``encode_clips``: video -> scaled VAE latents (the native VAE encoder on the GPU);
* ``make_latent_records``: forward-diffusion sample, DDIM inversion, the teacher's two outputs and the motion-prior score of a batch
  of clips -> one pickled record per clip;
* ``write_latent_records``: the record files and the CSV the dataset opens.

CUDA tensors take the HIP kernels of csrc/train.hip between the teacher's forwards (``t2v_cd_add_noise``, ``t2v_ddim_reverse_step``,
``t2v_pack_f16_multi``: every per-clip coefficient looked up on the device, no host synchronisation before the one copy that brings
the records to the host).  CPU tensors — nothing then touches the library — and ``T2V_NATIVE_RECORD=0`` take the torch twin, the same
function composed from ``scheduler.add_noise``, ``motion_prior.reverse_ddim_loop``, ``get_motion_prior_score`` and
``pack_latent_record``; the ``*_torch`` functions below are also the specification the kernels are tested against (evaluated in
float64 when given float64 tensors)."""
import copy
import csv
import os

import torch

from . import cd_head, motion_prior
from .latent_io import pack_latent_record
from .native import shared_ops

RECORD_TENSORS = ("z_t", "cond_teacher_out", "uncond_teacher_out", "score", "z_example", "z_example_prev", "prompt_emb")


def native_enabled():
    """``T2V_NATIVE_RECORD`` (default 1), read at every call."""
    return os.environ.get("T2V_NATIVE_RECORD", "1") != "0"


# --------------------------------------------------------------------------------------------------------------- twins of the kernels
def _acp(alphas_cumprod, dev, cdt):
    return cd_head._table(alphas_cumprod, dev, torch.float32).to(cdt)     # (the fp32 table the kernels read)


def add_noise_torch(solver, alphas_cumprod, index, x, noise):
    """``T2VTurboScheduler.add_noise`` at t_s = ddim_timesteps[index] in fp32 (float64 for float64 inputs)."""
    cdt, dev = cd_head._compute_dtype(x), x.device
    acp = _acp(alphas_cumprod, dev, cdt)[cd_head._table(solver.ddim_timesteps, dev, torch.int64)[index.to(dev).long()]]
    shape = (-1,) + (1,) * (x.dim() - 1)
    return (acp ** 0.5).reshape(shape) * x.to(cdt) + ((1 - acp) ** 0.5).reshape(shape) * noise.to(cdt)


def ddim_reverse_step_torch(solver, alphas_cumprod, index, i, x, eps, prev=None, step_ratio=None):
    """Inversion step ``i`` of every clip, as ``t2v_ddim_reverse_step`` defines it, out of place: -> (x after the step, prev).  A clip
    with ``index < i`` keeps its state; a clip with ``index == i`` hands its old state to ``prev`` (returned as given otherwise)."""
    cdt, dev = cd_head._compute_dtype(x), x.device
    acp = _acp(alphas_cumprod, dev, cdt)
    step_ratio = solver.step_ratio if step_ratio is None else step_ratio
    t = cd_head._table(solver.ddim_timesteps, dev, torch.int64)[int(i)]
    a_next, a = acp[t], acp[torch.clamp(t - step_ratio, min=0)]
    x = x.to(cdt)
    e = eps.to(cdt)
    stepped = (x - (1 - a).sqrt() * e) * (a_next / a).sqrt() + (1 - a_next).sqrt() * e
    shape = (-1,) + (1,) * (x.dim() - 1)
    idx = index.to(dev).long().clamp(0, solver.ddim_timesteps.numel() - 1).reshape(shape)
    if prev is not None:
        prev = torch.where(idx == i, x, prev.to(cdt))
    return torch.where(idx >= i, stepped, x), prev


# --------------------------------------------------------------------------------------------------------------- small pieces
@torch.no_grad()
def encode_clips(vae, video, scale_factor=0.18215, generator=None):
    """Video -> scaled latents (B,4,T,h,w) through the VAE encoder (preprocess_with_motion_prior.py:316-324: ``encode(...).sample()``
    per frame, times ``scale_factor``): uint8 (B,T,H,W,C) frames, or float (B,T,C,H,W) in [-1, 1] as the reference's dataset yields
    them.  On the GPU every frame goes through the native encoder in one batched pass."""
    from .vae import DiagonalGaussianDistribution
    p = next(vae.parameters())
    if video.dtype == torch.uint8:
        video = video.to(p.device).permute(0, 1, 4, 2, 3).to(p.dtype) / 127.5 - 1.0
    else:
        video = video.to(p.device, p.dtype)
    moments = vae.encode_moments_video(video.transpose(1, 2).contiguous())          # (B,3,T,H,W) -> (B,8,T,h,w)
    post = DiagonalGaussianDistribution(moments.to(video.dtype))
    noise = torch.randn(post.mean.shape, generator=generator)
    return post.sample(noise.to(post.mean.dtype)) * scale_factor


def write_latent_records(root_dir, latent_root, relpaths, blobs, texts, csv_path):
    """``blobs[i]`` -> ``<root_dir>/<latent_root>/<relpaths[i]>`` and the annotation file ``csv_path`` (columns ``relpath,text``) that
    ``LatentRecordDataset(csv_path, latent_root, root_dir)`` opens."""
    assert len(relpaths) == len(blobs) == len(texts)
    for rel, blob in zip(relpaths, blobs):
        path = os.path.join(root_dir, latent_root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(blob)
    with open(csv_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["relpath", "text"])
        for rel, text in zip(relpaths, texts):
            w.writerow([rel, text])


# --------------------------------------------------------------------------------------------------------------- the producer
def _draw(solver, latents, motion, max_percentage, rng, generator):
    """index (CPU int64, validated) and noise (on the latents' device): pinned by ``rng`` or drawn on the host."""
    n_ddim, bsz = solver.ddim_timesteps.numel(), latents.shape[0]
    edge = int(n_ddim * (1 - max_percentage))
    lo, hi = (edge, n_ddim) if motion else (0, edge)
    index = rng["index"] if "index" in rng else torch.randint(lo, hi, (bsz,), generator=generator)
    index = index.cpu().long().reshape(bsz)
    cd_head.check_index(index, n_ddim)
    noise = rng["noise"] if "noise" in rng else torch.randn(latents.shape, generator=generator)
    return index, noise


def _records(index, tensors, text):
    """One ``pack_latent_record`` per clip from fp16 CPU tensors [B, ...]; every per-clip view is cloned first: a pickled view
    carries its whole storage."""
    blobs = []
    for b in range(index.shape[0]):
        rec = {k: tensors[k][b].clone() for k in RECORD_TENSORS}
        blobs.append(pack_latent_record(index[b].clone(), text=None if text is None else text[b], **rec))
    return blobs


def _make_torch(unet, solver, noise_scheduler, latents, prompt_embeds, uncond_prompt_embeds, index, noise, motion, fps, temp_loss_scale):
    """The twin: the reference's own sequence, clip by clip where the reference is limited to one clip (``index.item()``)."""
    dev, pdt = latents.device, next(unet.parameters()).dtype
    view = copy.copy(solver).to(dev)          # (``to`` rebinds attributes: the caller's solver stays where it is)
    index_dev = index.to(dev)
    start_timesteps = view.ddim_timesteps[index_dev]
    lat = latents.to(pdt)
    with torch.no_grad():
        z_t32 = noise_scheduler.add_noise(latents.float(), noise.to(dev, torch.float32), start_timesteps)          # (fp32, as the kernel)
        z_ts = z_t32.to(pdt)
        context = {"context": prompt_embeds.to(dev, pdt), "fps": fps}
        if motion:
            z_examples, z_examples_prev = [], []
            for b in range(lat.shape[0]):
                ctx_b = {"context": context["context"][b:b + 1], "fps": fps}
                inter = motion_prior.reverse_ddim_loop(lat[b:b + 1], unet, ctx_b, view, int(index[b]) + 1, dev)
                z_examples.append(inter[-1].float())
                z_examples_prev.append((inter[-2] if int(index[b]) > 0 else latents[b:b + 1]).float())
            z_examples, z_examples_prev = torch.cat(z_examples), torch.cat(z_examples_prev)
        uncond_out = unet(z_ts, start_timesteps, context=uncond_prompt_embeds.to(dev, pdt), fps=fps)
        if not motion:
            cond_out = unet(z_ts, start_timesteps, **context)
    if motion:
        scores, cond_out = [], []
        for b in range(lat.shape[0]):          # (the loss is a mean over the rows of the call: one clip per call, as the script runs)
            ctx_b = {"context": context["context"][b:b + 1], "fps": fps}
            s_b, c_b = motion_prior.get_motion_prior_score(unet, z_ts[b:b + 1].detach(), start_timesteps[b:b + 1],
                                                           z_examples[b:b + 1].to(pdt), ctx_b, ctx_b, temp_loss_scale)
            scores.append(s_b.detach())
            cond_out.append(c_b.detach())
        scores, cond_out = torch.cat(scores), torch.cat(cond_out)
    else:
        scores = z_examples = z_examples_prev = torch.zeros_like(z_ts)
    out = dict(z_t=z_t32, cond_teacher_out=cond_out.detach(), uncond_teacher_out=uncond_out, score=scores, z_example=z_examples,
               z_example_prev=z_examples_prev, prompt_emb=prompt_embeds)
    return {k: v.detach().to(torch.float16).cpu() for k, v in out.items()}, {"device_to_host_copies": len(out), "forwards": None}


def _make_native(ops, unet, solver, noise_scheduler, latents, prompt_embeds, uncond_prompt_embeds, index, noise, motion, fps,
                 temp_loss_scale):
    from .distill import _to_device_async
    dev, pdt = latents.device, next(unet.parameters()).dtype
    lp = pdt if pdt in (torch.bfloat16, torch.float16) else None          # the UNet's input: a rounded copy, or the fp32 state itself
    B = latents.shape[0]
    index_dev = _to_device_async(index, dev)
    start_timesteps = _to_device_async(cd_head._table(solver.ddim_timesteps, torch.device("cpu"), torch.int64)[index], dev)
    sched, tabs = cd_head._sched_struct(ops, solver, noise_scheduler.alphas_cumprod, index_dev, 0, 1.0)
    lat = latents.detach().contiguous()
    if lat.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        lat = lat.float()
    noise = _to_device_async(noise, dev).contiguous()
    forwards = 0
    with torch.no_grad():
        # 1. z_t = sqrt(acp[t_s]) x + sqrt(1 - acp[t_s]) noise, fp32 and the copy the teacher reads
        z_t = torch.empty(lat.shape, dtype=torch.float32, device=dev)
        z_in = torch.empty(lat.shape, dtype=lp, device=dev) if lp is not None else None
        ops.cd_add_noise(sched, lat, noise, z_t, z_in)
        z_in = z_t if z_in is None else z_in
        context = {"context": prompt_embeds.to(dev, pdt), "fps": fps}
        zeros = None
        if motion:
            # 2. inversion: max(index) + 1 batched forwards, each followed by one launch on the fp32 state
            x = lat.to(torch.float32, copy=True)
            x_in = lat.to(lp, copy=True) if lp is not None else None
            prev = torch.empty_like(x)
            n_steps = int(index.max()) + 1          # (from the CPU tensor: no device synchronisation)
            ts_grid = tabs[1][:n_steps, None].expand(n_steps, B).contiguous()
            for i in range(n_steps):
                eps = unet(x if x_in is None else x_in, ts_grid[i], **context)
                forwards += 1
                if eps.dtype not in (torch.float32, torch.bfloat16):
                    eps = eps.float()
                ops.ddim_reverse_step(sched, i, solver.step_ratio, x, eps.contiguous(), prev, x_in)
            z_example, z_example_prev = x, prev
        else:
            zeros = torch.zeros(lat.shape, dtype=torch.float16, device=dev)
        # 3. the unconditional teacher output
        uncond_out = unet(z_in, start_timesteps, context=uncond_prompt_embeds.to(dev, pdt), fps=fps)
        forwards += 1
        if not motion:
            cond_out = unet(z_in, start_timesteps, **context)
            forwards += 1
    if motion:
        # 4. the motion-prior score on the input-gradient route: score and the conditional teacher output.  The loss is a mean over the
        # rows of the call and the clips do not mix: one batched call at B times the scale gives every clip the score of its own call.
        score, cond_out = motion_prior.get_motion_prior_score(unet, z_in.detach(), start_timesteps,
                                                              z_example if x_in is None else x_in, context, context, temp_loss_scale * B)
        forwards += 2
    else:
        score = z_example = z_example_prev = zeros
    # 5. one launch: every tensor of every clip into [B][z_t | cond | uncond | score | z_example | z_example_prev | prompt_emb] fp16
    srcs = [z_t, cond_out.detach(), uncond_out, score, z_example, z_example_prev, prompt_embeds.to(dev)]
    srcs = [(t if t.dtype in (torch.float32, torch.bfloat16, torch.float16) else t.float()).contiguous() for t in srcs]
    sizes = [t.numel() // B for t in srcs]
    rec = sum(sizes)
    packed = torch.empty((B, rec), dtype=torch.float16, device=dev)
    entries, off = [], 0
    for t, n in zip(srcs, sizes):
        entries.append((t, off, B, rec))
        off += n
    ops.pack_f16_multi(entries, packed)
    # 6. one copy into pinned memory (this is where the host waits for the device)
    host = torch.empty((B, rec), dtype=torch.float16, pin_memory=True)
    host.copy_(packed, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    out, off = {}, 0
    for k, t, n in zip(RECORD_TENSORS, srcs, sizes):
        out[k] = host[:, off:off + n].reshape(t.shape)
        off += n
    return out, {"device_to_host_copies": 1, "forwards": forwards}


def make_latent_records(unet, solver, noise_scheduler, latents, prompt_embeds, uncond_prompt_embeds, *, motion=True, fps=8, topk=5,
                        max_percentage=0.5, temp_loss_scale=100.0, text=None, rng=None, generator=None):
    """Records of a batch of clips -> (list of ``bytes``, one pickled record per clip; info).

    ``motion=True`` is ``preprocess_with_motion_prior.py:328-409`` for one process: index in [int(n_ddim (1 - max_percentage)), n_ddim),
    z_t by forward diffusion, ``index + 1`` steps of DDIM inversion of the clean latent (``z_example``, ``z_example_prev``), the
    unconditional teacher output, and the motion-prior score together with the conditional teacher output.  ``motion=False`` is
    ``preprocess_no_motion_mp4.py:326-376``: index in [0, int(n_ddim (1 - max_percentage))), the two teacher outputs, zeros for
    ``score`` / ``z_example`` / ``z_example_prev``, and ``text`` stored in the record.

    ``unet``: the frozen teacher in eval mode (built with ``record_attn_probs=True`` for ``motion=True``); ``latents``: scaled VAE
    latents (B,4,F,h,w) (``encode_clips``); ``prompt_embeds`` / ``uncond_prompt_embeds``: (B,77,D); ``text``: a caption per clip or
    None.  ``rng`` may pin the draws for tests: dict(index, noise); ``generator``: a CPU generator for both.  ``topk`` is recorded in
    ``info`` (the script computes ``timesteps`` from it and never uses them).

    On CUDA tensors the inversion runs ALL clips of the batch together: max(index) + 1 batched forwards, each followed by one launch
    that keeps the inverted latent in fp32 in place and freezes a clip once its own ``index + 1`` steps are done.  The reference's
    ``index.item()`` limits it to one clip per call; the per-clip freeze lifts that limit at the price of idle forwards for the clips
    with a smaller index (their rows of the batched forward are computed and not used).  ``index`` is validated and the loop count is
    taken while it is a CPU tensor; the host first waits for the device at the single copy that brings the records back."""
    rng = rng or {}
    if unet.training or any(p.requires_grad for p in unet.parameters()):
        raise ValueError("make_latent_records: the teacher must be frozen and in eval mode")
    assert not getattr(solver, "use_scale", False), "use_scale = True is out of scope"
    bsz = latents.shape[0]
    assert prompt_embeds.shape[0] == bsz and uncond_prompt_embeds.shape[0] == bsz and (text is None or len(text) == bsz)
    index, noise = _draw(solver, latents, motion, max_percentage, rng, generator)
    native = latents.is_cuda and native_enabled()
    route = unet.native_input_grad if hasattr(type(unet), "native_input_grad") else None
    if motion and latents.is_cuda and route is None:
        unet.native_input_grad = True          # the score's differentiated pass on the data-gradient engine
    try:
        if native:
            with torch.cuda.device(latents.device):
                tensors, info = _make_native(shared_ops(), unet, solver, noise_scheduler, latents, prompt_embeds, uncond_prompt_embeds,
                                             index, noise, motion, fps, temp_loss_scale)
        else:
            tensors, info = _make_torch(unet, solver, noise_scheduler, latents, prompt_embeds, uncond_prompt_embeds, index, noise, motion,
                                        fps, temp_loss_scale)
    finally:
        if motion and latents.is_cuda and route is None:
            unet.native_input_grad = None
    blobs = _records(index, tensors, None if motion else text)          # (the motion script stores no caption, the other one does)
    info.update(native=native, index=index, topk=topk, start_timesteps=cd_head._table(solver.ddim_timesteps, torch.device("cpu"),
                                                                                       torch.int64)[index])
    return blobs, info
