"""Data gradient of the UNet forward: d(loss)/d(latents) for a loss on the denoiser output and / or on the recorded
temporal attention probabilities — what ``get_motion_prior_score`` asks of autograd (``motion_prior_sample.py:59-84``:
``latents.requires_grad_(True)`` -> UNet -> ``attn1.attention_probs`` of the output-block temporal transformers ->
``autograd.grad(loss, latents)``), and the native student backward of the distillation step.  With frozen
weights only data gradients are computed, and the conditioning branch (time / fps / guidance embeddings, text K / V) carries
none because it does not depend on the latents.  With the LoRA tensors bound (``bind_lora``, engine_lora.py) the same tape also
runs the un-merged LoRA branch of every injected leaf, takes its weight gradients at the leaf's backward, applies the
train-mode dropouts, and hands d(loss)/d(emb_all) back for the conditioning branch that stays in torch.

Same construction as the VAE decoder's gradient engine: the forward is recorded together with a *tape* of closures, each
recording its block's backward launches; forward and backward are two replayable launch lists over one buffer pool.
Saved per block: GroupNorm inputs + (mean, rstd), LayerNorm inputs, q / k / v (or q, k, V^T) of every attention, the GEGLU
pre-activation.  Recomputed in the backward: attention probabilities (GEMM-formulated for the spatial layers, in-register
for the 16-frame temporal ones), everything element-wise.

  conv3x3 / (3,1,1) / 1x1 dX   the implicit-GEMM kernel on re-packed weights (flipped taps, swapped channels)
  stride-2 conv dX             zero-interleave the gradient to the input grid (``scatter2x``), then the flipped 3x3
  nearest-x2 + conv dX         flipped 3x3 at the high resolution, then a 2x2 sum-pool
  GroupNorm(+SiLU)             ``gn_bwd`` (two-part input for the skip concats; the residual branch rides in ``resid``)
  LayerNorm                    ``layernorm_bwd`` (statistics recomputed per row; residual fused)
  GEGLU                        ``geglu_bwd`` on the saved pre-activation (packed [32 value | 32 gate] column groups)
  temporal attention           ``attn_temporal_bwd`` (one wave-sized problem per pixel and head; takes d(probs) as well)
  spatial self / text cross    batched GEMMs around ``softmax_rows`` / ``softmax_bwd_rows`` with bf16 transposes; spatial self with
                               ``flash_attn_bwd``: ``attn_spatial_bwd`` (csrc/attention_bwd.hip, probabilities never in memory)

Status: the dataflow is verified on CPU against torch autograd (tests/test_unet_grad_cpu.py, emulated op backend), and the
device kernels (csrc/backward_unet.hip, train.hip, attention_bwd.hip, wgrad_tn.hip) against the emulated backend and the whole engine
against autograd on MI355X (tests/test_gpu_unet_grad.py; the same sources also run on a host SIMT simulator, tests/test_hostsim_*.py)."""
import os

import torch
import torch.nn as nn

from . import native as nt
from .native import on_tensor_device
from .bridge import TriState
from .engine import Act, Packer, UNetEngine, effective_weight_bias, is_lora_leaf, leaf_out_channels
from .engine_full import FullTrainMixin
from .engine_lora import LoraTrainMixin, _pad
from .unet3d import Downsample, ResBlock, SpatialTransformer, TemporalTransformer, TimestepEmbedSequential, Upsample


class UNetGradEngine(FullTrainMixin, LoraTrainMixin, UNetEngine):
    # spatial self-attention backward by the flash-style kernels of csrc/attention_bwd.hip (probabilities never in memory);
    # T2V_FLASH_ATTN_BWD=0 selects the GEMM-formulated one (both validated on MI355X; 342 -> 320 ms per distillation step)
    flash_attn_bwd = os.environ.get("T2V_FLASH_ATTN_BWD", "1") == "1"
    # activation checkpointing of the reference (lvdm/common.py:96-112 around ResBlock._forward, openaimodel3d.py:223-254, and
    # BasicTransformerBlock._forward, attention.py:300-311; yaml ``use_checkpoint: true``): with ``checkpoint_blocks`` every
    # residual block and every spatial / temporal transformer keeps only its INPUT in the forward and re-runs its forward inside
    # the backward (the counter-based dropout masks regenerate from (seed, site), so the recomputation is the same function).
    # Same gradients bit for bit, fewer live activations, one more block forward per block.  LoRA training and full fine-tuning
    # alike: under ``bind_full`` the leaf inputs kept for the weight gradients are rewound with the block's discarded forward and
    # saved again by its recomputation (engine_full.full_rewind).  Default off: at full size and B = 1 the full fine-tuning
    # step's activation pool is 20.2 GB on the tape (6.9 GB checkpointed) inside a 44.6 GB peak of the process, of 288
    # (profiles/r08_full_finetune_checkpoint_memory.jsonl), and checkpointing costs a fifth of the step.
    # T2V_NATIVE_CHECKPOINT=1 turns it on, =model follows the module's own ``use_checkpoint`` (what the reference's yaml
    # sets); ``UNetModel.native_checkpoint`` = True / False overrides the variable per module, and the attribute below can be set
    # on an engine at any time (a change of mode drops the recorded plans).
    _ckpt_env = os.environ.get("T2V_NATIVE_CHECKPOINT", "0")

    def _ckpt_changed(self, before):
        if self.checkpoint_blocks != before:
            self.plans.clear()                      # recorded launch lists are specific to the mode

    checkpoint_blocks = TriState(
        "True / False, or None: back to what T2V_NATIVE_CHECKPOINT says.",
        follow=lambda self: bool(getattr(self.model, "use_checkpoint", False)) if self._ckpt_env == "model" else self._ckpt_env == "1",
        changed=_ckpt_changed)

    # The B-row conditioning branch (time / fps / guidance MLPs, every ResBlock's emb_layers) on the engine instead of torch autograd:
    # recorded from the step's real inputs with the fp32 row kernels of csrc/full_grad.hip (t2v_rowlin_*), which read the master
    # parameters in place — no packs, nothing to refresh — and its backward, run from ``plan["d_emb"]``, ends the recorded backward
    # list.  Opt-in: T2V_NATIVE_COND=1 (read when the engine is built), ``UNetModel.native_conditioning`` = True / False per module,
    # or the attribute below on an engine (a change drops the recorded plans).  Full fine-tuning and LoRA training; a batch of more
    # than T2V_ROWLIN_MAX_ROWS clips (or input rows beyond the forward kernel's LDS) keeps the torch branch for that plan.
    def _cond_changed(self, before):
        if self.native_conditioning != before:
            self.plans.clear()
            if self.training_full:      # the conditioning leaves join / leave the parameters the engine differentiates
                self.bind_full(self.engine_parameters(self.model, conditioning=self.native_conditioning))

    native_conditioning = TriState("True / False, or None: back to what T2V_NATIVE_COND said when the engine was built.",
                                   follow=lambda self: self._cond_env, changed=_cond_changed)

    @property
    def _tape_refusal(self):
        return (f"{'native student' if self.trains else 'native input gradient'}: another grad-mode forward of the same shape ran "
                "before this backward (the engine keeps one outstanding tape per input shape)")

    def owns_conditioning(self, batch):
        """The engine runs the conditioning branch of a training plan with ``batch`` clips itself (then ``forward_tape`` takes no emb_all)."""
        if not (self.native_conditioning and self.trains and batch <= nt.ROWLIN_MAX_ROWS):
            return False
        return batch * self._cond_linears()[2] <= nt.ROWLIN_LDS_FLOATS     # (t2v_rowlin_fwd keeps a problem's B x K input rows in LDS)

    def __init__(self, model, ops):
        super().__init__(model, ops)
        self._cond_env = os.environ.get("T2V_NATIVE_COND", "0") == "1"
        # GroupNorm statistics of the forward from the producing GEMMs' epilogues (t2v_gemm colstat_out -> t2v_gn_stats_cs), as on
        # the inference engine; the tape keeps (mean, rstd) for the backward either way.  T2V_FUSE_GN_TRAIN=0: statistics pass
        # over the tensor (t2v_gn_stats).
        self.fuse_gn = os.environ.get("T2V_FUSE_GN_TRAIN", "1") == "1"
        # 3x3 convs on t2v_conv_halo where it takes them: the base data-gradient convs of the backward (flipped packs), and the
        # forward convs when the LoRA branch does not ride in the base leaf's epilogue (T2V_LORA_EPILOGUE=0).  Its residual add is
        # the fp32 row pass of tile80.h (one rounding), so the training numerics are those of t2v_gemm.  T2V_CONV_HALO_TRAIN=0: off.
        self.conv_halo = os.environ.get("T2V_CONV_HALO_TRAIN", "1") == "1"

    # ---- public: forward with tape, then backward ----------------------------------------------------------------
    def _active_dropouts(self):
        """Number of active Dropout(p > 0) modules; in LoRA training they must all be ones the engine (or torch's conditioning
        branch) applies: the LoRA branches' and the temporal conv blocks' (train-mode student, train_t2v_turbo_v1_lora.py:641)."""
        from .nn_util import walk_modules
        mods = walk_modules(self.model)  # (one cheap walk per call: order does not matter here)
        active = [mod for mod in mods if isinstance(mod, nn.Dropout) and mod.p > 0 and mod.training]
        if active and self.trains:
            from .unet3d import TemporalConvBlock
            known = {id(mod.dropout) for mod in mods if is_lora_leaf(mod)}
            for blk in mods:
                if isinstance(blk, TemporalConvBlock):
                    known.update(id(l) for st in (blk.conv1, blk.conv2, blk.conv3, blk.conv4) for l in st if isinstance(l, nn.Dropout))
            other = [mod for mod in active if id(mod) not in known]
            if other:
                raise RuntimeError(f"native training: {len(other)} active Dropout module(s) the engine does not apply")
        return len(active)

    @on_tensor_device
    def forward_tape(self, x, timesteps, context, fps=16, timestep_cond=None, motion_cond=None, emb_all=None, seed=None):
        """``emb_all`` (LoRA training only): the conditioning branch's output [B, sum of ResBlock widths] fp32, computed by
        the caller in torch (``conditioning_torch``) so that autograd owns that branch's 27 tiny leaves."""
        m = self.model
        assert x.dim() == 5 and context is not None
        owns = self.owns_conditioning(x.shape[0])
        assert (emb_all is not None) == (self.trains and not owns), \
            "emb_all is given exactly when LoRA tensors / the base weights are bound for training and the engine does not own the conditioning branch"
        # (full fine-tuning: every parameter moves every step — the packs are re-filled in place instead of dropping the plans)
        if not self.training_full:
            self._check_weights(m, self.lora_ids if self.training_lora else ())
        dropping = self._active_dropouts()
        if dropping and not self.trains:
            raise RuntimeError("native UNet gradient path: a Dropout(p>0) is in training mode; call .eval() first")
        key = ("grad", dropping, tuple(x.shape), x.dtype, tuple(context.shape), context.dtype, isinstance(fps, int),
               None if timestep_cond is None else tuple(timestep_cond.shape),
               None if motion_cond is None else tuple(motion_cond.shape), x.device, self.training_lora, self.training_full)
        plan = self.plans.get(key)
        if plan is not None and owns and plan.get("cond_ptrs") != self._cond_ptrs():
            del self.plans[key]                     # a conditioning parameter was re-homed: its recorded launches read the old storage
            plan = None
        if dropping:  # one seed per forward; the backward regenerates the same masks from it
            self._seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        if plan is None:
            if self.training_lora:
                # the LoRA operand / gradient arenas (engine_lora._lora_begin) are per engine, not per plan: a new input signature
                # replaces the recorded plan instead of leaving one behind whose launches point into freed arenas
                self.plans.clear()
            plan = self._adopt(key, self._record_grad(x, timesteps, context, fps, timestep_cond, motion_cond, emb_all))
        else:
            st = plan["static"]
            self._load_inputs(st, x, timesteps, context, fps, timestep_cond, motion_cond)
            if self.trains:
                if emb_all is not None:
                    st["emb_all"].copy_(emb_all.detach())
                if self.training_lora:
                    self.refresh_lora_packs()
                else:
                    self.full_activate(plan)      # this plan's Packer (not the one recorded last), then ITS packs up to date
                    self.full_refresh_packs(plan)
            if dropping:
                st["seed"].fill_(self._seed)
            if "seed" in st:
                self.seed_t = st["seed"]
            self._replay(plan, "rec")
        self._end_tape(plan)
        self._publish_probs(plan)
        return plan["out"].clone()

    def backward(self, dout=None, dprobs=None, flat_grad=None, accumulate=True, grad_sync=None, token=None):
        """d(loss)/dx for the ``forward_tape`` of ``token`` (``tape_token`` right after it; default: the most recent one).
        ``dout``: gradient w.r.t. the output (or None = 0);
        ``dprobs``: {attention module: gradient w.r.t. its ``attention_probs``} for any of the recorded layers.
        LoRA training: the weight gradients land in ``flat_grad`` (fp32, ``bind_lora`` order; added to what is there
        when ``accumulate``) and ``self.d_emb_all`` holds d(loss)/d(emb_all) for the caller's torch branch.
        ``grad_sync``: the ``dist.FlatGradSync`` that owns ``flat_grad``.  In a multi-rank job the engine then all-reduces its
        gradient arena in segments WHILE the backward runs (engine_lora: "gradient exchange overlapped with the backward") and
        hands over already averaged gradients; ``grad_sync.all_reduce_mean()`` afterwards only exchanges the conditioning
        branch's tensors.  T2V_ASYNC_ALLREDUCE=0 keeps the single blocking all-reduce after the backward.  Under ``use_graph``
        the backward list is captured as one hipGraph per run of launches between two markers."""
        plan = (token or self.tape_token)[0]
        if plan["out"].is_cuda and plan["out"].device.index != torch.cuda.current_device():
            with torch.cuda.device(plan["out"].device):
                return self.backward(dout, dprobs, flat_grad, accumulate, grad_sync, token)
        self._claim_tape("UNet gradient", token)
        if self.training_full:
            self.full_activate(plan)              # (another signature's forward may have run since this plan's)
        st = plan["static"]
        st["dout"].zero_() if dout is None else st["dout"].copy_(dout)
        dprobs = dprobs or {}
        known = {id(a) for a, _ in plan["probs"]}
        for a in dprobs:
            if id(a) not in known:
                raise KeyError("dprobs given for a layer that does not record attention_probs")
        for attn, _ in plan["probs"]:
            buf = plan["dprobs"][id(attn)]
            g = dprobs.get(attn)
            buf.zero_() if g is None else buf.copy_(g)
        world = self._overlap_world(grad_sync, flat_grad)
        self._overlap, self._handles = (grad_sync if world else None), []
        try:
            self._replay(plan, "rec_bwd")
        finally:
            self._overlap = None
        if self.trains:
            self.d_emb_all = plan["d_emb"]
        if self.training_lora:
            if flat_grad is not None:
                assert flat_grad.dtype == torch.float32 and flat_grad.numel() == self.lora_numel and flat_grad.is_contiguous()
                if world:
                    assert self._handles, "overlapped gradient exchange: the backward list carries no segment markers"
                    for h in self._handles:
                        h.wait()
                    self.lora_grads_into(flat_grad, accumulate, alpha=1.0 / world)
                    grad_sync.mark_engine_reduced(self.conditioning_index())
                else:
                    self.lora_grads_into(flat_grad, accumulate)
                    if grad_sync is not None and hasattr(grad_sync, "note_local_grads"):
                        grad_sync.note_local_grads()   # un-averaged: the next all_reduce_mean covers the whole buffer
        return plan["dx"].clone()

    def _overlap_world(self, grad_sync, flat_grad):
        """World size when this backward should exchange its gradient arena itself, else 0."""
        if grad_sync is None or flat_grad is None or not self.training_lora or os.environ.get("T2V_ASYNC_ALLREDUCE", "1") == "0":
            return 0
        import torch.distributed as dist
        if not dist.is_initialized() or grad_sync.flat.data_ptr() != flat_grad.data_ptr():
            return 0
        world = dist.get_world_size()
        if world == 1 and not getattr(grad_sync, "force", False):
            return 0
        return world

    # ---- recording ------------------------------------------------------------------------------------------------
    def _record_grad(self, x, timesteps, context, fps, timestep_cond, motion_cond, emb_all=None):
        m = self.model
        self._begin(x.device)
        B, Cin, F, H, W = x.shape
        self.B, self.F = B, F
        st = self._static_inputs(x, timesteps, context, fps, timestep_cond, motion_cond)
        out = torch.empty(B, m.out_channels, F, H, W, dtype=x.dtype, device=x.device)
        st["dout"] = torch.zeros_like(out)
        plan = {"static": st, "out": out, "dx": torch.empty_like(st["x"]), "probs": [], "dprobs": {}}
        if self.training_lora:
            # frozen base weights are packed as they are; the LoRA branch runs as its own GEMMs on per-step operand packs
            self.pk = Packer(self.adt, x.device, merge_lora=False)
            self._cond_owned = emb_all is None      # (the conditioning leaves' gradient slots are part of the arena then)
            self._lora_begin()
        if self.training_full:
            # plain leaves on packs of the current weights (re-filled in place per step: Packer.refresh); one fp32 gradient per parameter
            self.pk = Packer(self.adt, x.device)
            plan["fgrads"] = {}
            from .engine import params_fingerprint
            plan["full_fp"] = params_fingerprint(m)   # the weights this plan's packs are made from, while it is recorded
        if self.trains:
            if emb_all is not None:
                st["emb_all"] = emb_all.detach().to(x.device, torch.float32).clone().contiguous()
                plan["d_emb"] = torch.zeros_like(st["emb_all"])
            else:   # the engine owns the conditioning branch: emb_all is made by the recorded forward, d_emb consumed by the recorded backward
                plan["d_emb"] = torch.zeros(B, self._emb_table()[1], dtype=torch.float32, device=x.device)
                plan["cond_ptrs"] = self._cond_ptrs()
            st["seed"] = torch.full((1,), getattr(self, "_seed", 0), dtype=torch.int64, device=x.device)
            self.seed_t = st["seed"]
        plan["geom"] = (B, F)
        self.plan = plan
        self.tape, self.refs = [], {}
        self._fsaved = {}

        def fwd():
            self.tape.clear()
            self.refs.clear()
            self._fsaved.clear()
            self.drop_sites = []
            plan["probs"].clear()
            self._forward_tape(st, out)

        def bwd():
            self._backward_tape(st["dout"], plan["dx"])

        return self._record_lists(plan, ("rec", fwd), ("rec_bwd", bwd))

    # ---- saved-activation bookkeeping: a tensor may be kept by several backward closures (skip connections) ----------
    def hold(self, *ts):
        for t in ts:
            if t is not None:
                self.refs[t.data_ptr()] = self.refs.get(t.data_ptr(), 0) + 1

    def drop(self, *ts):
        for t in ts:
            if t is None:
                continue
            k = t.data_ptr()
            n = self.refs.get(k, 0) - 1
            if n > 0:
                self.refs[k] = n
            else:
                self.refs.pop(k, None)
                self.pool.put(t)

    # ---- helpers ------------------------------------------------------------------------------------------------------
    def gn_t(self, x, norm, units, rows, silu):
        """GroupNorm(+SiLU) of an Act keeping (mean, rstd); the caller keeps x for the backward."""
        ops = self.ops
        G = norm.num_groups
        stats = self.buf(units, G * 2, torch.float32)
        if self.fuse_gn and all(c is not None for c in x.cs) and rows % 32 == 0:
            ws = self.buf(1, max(ops.group_norm_cs_ws_floats(units, rows, G), 1), torch.float32)
            ops.gn_stats_cs(x.cs[0], x.cs[1] if len(x.cs) > 1 else None, x.parts[0].shape[1],
                            x.parts[1].shape[1] if len(x.parts) > 1 else 0, units, rows, norm.eps, ws, stats, G)
        else:
            ws = self.buf(1, max(ops.gn_ws_floats(units, rows, G), 1), torch.float32)
            ops.gn_stats(x.parts[0], x.p1, units, rows, norm.eps, ws, stats, G)
        out = self.buf(x.M, x.C)
        ops.gn_apply(x.parts[0], x.p1, units, rows, stats, self.pk.f32(norm.weight), self.pk.f32(norm.bias), silu, out, G)
        self.pool.put(ws)
        return out, stats

    def gn_b(self, x, norm, units, rows, silu, stats, dy, resid=None):
        """-> dx [M, C] (one buffer even when x is a virtual concat: the consumer takes column slices)."""
        ops = self.ops
        G = norm.num_groups
        if self.training_full:
            self.full_norm_grads(norm, x, dy, kind=0, silu=silu, rows_per_unit=rows, stats=stats)
        ws = self.buf(1, max(ops.gn_bwd_ws_floats(units, rows, G), 1), torch.float32)
        dx = self.buf(x.M, x.C)
        ops.gn_bwd(x.parts[0], units, rows, stats, self.pk.f32(norm.weight), self.pk.f32(norm.bias), silu, dy, resid, ws, dx, G,
                   x1=x.p1)
        self.pool.put(ws)
        return dx

    def drop_site(self, drops, kind, meta=None):
        """(p, site id) of an active dropout (None if inactive).  ``drops``: the nn.Dropout module(s) this site stands for
        (one per leaf of a LoRA group); kind / meta describe the row order for tests that replay the masks in torch."""
        ps = {(d.p if d.training else 0.0) for d in drops}
        assert len(ps) == 1, "leaves of one LoRA group must share the dropout probability"
        p = ps.pop()
        if p <= 0:
            return None
        assert self.trains, "dropout is only applied on the training paths"
        self.drop_sites.append((drops, kind, meta))
        return float(p), len(self.drop_sites) - 1

    def rel(self, *ts):
        """Forward-side release of an intermediate: kept alive while a backward closure / LoRA group still holds it."""
        for t in ts:
            if t is not None and self.refs.get(t.data_ptr(), 0) == 0:
                self.pool.put(t)

    # ---- leaves: forward with the LoRA branch (training), backward with the LoRA weight gradients -----------------------
    def linear(self, a, mod, *, residual=None, act=nt.ACT_NONE, out_dtype=None, w=None, bias="auto", N=None, lora=None, perm=None,
               conv_geom=None, want_cs=False):
        """``a``: tensor or two-part Act.  ``lora``: the injected leaves whose row-concatenated weights ``w`` holds (default:
        [mod]); ``perm``: packed output row j = original row perm[j] (GEGLU packing)."""
        x = a if isinstance(a, Act) else Act(a, 0, 0, 0)
        mods = lora if lora is not None else ([mod] if mod is not None else None)
        zf = grp = None
        if self.training_full and mods:
            self.full_save(mods, x, perm=perm)
        if self.training_lora and mods and all(is_lora_leaf(mm) for mm in mods):
            assert act == nt.ACT_NONE
            meta = (self.B, self.F, x.M // (self.B * self.F)) if self.row_kind == "temporal" else (self.B, self.F, self.ctx_len)
            if conv_geom is not None:  # a 1x1 conv run as a linear layer: torch sees (n, C, h, w)
                meta = conv_geom
            grp = self.lgroup(mods, nt.GEMM_LINEAR, perm)
            self.lora_t(grp, x, x.M, kind_meta=meta, kind="conv" if conv_geom is not None else None)
        w = self.pk.mat(mod) if w is None else w
        bias = self.pk.bias(mod) if isinstance(bias, str) else bias
        N = w.shape[0] if N is None else N
        out = self.buf(x.M, N // 2 if act == nt.ACT_GEGLU else N, out_dtype)
        kw = dict(M=x.M, N=N, a1=x.p1, bias=bias, residual=residual, act=act)
        if grp is not None:
            # the LoRA branch: inside this launch's epilogue where the launch can carry it, else as up-projection launches whose
            # sum z becomes this launch's residual operand
            extra = self.lora_epilogue_args(grp) if N == grp.ntot else None
            if (extra is not None and self.lora_split_aware and hasattr(self.ops, "gemm_plan")
                    and self.ops.gemm_plan(x.parts[0], w, out, **kw)[1] > 1):
                extra = None   # (the plain launch splits K: the epilogue form, one split, would lose more than it saves)
            if extra is not None and self.ops.gemm_fuse_supported(x.parts[0], w, out, **kw, **extra):
                kw.update(extra)
            else:
                zf, kw["residual"] = self.lora_up(grp, x.M, residual)
        self.last_cs = self._colstat_for(x.parts[0], w, out, **kw) if want_cs else None   # (for the GroupNorm of the next block)
        if self.last_cs is not None:
            kw["colstat"] = self.last_cs
        self.ops.gemm(x.parts[0], w, out, **kw)
        if zf is not None:
            self.pool.put(zf)
        return out

    def conv(self, x, mod, mode, *, frames=0, rowvec=None, rowvec_div=0, residual=None, out_dtype=None, w=None, bias="auto", frozen_pack=False):
        zf = extra = None
        if w is None and self.training_full and mod is not None:
            self.full_save([mod], x, frames=frames)
        if w is None and self.training_lora and is_lora_leaf(mod):
            if mode == nt.GEMM_CONV3X3_S2:
                ho, wo = (x.h - 1) // 2 + 1, (x.w - 1) // 2 + 1
            elif mode == nt.GEMM_CONV3X3_UP2:
                ho, wo = 2 * x.h, 2 * x.w
            else:
                ho, wo = x.h, x.w
            grp = self.lgroup([mod], mode)
            self.lora_t(grp, x, x.n_img * ho * wo, frames, kind_meta=(x.n_img, ho, wo))
            extra = self.lora_epilogue_args(grp) if out_dtype in (None, self.adt) else None
            if extra is None:
                zf, residual = self.lora_up(grp, x.n_img * ho * wo, residual)
        y = super().conv(x, mod, mode, frames=frames, rowvec=rowvec, rowvec_div=rowvec_div, residual=residual,
                         out_dtype=out_dtype, w=w, bias=bias, want_cs=w is None,   # (data-gradient convs pass their own pack: no statistics)
                         frozen_pack=frozen_pack, extra=extra, fallback=None if extra is None else (lambda: self.lora_up(grp, x.n_img * ho * wo, residual)))
        if zf is not None:
            self.pool.put(zf)
        return y

    def lin_b(self, dy, w_t, residual=None, lora=None, need_dx=True, colsum=None):
        """dx = dy @ W for a [K, N]-transposed pack w_t (rows = input features); ``lora``: the leaves behind w_t — in
        training their weight gradients are taken here and their branch's data gradient joins dx."""
        if self.training_full and lora:
            self.full_linear_grads(lora, dy)
        grp = self.saved_group(lora, nt.GEMM_LINEAR)
        dl = None
        if grp is not None:
            g = self.lora_wgrad(grp, dy, colsum)
            if need_dx:
                dl = self.buf(dy.shape[0], grp.ce)
                self.ops.gemm(g, grp.Db, dl, M=dy.shape[0], N=grp.ce, residual=residual)
                residual = dl
            self.lora_wgrad_down(grp, g)
            self.pool.put(g)
        if not need_dx:
            return None
        out = self.buf(dy.shape[0], w_t.shape[0])
        self.ops.gemm(dy, w_t, out, M=dy.shape[0], N=w_t.shape[0], residual=residual)
        if dl is not None:
            self.pool.put(dl)
        return out

    def conv_b(self, dy, mod, mode, in_geom, frames=0, colsum=None, out_dtype=None, dy_pad=None):
        """Data gradient of a conv leaf: dy is an Act on the leaf's OUTPUT grid, the result an Act on its input grid
        ``in_geom`` = (n_img, h, w).  The adjoint of every gather mode is the 3x3 / (3,1,1) kernel itself on re-packed
        weights (stride 2: zero-interleaved dy; nearest-x2: 2x2 sum-pool of the result).  In training the leaf's LoRA weight
        gradients are taken here as well.  ``dy_pad``: dy with its columns zero-padded to 64 (narrow exit conv)."""
        ops = self.ops
        n, h, w = in_geom
        m_in = n * h * w
        base = self.pk.tconv_dgrad(mod) if mode == nt.GEMM_TCONV3 else self.pk.conv_dgrad(mod)
        inner_mode = nt.GEMM_TCONV3 if mode == nt.GEMM_TCONV3 else nt.GEMM_CONV3X3

        def run(src, wpack, residual=None, odt=None, pool=True, frozen=False):
            """adjoint gather of ``src`` (a tensor on the output grid) against an [N, taps*c] pack (``frozen``: of frozen weights)"""
            if mode == nt.GEMM_CONV3X3_S2:
                z = self.buf(m_in, src.shape[1])
                ops.scatter2x(src, n, dy.h, dy.w, h, w, z)
                y = self.conv(Act(z, n, h, w), None, inner_mode, w=wpack, bias=None, residual=residual, out_dtype=odt)
                self.pool.put(z)
                return y.t
            if mode == nt.GEMM_CONV3X3_UP2:
                hi = self.conv(Act(src, n, 2 * h, 2 * w), None, inner_mode, w=wpack, bias=None, residual=residual)
                if not pool:
                    return hi.t
                lo = self.buf(m_in, wpack.shape[0])
                ops.sumpool2x2(hi.t, n, h, w, lo)
                self.pool.put(hi.t)
                return lo
            return self.conv(Act(src, n, h, w), None, inner_mode, frames=frames, w=wpack, bias=None, residual=residual,
                             out_dtype=odt, frozen_pack=frozen).t

        if self.training_full and dy_pad is None:
            self.full_conv_grads(mod, mode, dy.t)
        grp = self.saved_group([mod], mode)
        dl = None
        if grp is not None:
            g = self.lora_wgrad(grp, dy.t if dy_pad is None else dy_pad, colsum)
            if mode == nt.GEMM_CONV3X3_UP2:
                dl = run(g, grp.Db, pool=False)                  # LoRA branch's data gradient, high-res: pooled with the base
                G = run(g, self.sel_pack(grp.taps, grp.rp))      # rank-r gradient gathered to the input grid, per tap
                self.pool.put(g)
                self.lora_wgrad_down(grp, G)
                self.pool.put(G)
            else:  # both from one launch: columns [0, ce) = data gradient, [ce, ce + taps*rp) = gathered rank-r gradient
                dl = run(g, grp.DbSel)
                self.pool.put(g)
                self.lora_wgrad_down(grp, dl[:, grp.ce:])
        cin = base.shape[0]
        res = None if dl is None else dl[:, :cin]
        dx = run(dy.t, base, residual=res, odt=out_dtype, frozen=True)
        if dl is not None:
            self.pool.put(dl)
        return Act(dx, n, h, w)

    def add(self, a, b):
        out = self.buf(a.shape[0], a.shape[1])
        self.ops.add(a, b, out)
        return out

    # ---- forward with tape ------------------------------------------------------------------------------------------
    def _forward_tape(self, st, out):
        m, ops, pk = self.model, self.ops, self.pk
        B, F = self.B, self.F
        x = st["x"]
        _, Cin, _, H, W = x.shape
        self._conditioning(st)
        xt = self.buf(B * F * H * W, Cin)
        ops.ncfhw_to_tokens(x, xt)
        conv_in = m.input_blocks[0][0]
        c_first = leaf_out_channels(conv_in)
        h0 = self.buf(B * F * H * W, c_first)
        ops.conv_small(xt, B * F, H, W, pk.small_conv(conv_in), pk.bias(conv_in), h0)
        self.pool.put(xt)
        if self.training_full:   # the entry conv's weight gradient contracts against the latent rows, zero-padded to one 16-byte chunk
            x8 = self.buf(B * F * H * W, 8)
            ops.fill_zero(x8)
            ops.ncfhw_to_tokens(x, x8)
            self.full_save([conv_in], Act(x8, B * F, H, W), frames=0)
        if self.training_lora and is_lora_leaf(conv_in):
            # LoRA branch of the entry conv: the 4-channel latent zero-padded to one 64-channel K slab of the implicit GEMM
            x64 = self.buf(B * F * H * W, 64)
            ops.fill_zero(x64)
            ops.ncfhw_to_tokens(x, x64)
            zf, z = self.lora_z(self.lgroup([conv_in], nt.GEMM_CONV3X3), Act(x64, B * F, H, W), B * F * H * W, kind_meta=(B * F, H, W))
            h0b = self.add(h0, z)
            self.pool.put(h0, zf)
            h0 = h0b
        h = Act(h0, B * F, H, W)
        hs = []
        for i, block in enumerate(m.input_blocks):
            if i > 0:
                h = self.run_sequential_t(block, h)
            if i == 0 and m.addition_attention:
                h = self.run_sequential_t(m.init_attn, h)
            hs.append(h)
            # h is a skip connection too: in the backward, the gradient the matching output block left for it is added
            # here, i.e. after everything downstream of h on the main chain has been walked back
            self.tape.append(("join", None))
        h = self.run_sequential_t(m.middle_block, h)
        for block in m.output_blocks:
            skip = hs.pop()
            # (reverse order!) once the block below is walked back, its input gradient [M, c(h) + c(skip)] splits in two
            self.tape.append(("split", h.C))
            h = self.run_sequential_t(block, Act([h.t, skip.t], h.n_img, h.h, h.w, cs=[h.cs[0], skip.cs[0]]))
        xin = h
        self.hold(xin.t)
        tt, st_out = self.gn_t(xin, m.out[0], B * F, H * W, True)
        y = self.conv(Act(tt, h.n_img, h.h, h.w), m.out[2], nt.GEMM_CONV3X3, out_dtype=torch.float32)
        self.rel(tt)
        ops.tokens_to_ncfhw(y.t, out)
        self.pool.put(y.t)
        n_img = B * F

        cpad = 4 if m.out_channels <= 4 else 8
        assert m.out_channels <= 8, "the direct small-channel conv handles up to 8 gradient channels"

        def exit_bwd(dout):
            # conv_out data gradient (4 -> 320 channels) on the direct small-channel conv, like the VAE decoder's exit
            d4 = self.buf(n_img * H * W, cpad)
            if cpad != m.out_channels:
                ops.fill_zero(d4)
            ops.ncfhw_to_tokens(dout, d4)
            dt = self.buf(n_img * H * W, xin.C)
            ops.conv_small(d4, n_img, H, W, pk.small_conv_dgrad(m.out[2], cin_pad=cpad), None, dt)
            self.pool.put(d4)
            if self.training_full:   # the exit conv's own weight / bias gradient: dy zero-padded to one 16-byte chunk of columns
                d8 = self.buf(n_img * H * W, 8)
                ops.fill_zero(d8)
                ops.ncfhw_to_tokens(dout, d8)
                self.full_conv_grads(m.out[2], nt.GEMM_CONV3X3, d8)
                self.pool.put(d8)
            grp = self.saved_group([m.out[2]], nt.GEMM_CONV3X3)
            if grp is not None:  # LoRA of the exit conv: dy zero-padded to 64 columns (K of  g = s dy U)
                d64 = self.buf(n_img * H * W, 64)
                ops.fill_zero(d64)
                ops.ncfhw_to_tokens(dout, d64)
                g = self.lora_wgrad(grp, d64)
                self.pool.put(d64)
                dl = self.conv(Act(g, n_img, H, W), None, nt.GEMM_CONV3X3, w=grp.DbSel, bias=None).t
                self.pool.put(g)
                self.lora_wgrad_down(grp, dl[:, grp.ce:])
                dt2 = self.add(dt, dl[:, :grp.ce])
                self.pool.put(dt, dl)
                dt = dt2
            dx = self.gn_b(xin, m.out[0], n_img, H * W, True, st_out, dt)
            self.pool.put(dt, st_out)
            self.drop(xin.t)
            return Act(dx, n_img, H, W)

        def entry_bwd(dy, dx_out):
            # conv_in data gradient (320 -> 4 channels): a narrow-N implicit GEMM like the forward's conv_out, fp32 out
            d = self.conv_b(dy, conv_in, nt.GEMM_CONV3X3, (n_img, H, W), out_dtype=torch.float32)
            self._free_view(dy.t)
            ops.tokens_to_ncfhw(d.t, dx_out)
            self.pool.put(d.t)

        self.exit_bwd, self.entry_bwd = exit_bwd, entry_bwd

    def _conditioning(self, st):
        """Embedding / context branch of UNetEngine._forward (no dependence on the latents: no tape)."""
        self._context(st)
        self._ctx_f = None
        if self.trains and "emb_all" not in st:
            self._conditioning_t(st)
        elif self.trains:  # the M = B-row branch belongs to torch autograd (engine_lora.py / engine_full.py); its result is an input
            width = self._emb_table()[1]
            assert st["emb_all"].shape == (self.B, width)
            self.emb_all = st["emb_all"]
        else:
            self._embedding(st)

    # ---- the conditioning branch on the engine (``native_conditioning``) ---------------------------------------------------------------
    def _cond_linears(self):
        """The Linear leaves of the conditioning branch (injected ones as their wrapper), found once per engine."""
        got = self.__dict__.get("_cond_lin")
        if got is None or got[0] is not self.full_params or got[1] is not self.lora_params:
            m = self.model
            mods = [getattr(m, n, None) for n in ("time_cond_proj", "motion_cond_proj", "combine_proj")]
            mods += [m.time_embed[0], m.time_embed[2]] + ([m.fps_embedding[0], m.fps_embedding[2]] if m.fps_cond else [])
            mods += [rb.emb_layers[1] for rb in self._emb_table()[0]]
            mods = [mod for mod in mods if mod is not None]
            params = [p for mod in mods for sub in mod.modules() for p in sub._parameters.values() if p is not None]
            kmax = max((mod.linear if is_lora_leaf(mod) else mod).weight.shape[1] for mod in mods)
            got = self._cond_lin = (self.full_params, self.lora_params, mods, params, kmax)
        return got[2:]

    def _cond_ptrs(self):
        return tuple(p.data_ptr() for p in self._cond_linears()[1])

    def cond_lora_leaves(self):
        return [mod for mod in self._cond_linears()[0] if is_lora_leaf(mod)]

    def _conditioning_t(self, st):
        """UNetEngine._embedding in fp32 on the live parameters (t2v_rowlin_fwd), from the static inputs ts / fps / tc / mc.  Keeps the B-row
        activations the backward needs in the plan (a few kilobytes, outside the pool: a checkpointed block never discards them).  An
        injected leaf runs its LoRA branch as the same entry three times — t = f(x) D^T, u = s t U^T (+ res), [u = dropout(u) (+ res),]
        y = f(x) W^T + b + u (utils/lora.py:45-50) — and gets its gradient slots at the bottom of the arena E."""
        m, ops = self.model, self.ops
        B, mc, dev = self.B, m.model_channels, st["x"].device
        blocks, width = self._emb_table()
        c = {"keep": []}

        def new(cols):
            t = torch.empty(B, cols, dtype=torch.float32, device=dev)
            c["keep"].append(t)
            return t

        def f32(t):
            if t.dtype == torch.float32:
                return t
            out = new(t.shape[1])
            ops.cast(t, out)
            return out

        def lin_table(items, per_frame=False):
            """items: (x, module, y or None, silu, res) of leaves that do not depend on one another -> their leaf records (with "y")."""
            downs, ups, drops, bases, leaves = [], [], [], [], []
            # how torch orders the rows a leaf's dropout sees (tests replay the masks): the MLPs run on B rows; the composite path repeats emb
            # per frame before emb_layers, and one mask per CLIP, as conditioning_emb_all draws it, is every frame's — the "ctx" order, L = 1
            kind = ("ctx", (B, self.F, 1)) if per_frame else ("rows", None)
            for x, mod, y, silu, res in items:
                base = mod.linear if is_lora_leaf(mod) else mod
                y = new(base.weight.shape[0]) if y is None else y
                leaf = dict(mod=mod, x=x, silu=silu, y=y)
                if is_lora_leaf(mod):
                    assert self.training_lora, "native full fine-tuning of a LoRA-injected network (train the LoRA tensors, or merge them first)"
                    if not isinstance(mod.selector, nn.Identity):
                        raise NotImplementedError("native LoRA training: a selector is set on an injected leaf")
                    D, U = mod.lora_down.weight, mod.lora_up.weight
                    if id(D) not in self.lora_off or id(U) not in self.lora_off:
                        raise ValueError("a LoRA leaf's tensors are not in the list given to bind_lora")
                    n_out, r = U.shape
                    slots = self._cond_slots.get(id(mod))     # (per arena, like the token-row groups: a closure backend re-runs this forward)
                    if slots is None:
                        slots = []
                        for w, (rows, cols) in ((U, (n_out, r)), (D, (r, D.shape[1]))):   # gradient slots, in the parameter's own layout
                            off, e = self._e_alloc(rows, cols)
                            o = self.lora_off[id(w)]
                            self.g_idx[o:o + w.numel()] = (off + torch.arange(w.numel())).to(dev, torch.int32)
                            slots.append(e)
                        self._cond_slots[id(mod)] = slots
                    leaf["EU"], leaf["ED"] = slots
                    site = self.drop_site([mod.dropout], *kind)
                    t, u = new(r), new(n_out)
                    downs.append(dict(x=x, w=D, y=t, silu=silu))
                    ups.append(dict(x=t, w=U, y=u, alpha=float(mod.scale), res=None if site else res))
                    if site:
                        if n_out % 2:
                            raise NotImplementedError("native conditioning: dropout on a LoRA branch with an odd number of features")
                        drops.append((u, res, n_out, site))
                    leaf.update(t=t, site=site, scale=float(mod.scale))
                    res = u
                bases.append(dict(x=x, w=base.weight, bias=base.bias, y=y, silu=silu, res=res))
                leaves.append(leaf)
            for table in (downs, ups):
                if table:
                    ops.rowlin_fwd(table, B)
            for u, res, n_out, site in drops:
                ops.dropout(u, res, u, n_out, site[0], self.seed_t, site[1])
            ops.rowlin_fwd(bases, B)
            return leaves

        def lin(x, mod, y=None, silu=False, res=None):
            leaf = lin_table([(x, mod, y, silu, res)])[0]
            c[id(mod)] = leaf
            return leaf["y"]

        c["t_emb"] = new(mc)
        ops.timestep_embedding_f32(st["ts"], mc, False, c["t_emb"])
        c["emb_in"] = c["t_emb"]
        if "tc" in st:
            c["tc"] = f32(st["tc"])
            if "mc" in st:   # combine_proj(cat[time_cond_proj(tc), motion_cond_proj(mc)]) + t_emb: the two projections write the halves of one buffer
                c["mc"] = f32(st["mc"])
                c["cat"] = new(2 * mc)
                lin(c["tc"], m.time_cond_proj, y=c["cat"][:, :mc])
                lin(c["mc"], m.motion_cond_proj, y=c["cat"][:, mc:])
                c["emb_in"] = lin(c["cat"], m.combine_proj, res=c["t_emb"])
            else:
                c["emb_in"] = lin(c["tc"], m.time_cond_proj, res=c["t_emb"])
        c["e1"] = lin(c["emb_in"], m.time_embed[0])
        c["emb"] = lin(c["e1"], m.time_embed[2], silu=True)
        if m.fps_cond:
            c["f_emb"] = new(mc)
            ops.timestep_embedding_f32(st["fps"], mc, False, c["f_emb"])
            c["f1"] = lin(c["f_emb"], m.fps_embedding[0])
            c["emb"] = lin(c["f1"], m.fps_embedding[2], silu=True, res=c["emb"])
        # every ResBlock's emb_layers (SiLU -> Linear) as ONE table: problem i writes its column slice of emb_all
        self.emb_all = new(width)     # (``self.emb_all`` is the NEXT recorded plan's soon: this plan keeps its own)
        c["layers"] = lin_table([(c["emb"], rb.emb_layers[1], self.emb_all[:, self.emb_off[id(rb)]:self.emb_off[id(rb)] + rb.out_channels], True, None)
                                 for rb in blocks], per_frame=True)
        c["blocks"] = blocks
        self.plan["cond"] = c

    def _conditioning_b(self):
        """Backward of ``_conditioning_t`` from ``plan["d_emb"]`` (the per-clip column sums the ResBlock backwards left).  Full fine-tuning:
        every weight and bias gradient by t2v_rowlin_wgrad straight into its slot of the gradient arena.  LoRA training: dU = s dy'^T t and
        dD = s g^T f(x) (dy' = dy through the forward's mask, g = dy' U) into the leaf's slots of the arena E, from where the one gather of
        ``lora_grads_into`` carries them to the flat gradient with every other LoRA tensor's.  Data gradients by t2v_rowlin_bwd_data: the
        frozen base weight and the down-projection of a leaf are two problems that share its dx."""
        m, ops, c, B = self.model, self.ops, self.plan["cond"], self.B
        d_all = self.plan["d_emb"]
        dev = d_all.device

        def new(cols):
            t = torch.empty(B, cols, dtype=torch.float32, device=dev)
            c["keep"].append(t)     # (recorded launches hold raw pointers: the plan keeps the tensors alive)
            return t

        def bwd_data(table):
            ws = torch.empty(max(ops.rowlin_ws_floats(table, B), 1), dtype=torch.float32, device=dev)
            c["keep"].append(ws)
            ops.rowlin_bwd_data(table, B, ws)

        def back(items, pre=None, need_dx=True):
            """items: (leaf record, dy) of leaves reading the same input -> d(input) = g(pre) * sum of their data gradients (or None)."""
            if self.training_full:
                ops.rowlin_wgrad([dict(x=lf["x"], y=dy, silu=lf["silu"], dw=self.fgrad(lf["mod"].weight),
                                       db=None if lf["mod"].bias is None else self.fgrad(lf["mod"].bias)) for lf, dy in items], B)
            probs, ups, gs, downs = [], [], [], []
            for lf, dy in items:
                mod = lf["mod"]
                if not is_lora_leaf(mod):
                    probs.append(dict(w=mod.weight, y=dy))
                    continue
                probs.append(dict(w=mod.linear.weight, y=dy))
                dym = dy
                if lf["site"]:   # the LoRA branch saw dy through the forward's mask; the base leaf sees dy itself
                    dym = new(dy.shape[1])
                    ops.dropout(dy, None, dym, dy.shape[1], lf["site"][0], self.seed_t, lf["site"][1])
                g = new(lf["t"].shape[1])
                ups.append(dict(x=lf["t"], y=dym, dw=lf["EU"], alpha=lf["scale"]))
                gs.append(dict(w=mod.lora_up.weight, y=dym, dx=g))
                downs.append(dict(x=lf["x"], silu=lf["silu"], y=g, dw=lf["ED"], alpha=lf["scale"]))
                probs.append(dict(w=mod.lora_down.weight, y=g, alpha=lf["scale"]))
            if ups:
                ops.rowlin_wgrad(ups, B)
                bwd_data(gs)
                ops.rowlin_wgrad(downs, B)
            if not need_dx:
                return None
            dx = new(probs[0]["w"].shape[1])
            for q in probs:
                q.update(dx=dx, x=pre, silu=pre is not None)
            bwd_data(probs)
            return dx

        layers = [(lf, d_all[:, self.emb_off[id(rb)]:self.emb_off[id(rb)] + rb.out_channels]) for lf, rb in zip(c["layers"], c["blocks"])]
        d_emb = back(layers, pre=c["emb"])                          # d(emb): also d(time_embed out) and d(fps_embedding out)
        if m.fps_cond:
            d_f1 = back([(c[id(m.fps_embedding[2])], d_emb)], pre=c["f1"])
            back([(c[id(m.fps_embedding[0])], d_f1)], need_dx=False)
        d_e1 = back([(c[id(m.time_embed[2])], d_emb)], pre=c["e1"])
        d_in = back([(c[id(m.time_embed[0])], d_e1)], need_dx="tc" in c)
        if "mc" in c:
            mc = m.model_channels
            d_cat = back([(c[id(m.combine_proj)], d_in)])
            back([(c[id(m.time_cond_proj)], d_cat[:, :mc])], need_dx=False)
            back([(c[id(m.motion_cond_proj)], d_cat[:, mc:])], need_dx=False)
        elif "tc" in c:
            back([(c[id(m.time_cond_proj)], d_in)], need_dx=False)

    def context_kv_t(self, attn, per_frame=False):
        """Training: K / V of ONE cross-attention layer through its own injected to_k / to_v (token-major rows of the text
        context), V^T by a per-image transpose.  (Inference stacks all 16 layers' projections into two GEMMs.)
        ``per_frame``: project the context repeated per frame, as the reference does — needed when the LoRA branches' dropout
        is active, so that every frame draws its own masks."""
        ops = self.ops
        B, L = self.B, self.ctx_len
        inner = attn.heads * attn.dim_head
        kp = _pad(L, 64)
        src, n_sets = self.ctx, B
        if per_frame:
            src, n_sets = self.context_per_frame(), B * self.F
        kind, self.row_kind = self.row_kind, ("rows" if per_frame else "ctx")
        k = self.linear(src, attn.to_k, bias=None)
        v = self.linear(src, attn.to_v, bias=None)
        self.row_kind = kind
        vt = self.buf(n_sets * inner, kp)
        ops.fill_zero(vt)
        ops.transpose(v, L, inner, vt, batch=n_sets, in_stride=L * inner, out_stride=inner * kp)
        self.pool.put(v)
        return k, vt, kp, inner * kp

    def context_per_frame(self):
        """The text context with each clip's rows repeated for its F frames ([(b f) l, D]; context.repeat_interleave of
        openaimodel3d.py:710), built once per forward."""
        if getattr(self, "_ctx_f", None) is None:
            B, F, L = self.B, self.F, self.ctx_len
            self._ctx_f = self.buf(B * F * L, self.ctx.shape[1])
            for b in range(B):
                for f in range(F):
                    self.ops.cast(self.ctx[b * L:(b + 1) * L], self._ctx_f[(b * F + f) * L:(b * F + f + 1) * L])
        return self._ctx_f

    def _backward_tape(self, dout, dx_out):
        if self.training_lora:
            self._seg_reset()
        d = self.exit_bwd(dout)
        skip_grads = []  # gradients of the skip tensors, in the order the output blocks produced them
        for kind, fn in reversed(self.tape):
            if kind == "split":
                c0 = fn
                # d is [M, c0 + c_skip]: the first c0 columns continue down the chain, the rest wait for their producer
                skip_grads.append((d.t, c0))
                d = Act(d.t[:, :c0], d.n_img, d.h, d.w)
            elif kind == "join":
                # the tensor this block produced was also a skip connection: add that gradient before going on
                buf, c0 = skip_grads.pop()
                total = self.add(d.t, buf[:, c0:])
                self._free_view(d.t)
                self.pool.put(buf)
                d = Act(total, d.n_img, d.h, d.w)
            else:
                d = fn(d)
        self.entry_bwd(d, dx_out)
        if self.plan.get("cond") is not None:
            self._conditioning_b()
        assert not (self.training_full and self._fsaved), "full fine-tuning: a saved leaf input was not taken by any backward"
        if self.training_lora:
            self._seg_emit_down_to(0)   # whatever is left of the arena (and every piece, if some group never finished)

    def _free_view(self, t):
        """Release a gradient tensor unless it is a column slice of a concat-gradient buffer (freed with the buffer)."""
        if t.data_ptr() in self.pool.live and t.stride(0) == t.shape[1]:
            self.pool.put(t)

    def checkpointed(self, block_t, layer, h):
        """``block_t(layer, h)`` (one tape entry) with the reference's checkpoint semantics: see ``checkpoint_blocks``."""
        if not self.checkpoint_blocks:
            return block_t(layer, h)
        pool, n_probs = self.pool, len(self.plan["probs"])
        if self.training_lora and self._active_dropouts():
            self.context_per_frame()                # shared by every cross-attention: must not belong to one block
        live0, refs0 = set(pool.live), dict(self.refs)
        n_tape, n_sites = len(self.tape), len(self.drop_sites)
        saved0 = {k: g.saved for k, g in getattr(self, "_groups", {}).items()}
        fmark = self.full_mark() if self.training_full else None
        y = block_t(layer, h)
        assert len(self.tape) == n_tape + 1 and self.tape[-1][0] == "block"
        if len(self.plan["probs"]) != n_probs:
            raise NotImplementedError("native checkpointing of a block that records attention_probs (record_attn_probs)")
        del self.tape[n_tape:]
        # nothing the block kept survives the forward, except its output (the next block's input) ...
        keep = {p.data_ptr() for p in y.parts}
        for q in list(keep):                        # (with the column statistics its producing GEMM wrote next to it)
            keep.update(side.data_ptr() for side in pool.links.get(q, ()))
        ctx_f = getattr(self, "_ctx_f", None)
        if ctx_f is not None:
            keep.add(ctx_f.data_ptr())
        for ptr in [q for q in pool.live if q not in live0 and q not in keep]:
            pool.release_ptr(ptr)
        # ... and what it holds of the tensors that were there before it (its input, the shared text context): those holds stay
        # until this block's backward has run, exactly as on the tape
        extra = {q: n - refs0.get(q, 0) for q, n in self.refs.items() if q in live0 and n > refs0.get(q, 0)}
        self.refs.clear()
        self.refs.update(refs0)
        for q, n in extra.items():
            self.refs[q] = self.refs.get(q, 0) + n
        for k, g in getattr(self, "_groups", {}).items():
            if g.saved is not saved0.get(k):
                g.saved = None
        if fmark is not None:
            # full fine-tuning: the leaf inputs the discarded forward recorded (their buffers went back to the pool above, and their
            # holds were rewound with ``refs``); the recomputation saves them again, and the block's backward takes them
            leaves_fwd = self.full_rewind(fmark)
        sites_fwd = self.drop_sites[n_sites:]

        def bwd(dy):
            outer_tape, outer_sites = self.tape, self.drop_sites
            self.tape, self.drop_sites = [], outer_sites[:n_sites]   # the block's dropout sites get the numbers they had
            fmark2 = self.full_mark() if self.training_full else None
            y2 = block_t(layer, h)
            assert [(k, m) for _, k, m in self.drop_sites[n_sites:]] == [(k, m) for _, k, m in sites_fwd]
            assert fmark2 is None or self.full_since(fmark2) == leaves_fwd, "the recomputation saved other leaf inputs than the forward"
            sub, self.tape, self.drop_sites = self.tape, outer_tape, outer_sites
            for p in y2.parts:                      # the recomputed output itself is not needed
                if self.refs.get(p.data_ptr(), 0) == 0 and p.data_ptr() in pool.live:
                    pool.put(p)
            d = dy
            for kind, fn in reversed(sub):
                assert kind == "block"
                d = fn(d)
            assert fmark2 is None or not self.full_since(fmark2), "a recomputed leaf input was not taken by the block's backward"
            for q, n in extra.items():              # the first forward's holds (the recomputation took and dropped its own)
                left = self.refs.get(q, 0) - n
                if left > 0:
                    self.refs[q] = left
                else:
                    self.refs.pop(q, None)
                    pool.release_ptr(q)
            return d

        self.tape.append(("block", bwd))
        return y

    def run_sequential_t(self, seq, h):
        assert isinstance(seq, TimestepEmbedSequential)
        for layer in seq:
            if isinstance(layer, ResBlock):
                h = self.checkpointed(self.res_block_t, layer, h)
            elif isinstance(layer, SpatialTransformer):
                h = self.checkpointed(self.spatial_transformer_t, layer, h)
            elif isinstance(layer, TemporalTransformer):
                h = self.checkpointed(self.temporal_transformer_t, layer, h)
            elif isinstance(layer, Downsample):
                assert layer.use_conv
                h = self.downsample_t(layer, h)
            elif isinstance(layer, Upsample):
                assert layer.use_conv
                src = h
                h = self.upsample_t(layer, h)
                if self.refs.get(src.t.data_ptr(), 0) == 0:  # an intermediate nobody keeps for the backward
                    self.pool.put(src.t)
            else:
                raise NotImplementedError(f"native gradient path: unsupported layer {type(layer).__name__}")
        return h

    # ---- blocks ----------------------------------------------------------------------------------------------------------
    def res_block_t(self, rb, x):
        B, F = self.B, self.F
        n, hw = x.n_img, x.h * x.w
        off, cout = self.emb_off[id(rb)], rb.out_channels
        self.hold(*x.parts)
        t1, st1 = self.gn_t(x, rb.in_layers[0], B * F, hw, True)
        h1 = self.conv(Act(t1, n, x.h, x.w), rb.in_layers[2], nt.GEMM_CONV3X3,
                       rowvec=self.emb_all[:, off:off + cout], rowvec_div=F * hw)
        self.rel(t1)
        t2, st2 = self.gn_t(h1, rb.out_layers[0], B * F, hw, True)
        identity = isinstance(rb.skip_connection, nn.Identity)
        if identity:
            skip, own = x.t, False
        else:
            sc = rb.skip_connection
            assert effective_weight_bias(sc)[0].shape[-1] == 1, "3x3 skip convs are not built by the VideoCrafter2 config"
            skip = self.linear(x, sc, conv_geom=(n, x.h, x.w))
            own = True
        h2 = self.conv(Act(t2, n, x.h, x.w), rb.out_layers[3], nt.GEMM_CONV3X3, residual=skip)
        self.rel(t2)
        if own:
            self.pool.put(skip)
        geom = (n, x.h, x.w)
        tc_bwd = None
        y = h2
        if rb.use_temporal_conv:
            y, tc_bwd = self.temporal_conv_block_t(rb.temopral_conv, h2)

        def bwd(dy):
            d_h2 = tc_bwd(dy) if tc_bwd is not None else dy.t
            d_t2 = self.conv_b(Act(d_h2, *geom), rb.out_layers[3], nt.GEMM_CONV3X3, geom)
            d_h1 = self.gn_b(h1, rb.out_layers[0], B * F, hw, True, st2, d_t2.t)
            self.pool.put(d_t2.t, h1.t, st2)
            # training: the per-clip column sums of d_h1 are d(loss)/d(emb_all) of this block (rowvec of the forward conv)
            colsum = self.plan["d_emb"][:, off:off + cout] if self.training_lora else None
            if self.training_full:
                self.full_colsum(d_h1, self.plan["d_emb"][:, off:off + cout], F * hw)
            d_t1 = self.conv_b(Act(d_h1, *geom), rb.in_layers[2], nt.GEMM_CONV3X3, geom, colsum=colsum)
            self.pool.put(d_h1)
            d_skip = d_h2 if identity else self.lin_b(d_h2, self.pk.mat_t(rb.skip_connection), lora=[rb.skip_connection])
            dx = self.gn_b(x, rb.in_layers[0], B * F, hw, True, st1, d_t1.t, resid=d_skip)
            self.pool.put(d_t1.t, st1)
            if not identity:
                self.pool.put(d_skip)
            self._free_view(d_h2)
            self.drop(*x.parts)
            return Act(dx, *geom)

        self.tape.append(("block", bwd))
        return y

    def temporal_conv_block_t(self, tc, h2):
        """-> (output, backward closure: dy Act -> gradient w.r.t. h2 as a tensor)."""
        B, F = self.B, self.F
        n, hw = h2.n_img, h2.h * h2.w
        geom = (n, h2.h, h2.w)
        stages = (tc.conv1, tc.conv2, tc.conv3, tc.conv4)
        saved = []
        y = h2
        for i, stage in enumerate(stages):
            tt, st = self.gn_t(y, stage[0], B, F * hw, True)
            site = self.drop_site([l for l in stage if isinstance(l, nn.Dropout)], "tconv", (B, F, h2.h, h2.w)) if len(stage) > 3 else None
            if site is not None:  # train-mode student: Dropout between SiLU and the (3,1,1) conv (openaimodel3d.py:280-297)
                self.ops.dropout(tt, None, tt, tt.shape[1], site[0], self.seed_t, site[1])
            ny = self.conv(Act(tt, *geom), stage[-1], nt.GEMM_TCONV3, frames=F, residual=h2.t if i == 3 else None)
            self.rel(tt)
            saved.append((y, st, site))
            y = ny

        def bwd(dy):
            d = dy.t
            for i in (3, 2, 1, 0):
                yi, st, site = saved[i]
                d_tt = self.conv_b(Act(d, *geom), stages[i][-1], nt.GEMM_TCONV3, geom, frames=F)
                if site is not None:
                    self.ops.dropout(d_tt.t, None, d_tt.t, d_tt.t.shape[1], site[0], self.seed_t, site[1])
                if i != 3:
                    self.pool.put(d)
                nd = self.gn_b(yi, stages[i][0], B, F * hw, True, st, d_tt.t, resid=dy.t if i == 0 else None)
                self.pool.put(d_tt.t, st)
                if i != 0:
                    self.pool.put(yi.t)  # h2 itself (i == 0) belongs to the residual block's closure
                d = nd
            self._free_view(dy.t)
            self.pool.put(h2.t)
            return d

        return y, bwd

    def downsample_t(self, layer, x):
        y = self.conv(x, layer.op, nt.GEMM_CONV3X3_S2)
        n, h, w, cin = x.n_img, x.h, x.w, x.C

        def bwd(dy):
            dx = self.conv_b(dy, layer.op, nt.GEMM_CONV3X3_S2, (n, h, w))
            self._free_view(dy.t)
            return dx

        self.tape.append(("block", bwd))
        return y

    def upsample_t(self, layer, x):
        y = self.conv(x, layer.conv, nt.GEMM_CONV3X3_UP2)
        n, h, w, cin = x.n_img, x.h, x.w, x.C

        def bwd(dy):
            dx = self.conv_b(dy, layer.conv, nt.GEMM_CONV3X3_UP2, (n, h, w))
            self._free_view(dy.t)
            return dx

        self.tape.append(("block", bwd))
        return y

    def spatial_transformer_t(self, st, x):
        return self._transformer_t(st, x, temporal=False)

    def temporal_transformer_t(self, tt, x):
        return self._transformer_t(tt, x, temporal=True)

    def _transformer_t(self, tr, x, temporal):
        B, F = self.B, self.F
        n, hw = x.n_img, x.h * x.w
        units, rows = (B, F * hw) if temporal else (B * F, hw)
        self.row_kind = "temporal" if temporal else "rows"
        self.hold(x.t)
        t, stats = self.gn_t(x, tr.norm, units, rows, False)
        y = self.linear(t, tr.proj_in)
        self.rel(t)
        blocks = []
        for blk in tr.transformer_blocks:
            y, b = self.transformer_block_t(blk, y, (n, hw), temporal)
            blocks.append(b)
        out = self.linear(y, tr.proj_out, residual=x.t, want_cs=True)
        out_cs = self.last_cs
        self.rel(y)
        geom = (n, x.h, x.w)

        def bwd(dy):
            d = self.lin_b(dy.t, self.pk.mat_t(tr.proj_out), lora=[tr.proj_out])
            for b in reversed(blocks):
                d = b(d)
            d_t = self.lin_b(d, self.pk.mat_t(tr.proj_in), lora=[tr.proj_in])
            self.pool.put(d)
            dx = self.gn_b(x, tr.norm, units, rows, False, stats, d_t, resid=dy.t)
            self.pool.put(d_t, stats)
            self._free_view(dy.t)
            self.drop(x.t)
            return Act(dx, *geom)

        self.tape.append(("block", bwd))
        return Act(out, *geom, cs=[out_cs])

    def transformer_block_t(self, blk, y, x_geom, temporal):
        """-> (output rows, backward closure: d(output) tensor -> d(input) tensor).  The block's input y stays alive
        until the closure ran; the closure frees it."""
        ops, pk = self.ops, self.pk
        B, F = self.B, self.F
        M, C = y.shape
        n_img, hw = x_geom
        a1, a2 = blk.attn1, blk.attn2
        self._check_heads(a1)
        inner = a1.heads * a1.dim_head

        def lnorm(norm, src):
            ln = self.buf(M, C)
            ops.layernorm(src, pk.f32(norm.weight), pk.f32(norm.bias), norm.eps, ln)
            return ln

        def ln_b(norm, src, d_ln, resid):
            if self.training_full:
                self.full_norm_grads(norm, src, d_ln, kind=1)
            dx = self.buf(M, C)
            ops.layernorm_bwd(src, pk.f32(norm.weight), norm.eps, d_ln, resid, dx)
            return dx

        # ---- attention flavours: forward returns (o, backward: d_o -> d(ln input of the attention)) ------------------
        def temporal_attn(attn, src):
            mods = [attn.to_q, attn.to_k, attn.to_v]
            qkv = self.linear(src, None, w=pk.cat_mats(mods, "qkv"), bias=None, lora=mods)
            o = self.buf(M, inner)
            probs = dprobs = None
            if attn.record_attn_probs:
                probs = torch.empty(B * hw * attn.heads, F, F, dtype=torch.float32, device=self.device)
                self.plan["probs"].append((attn, probs))
                dprobs = self.plan["dprobs"].setdefault(id(attn), torch.zeros_like(probs))
            ops.attn_temporal(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], o, B, F, hw, attn.heads, attn.scale, probs)

            def bwd(d_o):
                dqkv = self.buf(M, 3 * inner)
                ops.attn_temporal_bwd(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], d_o, dprobs,
                                      dqkv[:, :inner], dqkv[:, inner:2 * inner], dqkv[:, 2 * inner:], B, F, hw, attn.heads, attn.scale)
                self.pool.put(qkv, d_o)
                d_ln = self.lin_b(dqkv, self.pk.mats_t(mods, "qkv_t"), lora=mods)
                self.pool.put(dqkv)
                return d_ln
            return o, bwd

        def spatial_self_attn(attn, src):
            heads = attn.heads
            qk = self.linear(src, None, w=pk.cat_mats([attn.to_q, attn.to_k], "qk"), bias=None, lora=[attn.to_q, attn.to_k])
            kp = ((hw + 63) // 64) * 64
            vt = self.buf(n_img * inner, kp)
            if kp != hw:
                ops.fill_zero(vt)
            if (self.training_lora and is_lora_leaf(attn.to_v)) or self.training_full:
                # training: V token-major through the injected leaf, then transposed per image (inference: V^T straight
                # out of a GEMM with the weight as the row operand)
                v = self.linear(src, attn.to_v, bias=None)
                ops.transpose(v, hw, inner, vt, batch=n_img, in_stride=hw * inner, out_stride=inner * kp)
                if not self.flash_attn_bwd:
                    self.pool.put(v)
                    v = None
            else:
                v = None
                ops.gemm(pk.mat(attn.to_v), src, vt, M=inner, N=hw, batch=n_img, w_strides=(hw * src.stride(0), 0), o_strides=(inner * kp, 0))
            o = self.buf(M, inner)
            ops.attn_spatial(qk[:, :inner], qk[:, inner:], vt, kp, o, n_img, hw, hw, heads, 1, attn.scale)
            nb = n_img * heads
            if self.flash_attn_bwd:
                self.hold(o)  # the flash-style backward needs the forward's output (D = rowsum(dO * O))

            def bwd_flash(d_o):
                """dQ / dK / dV without the [queries x keys] matrices in memory (csrc/attention_bwd.hip): two launches + the
                three small operand transposes, instead of 5 batched GEMMs over 2 x 1 GB matrices, 2 softmax passes and 4 large
                transposes at the 2560-token level."""
                q, k = qk[:, :inner], qk[:, inner:]
                ld = qk.stride(0)
                if v is not None:   # token-major V of the training path
                    v_buf, vis, vhs = v, hw * inner, 64
                else:               # per (image, head) [keys][64]: the transpose of the forward's V^T rows
                    v_buf = self.buf(nb * kp, 64)
                    ops.transpose(vt, 64, kp, v_buf, batch=nb, in_stride=64 * kp, out_stride=kp * 64)
                    vis, vhs = heads * kp * 64, kp * 64
                kT = self.tposed(k, hw, inner, batch=n_img, in_stride=hw * ld)
                qT = self.tposed(q, hw, inner, batch=n_img, in_stride=hw * ld)
                doT = self.tposed(d_o, hw, inner, batch=n_img, in_stride=hw * inner)
                l2, dsum = self.buf(nb, kp, torch.float32), self.buf(nb, kp, torch.float32)
                dqk, d_v = self.buf(M, 2 * inner), self.buf(M, inner)
                ops.attn_spatial_bwd(q, k, v_buf, vis, vhs, kT, qT, doT, d_o, o, l2, dsum, dqk[:, :inner], dqk[:, inner:], d_v,
                                     n_img, hw, heads, attn.scale)
                self.pool.put(kT, qT, doT, l2, dsum, v_buf, vt, qk, d_o)
                self.drop(o)
                d1 = self.lin_b(dqk, self.pk.mats_t([attn.to_q, attn.to_k], "qk_t"), lora=[attn.to_q, attn.to_k])
                d_ln = self.lin_b(d_v, pk.mat_t(attn.to_v), residual=d1, lora=[attn.to_v])
                self.pool.put(dqk, d_v, d1)
                return d_ln

            def tposed(src2d, rows, cols, in_stride, batch):
                """[batch][rows][cols] -> [batch][cols][kp] (rows padded with zeros up to kp)."""
                dst = self.buf(batch * cols, kp)
                if kp != rows:
                    ops.fill_zero(dst)
                ops.transpose(src2d, rows, cols, dst, batch=batch, in_stride=in_stride, out_stride=cols * kp)
                return dst

            def bwd(d_o):
                q, k = qk[:, :inner], qk[:, inner:]
                ld = qk.stride(0)
                hb = dict(batch=nb, batch_inner=heads)
                # P = softmax(scale * Q K^T) per (image, head): rows (img, head, q), kp columns
                s = self.buf(nb * hw, kp)
                if kp != hw:
                    ops.fill_zero(s)
                ops.gemm(q[:, :64], k[:, :64], s, M=hw, N=hw, alpha=attn.scale, a_strides=(hw * ld, 64), w_strides=(hw * ld, 64),
                         o_strides=(heads * hw * kp, hw * kp), **hb)
                ops.softmax_rows(s, nb * hw, hw, kp, kp)
                # dP[q][kv] = sum_c dO[q][c] V[kv][c]: W = V token-major per head = transpose of the V^T rows
                v_tok = self.buf(nb * kp, 64)
                ops.transpose(vt, 64, kp, v_tok, batch=nb, in_stride=64 * kp, out_stride=kp * 64)
                dp = self.buf(nb * hw, kp)
                ops.gemm(d_o[:, :64], v_tok, dp, M=hw, N=kp, a_strides=(hw * inner, 64), w_strides=(heads * kp * 64, kp * 64),
                         o_strides=(heads * hw * kp, hw * kp), **hb)
                self.pool.put(v_tok, vt)
                # dV[kv][c] = sum_q P[q][kv] dO[q][c]: A = P^T [kv][q], W = dO^T [c][q] (one transpose per image covers all heads)
                pT = tposed(s, hw, kp, hw * kp, nb)                       # [nb][kp][kp]
                doT = tposed(d_o, hw, inner, hw * inner, n_img)           # [n_img][inner][kp] = [nb][64][kp]
                self.pool.put(d_o)
                d_v = self.buf(M, inner)
                ops.gemm(pT, doT, d_v[:, :64], M=hw, N=64, a_strides=(heads * kp * kp, kp * kp), w_strides=(inner * kp, 64 * kp),
                         o_strides=(hw * inner, 64), **hb)
                self.pool.put(pT, doT)
                ops.softmax_bwd_rows(s, dp, nb * hw, hw, kp, kp)         # dS in place on dP
                self.pool.put(s)
                dqk = self.buf(M, 2 * inner)
                kT = tposed(k, hw, inner, hw * ld, n_img)
                ops.gemm(dp, kT, dqk[:, :64], M=hw, N=64, alpha=attn.scale, a_strides=(heads * hw * kp, hw * kp),
                         w_strides=(inner * kp, 64 * kp), o_strides=(hw * 2 * inner, 64), **hb)
                self.pool.put(kT)
                dsT = tposed(dp, hw, kp, hw * kp, nb)
                qT = tposed(q, hw, inner, hw * ld, n_img)
                self.pool.put(dp, qk)
                ops.gemm(dsT, qT, dqk[:, inner:inner + 64], M=hw, N=64, alpha=attn.scale, a_strides=(heads * kp * kp, kp * kp),
                         w_strides=(inner * kp, 64 * kp), o_strides=(hw * 2 * inner, 64), **hb)
                self.pool.put(dsT, qT)
                d1 = self.lin_b(dqk, self.pk.mats_t([attn.to_q, attn.to_k], "qk_t"), lora=[attn.to_q, attn.to_k])
                d_ln = self.lin_b(d_v, pk.mat_t(attn.to_v), residual=d1, lora=[attn.to_v])
                self.pool.put(dqk, d_v, d1)
                return d_ln
            return o, (bwd_flash if self.flash_attn_bwd else bwd)

        def cross_attn(attn, src):
            heads, L = attn.heads, self.ctx_len
            q = self.linear(src, attn.to_q, bias=None)
            own_kv = (self.training_lora and is_lora_leaf(attn.to_k) and is_lora_leaf(attn.to_v)) or self.training_full
            # The frames of a clip share the text K / V (one attention of F*hw queries over L keys per clip and head) — unless
            # the train-mode student's dropout sits on the to_k / to_v LoRA branches: the reference projects the context
            # REPEATED per frame (openaimodel3d.py:710), so every frame draws its own masks and has its own K / V.
            per_frame = own_kv and self.training_lora and any(d.training and d.p > 0 for d in (attn.to_k.dropout, attn.to_v.dropout))
            nf = F if per_frame else 1           # K / V sets per clip
            mq = hw if per_frame else F * hw     # queries per K / V set
            if own_kv:
                k, vt, kp, vt_stride = self.context_kv_t(attn, per_frame)
            else:
                k, vt, kp, vt_stride = self.context_kv(attn)
            o = self.buf(M, inner)
            ops.attn_spatial(q, k, vt, kp, o, n_img, hw, L, heads, 1 if per_frame else F, attn.scale, vt_stride)

            def bwd(d_o):
                d_q = self.buf(M, inner)
                dk = dv = None
                if own_kv:  # the text context itself carries no gradient, its injected to_k / to_v projections do
                    dk, dv = self.buf(B * nf * L, inner), self.buf(B * nf * L, inner)
                    mqp = _pad(mq, 64)
                ldk = k.stride(0)
                hb = dict(batch=nf * heads, batch_inner=heads)  # z0 = K / V set (frame) of the clip, z1 = head
                for b in range(B):
                    rows = slice(b * F * hw, (b + 1) * F * hw)
                    qb, dob, dqb = q[rows], d_o[rows], d_q[rows]
                    kb = k[b * nf * L:(b + 1) * nf * L]
                    vtb = torch.as_strided(vt, (nf * inner, kp), (kp, 1), vt.storage_offset() + b * nf * vt_stride)
                    s = self.buf(nf * heads * mq, kp)
                    ops.fill_zero(s)
                    so = (heads * mq * kp, mq * kp)
                    ops.gemm(qb[:, :64], kb[:, :64], s, M=mq, N=L, alpha=attn.scale, a_strides=(mq * inner, 64), w_strides=(L * ldk, 64),
                             o_strides=so, **hb)
                    ops.softmax_rows(s, nf * heads * mq, L, kp, kp)
                    v_tok = self.buf(nf * heads * kp, 64)
                    ops.transpose(vtb, 64, kp, v_tok, batch=nf * heads, in_stride=64 * kp, out_stride=kp * 64)
                    dp = self.buf(nf * heads * mq, kp)
                    ops.gemm(dob[:, :64], v_tok, dp, M=mq, N=kp, a_strides=(mq * inner, 64), w_strides=(heads * kp * 64, kp * 64),
                             o_strides=so, **hb)
                    self.pool.put(v_tok)
                    kv_rows = slice(b * nf * L, (b + 1) * nf * L)
                    wg = dict(a_strides=(heads * kp * mqp, kp * mqp), w_strides=(inner * mqp, 64 * mqp), o_strides=(L * inner, 64),
                              split_k=self.split_for(L * heads, 64, mqp), **hb) if own_kv else None
                    if own_kv:  # dV[kv][c] = sum_q P[q][kv] dO[q][c], contraction over all queries of the K / V set
                        pT = self.tposed(s, mq, kp, batch=nf * heads, in_stride=mq * kp)
                        doT = self.tposed(dob, mq, inner, batch=nf, in_stride=mq * inner)
                        ops.gemm(pT, doT, dv[kv_rows][:, :64], M=L, N=64, **wg)
                        self.pool.put(pT, doT)
                    ops.softmax_bwd_rows(s, dp, nf * heads * mq, L, kp, kp)
                    self.pool.put(s)
                    kT = self.buf(nf * inner, kp)
                    ops.fill_zero(kT)
                    ops.transpose(kb, L, inner, kT, batch=nf, in_stride=L * ldk, out_stride=inner * kp)
                    ops.gemm(dp, kT, dqb[:, :64], M=mq, N=64, alpha=attn.scale, a_strides=so, w_strides=(inner * kp, 64 * kp),
                             o_strides=(mq * inner, 64), **hb)
                    self.pool.put(kT)
                    if own_kv:  # dK[kv][c] = scale * sum_q dS[q][kv] Q[q][c]
                        dsT = self.tposed(dp, mq, kp, batch=nf * heads, in_stride=mq * kp)
                        qT = self.tposed(qb, mq, inner, batch=nf, in_stride=mq * inner)
                        ops.gemm(dsT, qT, dk[kv_rows][:, :64], M=L, N=64, alpha=attn.scale, **wg)
                        self.pool.put(dsT, qT)
                    self.pool.put(dp)
                self.pool.put(q, d_o)
                if own_kv:
                    self.lin_b(dk, None, lora=[attn.to_k], need_dx=False)
                    self.lin_b(dv, None, lora=[attn.to_v], need_dx=False)
                    self.pool.put(dk, dv, k, vt)
                d_ln = self.lin_b(d_q, pk.mat_t(attn.to_q), lora=[attn.to_q])
                self.pool.put(d_q)
                return d_ln
            return o, bwd

        # ---- forward ------------------------------------------------------------------------------------------------
        ln = lnorm(blk.norm1, y)
        o, attn1_b = temporal_attn(a1, ln) if temporal else spatial_self_attn(a1, ln)
        self.rel(ln)
        y1 = self.linear(o, a1.to_out[0], residual=y)
        self.rel(o)
        ln = lnorm(blk.norm2, y1)
        o, attn2_b = temporal_attn(a2, ln) if temporal else cross_attn(a2, ln)
        self.rel(ln)
        y2 = self.linear(o, a2.to_out[0], residual=y1)
        self.rel(o)
        ln = lnorm(blk.norm3, y2)
        proj = blk.ff.net[0]
        assert hasattr(proj, "proj"), "non-gated FeedForward is not built by the VideoCrafter2 config"
        wg, bg = pk.geglu(proj.proj)
        ff_inner = wg.shape[0] // 2
        j = torch.arange(2 * ff_inner)  # packed GEGLU row j (64-row groups [32 value | 32 gate]) <- original projection row
        geglu_perm = (j // 64) * 32 + (j % 32) + (j % 64 >= 32) * ff_inner
        # pre-activation kept for the backward (packed value | gate groups)
        hpre = self.linear(ln, None, w=wg, bias=bg, lora=[proj.proj], perm=geglu_perm)
        self.rel(ln)
        g = self.buf(M, hpre.shape[1] // 2)
        ops.geglu_fwd(hpre, g)
        y3 = self.linear(g, blk.ff.net[2], residual=y2)
        self.rel(g)

        def bwd(dy3):
            d_g = self.lin_b(dy3, pk.mat_t(blk.ff.net[2]), lora=[blk.ff.net[2]])
            d_h = self.buf(M, hpre.shape[1])
            ops.geglu_bwd(hpre, d_g, d_h)
            self.pool.put(d_g, hpre)
            d_ln3 = self.lin_b(d_h, pk.geglu_t(proj.proj), lora=[proj.proj])
            self.pool.put(d_h)
            d_y2 = ln_b(blk.norm3, y2, d_ln3, dy3)
            self.pool.put(d_ln3, dy3, y2)
            d_o2 = self.lin_b(d_y2, pk.mat_t(a2.to_out[0]), lora=[a2.to_out[0]])
            d_ln2 = attn2_b(d_o2)
            d_y1 = ln_b(blk.norm2, y1, d_ln2, d_y2)
            self.pool.put(d_ln2, d_y2, y1)
            d_o1 = self.lin_b(d_y1, pk.mat_t(a1.to_out[0]), lora=[a1.to_out[0]])
            d_ln1 = attn1_b(d_o1)
            d_y = ln_b(blk.norm1, y, d_ln1, d_y1)
            self.pool.put(d_ln1, d_y1, y)
            return d_y

        return y3, bwd
