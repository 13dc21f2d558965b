"""Base-weight gradients of the student UNet on the native gradient engine: FULL fine-tuning, the call pattern of
``train_latent_t2v_turbo_v2.py`` (``:669`` ``unet.requires_grad_(True).train()``, ``:798-816`` every UNet parameter in an optimizer
group, ``:1262`` ``accelerator.backward``) — no LoRA injection, every leaf trainable.

The tape and the data gradients are the gradient engine's (engine_unet_bwd.py).  This mixin adds, at every leaf's backward,

  Linear / 1x1 conv        dW = dy^T x                     ``t2v_wgrad_tn`` on the token-major operands (per leaf of a q | k | v group,
                                                            per input part of a virtual concat); GEGLU: rows un-permuted by one gather
  3x3 / strided / x2 /     dW[n][tap][c] = dy^T xcol       ``t2v_im2col_bf16`` (the shifted-row matrix in the forward pack's K order) +
  (3,1,1) conv                                              ``t2v_wgrad_tn`` + one ``t2v_gather_f32`` into the parameter's [N, C, k..] layout
  bias                     db = column sums of dy          ``t2v_norm_affine_grad`` kind 2
  GroupNorm / LayerNorm    dgamma, dbeta                   ``t2v_norm_affine_grad`` kinds 0 / 1 (SiLU behind the norm included)
  time-embedding rows      d(loss)/d(emb_all)              per-clip column sums of the ResBlock's conv gradient (kind 2, sum_rows = F h w)

into one fp32 tensor per parameter (``plan["fgrads"]``), which the autograd bridge (bridge._NativeStudentFull) hands to torch.
The conditioning branch (time / fps / guidance MLPs, ``emb_layers``: B rows) stays with torch autograd behind ``emb_all``, as in LoRA
training — or, with ``native_conditioning`` on, runs on the engine as well (t2v_rowlin_* on the live fp32 parameters, no packs: nothing
below that refreshes packs sees those leaves).  The weights change every optimizer step: the Packer re-fills its packs IN PLACE (``Packer.refresh``), so the recorded launch
lists — raw device pointers — stay valid and nothing is re-recorded.  Every plan (input signature) owns its Packer and is refreshed on
its own, when its packs are behind the parameters.

Activation checkpointing (``checkpoint_blocks``, the yaml's ``use_checkpoint: true``) works with this mixin: what it keeps per leaf between
forward and backward is ``_fsaved`` alone, and ``engine_unet_bwd.checkpointed`` rewinds it with a block's discarded forward
(``full_mark`` / ``full_rewind``); the recomputation inside the block's backward saves the same leaves again and the leaf backwards take
them.  Same gradients bit for bit (tests/test_unet_full_ckpt_cpu.py, tests/test_gpu_full_ckpt.py).

Correctness first: im2col is materialised (2 taps C bytes per output row) and every leaf's gradient is its own launches; the step is
not a measured configuration of bench.py.  Verified on CPU against torch autograd through the module (tests/test_unet_full_grad_cpu.py),
on the host simulator per kernel, and on MI355X against the imported reference's own parameter gradients (tests/golden/unet_tiny_full_grad.npz)."""
import torch
import torch.nn as nn

from . import native as nt
from .engine import is_lora_leaf


class FullTrainMixin:
    full_params = None

    def bind_full(self, params):
        """``params``: the parameters whose gradients the engine computes (every UNet parameter outside the conditioning branch)."""
        self.full_params = list(params)
        self.full_ids = {id(p) for p in self.full_params}
        self.plans.clear()             # (with every plan go its Packer, its weight fingerprint and its captured refresh)
        self.fingerprint = None
        self._last = None

    @property
    def training_full(self):
        return self.full_params is not None

    @property
    def trains(self):
        """LoRA training or full fine-tuning: the forward keeps what weight gradients need, dropouts are applied, emb_all is an input."""
        return self.training_full or getattr(self, "lora_params", None) is not None

    @staticmethod
    def conditioning_module_ids(model):
        """Modules of the B-row conditioning branch (their parameters' gradients are torch's, through ``emb_all``, unless the engine
        owns the branch: ``UNetGradEngine.native_conditioning``)."""
        from .unet3d import ResBlock
        cond = set()
        for name in ("time_embed", "fps_embedding", "time_cond_proj", "motion_cond_proj", "combine_proj"):
            sub = getattr(model, name, None)
            if sub is not None:
                cond.update(id(x) for x in sub.modules())
        for mod in model.modules():
            if isinstance(mod, ResBlock):
                cond.update(id(x) for x in mod.emb_layers.modules())
        return cond

    @classmethod
    def engine_parameters(cls, model, conditioning=False):
        """Every parameter of ``model`` the engine differentiates, in ``named_parameters`` order.  ``conditioning``: the engine owns the
        B-row branch too (``UNetGradEngine.native_conditioning``) — then that is every parameter."""
        cond = set() if conditioning else cls.conditioning_module_ids(model)
        out, seen = [], set()
        for mod in model.modules():
            if id(mod) in cond:
                continue
            for p in mod._parameters.values():
                if p is not None and id(p) not in seen:
                    seen.add(id(p))
                    out.append(p)
        return out

    # ---- per-step pack refresh ------------------------------------------------------------------------------------------
    # Every full-mode plan OWNS its Packer (``plan["owned"]``): its launch list holds the raw pointers of those packs.  So everything the
    # refresh keeps lives IN THE PLAN — the fingerprint of the weights its packs were filled from (``full_fp``) and the captured refresh
    # (``refresh``) — and goes with it when the plan is evicted, when ``bind_full`` drops all plans, or when it is recorded again.  A second
    # input signature (the partial last batch of an epoch) then costs a second set of packs, and going back to the first plan after an
    # optimizer step re-fills ITS packs first.  (One engine-wide fingerprint and ``self.pk`` = the Packer recorded last used to leave every
    # other plan on bf16 packs of old weights next to live fp32 affines; one shared Packer instead would have to be brought up to date
    # before every recording and re-captured whenever a new signature adds a pack.)
    def full_activate(self, plan):
        """Put the engine on ``plan``: the Packer its launches point into, and — for the closure backends of the tests, which re-run the
        forward in Python — its pool, kept tensors and geometry."""
        self.plan = plan
        self.pool, self.pk, self.keep = plan["owned"]
        self.B, self.F = plan["geom"]
        self.device = plan["out"].device

    def full_refresh_packs(self, plan):
        """Re-fill the weight packs of ``plan`` in place when a parameter changed since they were filled (its launch list keeps its pointers)."""
        from .engine import params_fingerprint
        fp = params_fingerprint(self.model)
        if fp != plan["full_fp"]:
            self._refresh(plan)
            plan["full_fp"] = fp

    @property
    def _refresh_state(self):
        """The refresh bookkeeping of the plan that ran last (None: no refresh on the device yet); there is none outside the plans."""
        last = getattr(self, "_last", None)
        return None if last is None else last.get("refresh")

    # The pass itself is ``_Engine._refresh_packs`` (eager, then captured as ONE hipGraph and replayed per optimizer step), shared with
    # the inference engine; here its state lives in the plan, next to the Packer the plan owns.
    def _refresh(self, plan):
        pk = plan["owned"][1]
        assert pk is self.pk, "the pack refresh runs on the Packer of the plan being replayed (full_activate)"
        self._refresh_packs(pk, plan, self.model)

    # ---- forward side: keep the leaf's input ----------------------------------------------------------------------------
    def full_save(self, mods, x, **info):
        if any(is_lora_leaf(mm) for mm in mods):
            raise NotImplementedError("native full fine-tuning of a LoRA-injected network (train the LoRA tensors, or merge them first)")
        key = tuple(id(mm) for mm in mods)
        assert key not in self._fsaved, "a leaf input is saved once per forward (a checkpointed block's discarded forward is rewound: full_rewind)"
        self.hold(*x.parts)
        self._fsaved[key] = (x, info)

    def full_take(self, mods):
        x, info = self._fsaved.pop(tuple(id(mm) for mm in mods))
        return x, info

    # ---- activation checkpointing (engine_unet_bwd.checkpointed) --------------------------------------------------------
    # Everything this mixin keeps between a leaf's forward and its backward is in ``_fsaved``: the leaf's input Act (both parts of a
    # virtual concat; one entry for a q | k | v group) and the GEGLU row permutation.  The rest is either in the block's closures — the
    # GroupNorm statistics ``full_norm_grads`` reads and the per-clip text K / V of ``own_kv`` are pool buffers the discarded forward
    # gives back and the recomputation allocates again — or written by the backward alone: the ``d_emb`` column sums (once, from the
    # recomputed block's own backward) and the gradient arena, which is made at the first ``fgrad`` of the backward recording whether
    # that is the exit conv's or a recomputed block's.
    def full_mark(self):
        """How many leaf inputs are saved (taken before a checkpointed block runs).  Saving appends to ``_fsaved`` and a block takes only what
        it saved itself, so the entries older than a mark keep their places: what came after it is the tail of the insertion order."""
        return len(self._fsaved)

    def full_since(self, mark):
        """Leaf keys saved after ``mark`` and not taken yet, in saving order."""
        return list(self._fsaved)[mark:]

    def full_rewind(self, mark):
        """Forget what a block's discarded forward saved since ``mark`` -> those keys.  No ``drop``: the caller released the block's buffers
        and rewound ``refs``; what the block held of tensors older than itself stays held until its backward (``extra``)."""
        gone = self.full_since(mark)
        for k in gone:
            del self._fsaved[k]
        return gone

    def fgrad(self, p):
        """The fp32 gradient tensor of parameter ``p``: a view into the plan's gradient arena (one allocation for all parameters, made at the
        first request: recorded launches point into it, and the hand-over to torch is ONE copy of the arena instead of one per tensor)."""
        g = self.plan["fgrads"].get(id(p))
        if g is None:
            assert id(p) in self.full_ids, "a leaf parameter that was not given to bind_full"
            if self.plan.get("fgrad_arena") is None:
                off, offs = 0, {}
                for q in self.full_params:
                    offs[id(q)] = off
                    off += (q.numel() + 63) // 64 * 64        # (256-byte aligned views)
                self.plan["fgrad_off"] = offs
                self.plan["fgrad_arena"] = torch.zeros(off, dtype=torch.float32, device=self.device)
            o = self.plan["fgrad_off"][id(p)]
            g = self.plan["fgrads"][id(p)] = self.plan["fgrad_arena"][o:o + p.numel()].view(p.shape)
        return g

    def _idx(self, key, make):
        return self.pk.pack(("full_idx",) + key, lambda: make().to(torch.int32).to(self.device).contiguous(), static=True)

    def full_wgrad(self, dy, xmat, out):
        """out[R, C] = dy^T xmat by t2v_wgrad_tn (one launch pair, or one launch where the product has enough output tiles to fill the
        chip without splitting the token range — then it needs no partial slabs, however large the output: 1 280 x 23 040 fp32 = 118 MB
        for the 2 560-channel 3x3 convs of the decoder half)."""
        self.ops.wgrad_tn(dy, xmat, out)

    def full_colsum(self, dy, dst, sum_rows):
        """dst[u][c] = sum of ``sum_rows`` consecutive rows of dy (fp32 [rows / sum_rows, C], a column slice of a wider buffer allowed)."""
        ops = self.ops
        ws = self.buf(1, max(ops.norm_affine_grad_ws_floats(dy.shape[0], sum_rows, dy.shape[1]), 1), torch.float32)
        ops.norm_affine_grad(None, None, dy, kind=2, sum_rows=sum_rows, ws=ws, dbeta=dst)
        self.pool.put(ws)

    def full_bias_grad(self, bias, dy, inv_perm=None):
        if bias is None:
            return
        g = self.fgrad(bias)
        if inv_perm is None and dy.shape[1] == bias.numel():
            self.full_colsum(dy, g.view(1, -1), dy.shape[0])
            return
        tmp = self.buf(1, dy.shape[1], torch.float32)
        self.full_colsum(dy, tmp, dy.shape[0])
        idx = inv_perm if inv_perm is not None else self._idx(("head", bias.numel()), lambda: torch.arange(bias.numel()))
        self.ops.gather(tmp, idx, g)
        self.pool.put(tmp)

    def full_linear_grads(self, mods, dy):
        """dW (and db) of the Linear / 1x1-conv leaves ``mods`` whose row-concatenated weights produced dy's columns."""
        ops = self.ops
        x, info = self.full_take(mods)
        perm = info.get("perm")
        off = 0
        for mod in mods:
            w, b = mod.weight, mod.bias
            n, k = w.shape[0], w.numel() // w.shape[0]
            d = dy[:, off:off + n]
            off += n
            if perm is None:
                g2 = self.fgrad(w).view(n, k)
                c0 = x.parts[0].shape[1]
                self.full_wgrad(d, x.parts[0], g2[:, :c0])
                if x.p1 is not None:
                    self.full_wgrad(d, x.p1, g2[:, c0:])
                self.full_bias_grad(b, d)
            else:
                # packed output row j = original row perm[j] (GEGLU's [32 value | 32 gate] groups): gradient rows go back through the inverse
                assert len(mods) == 1 and x.p1 is None
                tmp = self.buf(n, k, torch.float32)
                self.full_wgrad(d, x.parts[0], tmp)
                inv = torch.empty_like(perm)
                inv[perm] = torch.arange(perm.numel())
                idx_w = self._idx(("rows", id(mod), n, k), lambda: (inv[:, None] * k + torch.arange(k)[None, :]).reshape(-1))
                ops.gather(tmp, idx_w, self.fgrad(w))
                self.pool.put(tmp)
                self.full_bias_grad(b, d, inv_perm=self._idx(("rows_b", id(mod), n), lambda: inv))
        self.drop(*x.parts)

    def full_conv_grads(self, mod, mode, dy):
        """dW (and db) of a 3x3 / strided / upsampled / temporal conv leaf; dy: its output gradient [M_out, N] (bf16, token-major)."""
        ops = self.ops
        x, info = self.full_take([mod])
        w, b = mod.weight, mod.bias
        n, cp = w.shape[0], w.shape[1]        # (the parameter's own channel counts: the operands may be zero-padded to 8)
        C = x.C
        taps = 3 if mode == nt.GEMM_TCONV3 else 9
        assert w.numel() == n * cp * taps and cp <= C and n <= dy.shape[1]
        rows = ops.im2col_rows(mode, x.n_img, x.h, x.w)
        assert rows == dy.shape[0], (rows, dy.shape)
        xcol = self.buf(rows, taps * C)
        ops.im2col(x.parts[0], x.p1, mode, x.n_img, x.h, x.w, info.get("frames", 0), xcol)
        tmp = self.buf(dy.shape[1], taps * C, torch.float32)
        self.full_wgrad(dy, xcol, tmp)
        self.pool.put(xcol)
        # parameter layout [N, C, k...] <- tap-major [N', taps, C']
        idx = self._idx(("conv", n, cp, C, taps), lambda: ((torch.arange(n)[:, None, None] * taps + torch.arange(taps)[None, None, :]) * C
                                                           + torch.arange(cp)[None, :, None]).reshape(-1))
        ops.gather(tmp, idx, self.fgrad(w))
        self.pool.put(tmp)
        self.full_bias_grad(b, dy)
        self.drop(*x.parts)

    def full_norm_grads(self, norm, x, dy, *, kind, silu=False, rows_per_unit=0, stats=None):
        """dgamma / dbeta of a GroupNorm (kind 0: ``x`` an Act, statistics of the forward) or LayerNorm (kind 1: ``x`` the rows)."""
        if not getattr(norm, "elementwise_affine", True) and kind == 1:
            return
        if norm.weight is None:
            return
        ops, pk = self.ops, self.pk
        x0, x1 = (x.parts[0], x.p1) if kind == 0 else (x, None)
        M, C = dy.shape
        ws = self.buf(1, max(ops.norm_affine_grad_ws_floats(M, M, C), 1), torch.float32)
        ops.norm_affine_grad(x0, x1, dy, kind=kind, sum_rows=M, ws=ws, dgamma=self.fgrad(norm.weight).view(1, C),
                             dbeta=self.fgrad(norm.bias).view(1, C), rows_per_unit=rows_per_unit,
                             groups=getattr(norm, "num_groups", 0), stats=stats, eps=getattr(norm, "eps", 0.0),
                             gamma=pk.f32(norm.weight), beta=pk.f32(norm.bias), silu=silu)
        self.pool.put(ws)

    def full_grads(self, params):
        """Gradients of ``params`` after ``backward``: views into ONE copy of the gradient arena (the engine's own buffers are overwritten by
        the next step; the copy lives as long as any of the returned tensors)."""
        plan = self._last
        if plan.get("fgrad_arena") is None:
            return [None for _ in params]
        flat = plan["fgrad_arena"].clone()
        out = []
        for p in params:
            if id(p) in plan["fgrads"]:
                o = plan["fgrad_off"][id(p)]
                out.append(flat[o:o + p.numel()].view(p.shape))
            else:
                out.append(None)
        return out
