"""Everything between an ``nn.Module`` call and a native engine call, once: the lazily built engines next to a module
(``EngineBox``), the tri-state switches (``TriState``), the autograd nodes whose backward runs on an engine (they hold the token of
the engines' tape protocol, ``_Engine._end_tape`` / ``_claim_tape``), and the declared routes of ``UNetModel`` (``ROUTES``,
``auto_route``, ``forward``).  The module files keep the reference-shaped trees, their composite forwards and thin entry points."""
import importlib
from functools import cached_property

import torch
import torch.nn as nn


# =================================================================================== engines next to a module
class EngineBox:
    """Holds a lazily built native engine next to an nn.Module without making it part of the module:
    copies / pickles of the module start with an empty box (engines own device buffers)."""

    def __init__(self):
        self.engine = None
        self.enc = None
        self.grad = None
        self.full = None
        self.input = None

    def __deepcopy__(self, memo):
        return EngineBox()

    def __reduce__(self):
        return (EngineBox, ())

    def get(self, slot, cls, owner, hook=False, setup=None):
        """The engine in ``slot``; built on first use as ``cls`` ("module.Class" of this package, imported now) over ``owner`` and a
        fresh op backend — ``HipOps``, or with ``hook`` what ``owner._native_ops_factory`` makes (tests substitute the emulated
        backend) — and handed to ``setup`` (switches, binding) before it is kept."""
        eng = getattr(self, slot)
        if eng is None:
            make_ops = getattr(owner, "_native_ops_factory", None) if hook else None
            if make_ops is None:
                from .native import HipOps as make_ops
            module, name = cls.split(".")
            eng = getattr(importlib.import_module("." + module, __package__), name)(owner, make_ops())
            if setup is not None:
                setup(eng)
            setattr(self, slot, eng)
        return eng


class TriState:
    """A switch attribute: None (the default) follows ``follow(obj)`` — an environment variable as the owner reads it; without
    ``follow`` the attribute reads None —, True / False override it for this object.  Every assignment ends in
    ``changed(obj, before)`` with the value read before it."""

    def __init__(self, doc, follow=None, changed=None):
        self.__doc__, self.follow, self.changed = doc, follow, changed

    def __set_name__(self, owner, name):
        self.key = "_" + name

    def __get__(self, obj, owner=None):
        if obj is None:
            return self
        on = obj.__dict__.get(self.key)
        return self.follow(obj) if on is None and self.follow is not None else on

    def __set__(self, obj, on):
        before = self.__get__(obj)
        obj.__dict__[self.key] = None if on is None else bool(on)
        if self.changed is not None:
            self.changed(obj, before)


def needs_grad(module, *tensors):
    """A call of ``module`` on ``tensors`` would hand autograd something to differentiate (grad mode aside)."""
    if any(t is not None and t.requires_grad for t in tensors):
        return True
    return any(p.requires_grad for p in module.parameters())


# =================================================================================== autograd nodes over the engines' tapes
def _flat_grad_buffer(eng, leaves):
    """The ``dist.FlatGradSync`` whose flat fp32 buffer's slots ARE the LoRA tensors' ``.grad`` (same order and
    offsets as ``bind_lora``), or None.  Only a buffer that announced itself (``FlatGradSync`` tags its parameters) is taken:
    writing into ``.grad`` bypasses AccumulateGrad, so a look-alike layout owned by somebody else — DDP's
    ``gradient_as_bucket_view`` bucket, accelerate's reducer — or any parameter with gradient hooks gets its gradients
    through autograd instead (the hooks then fire as usual)."""
    sync = getattr(eng.lora_params[0], "_t2v_flat_sync", None)
    if sync is None or sync.flat.dtype != torch.float32 or sync.numel != eng.lora_numel:
        return None
    base = sync.flat.data_ptr()
    for p in eng.lora_params:
        g = p.grad
        if getattr(p, "_t2v_flat_sync", None) is not sync or g is None or g.dtype != torch.float32 or not g.is_contiguous() \
                or g.data_ptr() != base + 4 * eng.lora_off[id(p)]:
            return None
        if p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
            return None
    return sync


class _NativeStudent(torch.autograd.Function):
    """UNet forward whose backward — d/d(latents), d/d(emb_all) and every token-row LoRA weight gradient — runs on the native
    gradient engine.  Inputs: latents, the conditioning branch's output (torch keeps differentiating behind it; None when the engine
    owns that branch: its LoRA tensors are among ``leaves`` then), and the LoRA tensors the engine owns (so autograd routes their
    gradients to the optimizer's ``.grad`` slots)."""

    @staticmethod
    def forward(ctx, x, emb_all, eng, args, *leaves):
        timesteps, context, fps, tc, mc = args
        y = eng.forward_tape(x.detach(), timesteps, context.detach(), fps, tc, mc, emb_all=None if emb_all is None else emb_all.detach())
        ctx.eng, ctx.token, ctx.leaves = eng, eng.tape_token, leaves
        ctx.x_dtype, ctx.e_dtype = x.dtype, None if emb_all is None else emb_all.dtype
        return y

    @staticmethod
    def _grads(ctx, dx, leaf_grads):
        d_emb = None if ctx.e_dtype is None else ctx.eng.d_emb_all.to(ctx.e_dtype).clone()
        return (dx.to(ctx.x_dtype), d_emb, None, None, *leaf_grads)

    @staticmethod
    def backward(ctx, dout):
        eng = ctx.eng
        sync = _flat_grad_buffer(eng, ctx.leaves)
        if sync is not None:
            # every LoRA tensor's .grad is already its slot of ONE flat fp32 buffer in bind_lora order (dist.FlatGradSync): the engine
            # adds its weight gradients there in one launch — what 1096 AccumulateGrad nodes would do with 1096 small kernels
            dx = eng.backward(dout, flat_grad=sync.flat, accumulate=True, grad_sync=sync, token=ctx.token)
            return _NativeStudent._grads(ctx, dx, [None] * len(ctx.leaves))
        flat = torch.empty(eng.lora_numel, dtype=torch.float32, device=dout.device)  # fresh: .grad may keep views of it
        dx = eng.backward(dout, flat_grad=flat, accumulate=False, token=ctx.token)
        offs = [eng.lora_off[id(p)] for p in ctx.leaves]
        return _NativeStudent._grads(ctx, dx, [flat[o:o + p.numel()].view_as(p).to(p.dtype) for o, p in zip(offs, ctx.leaves)])


class _NativeStudentFull(_NativeStudent):
    """UNet forward of the FULL fine-tuning student (train_latent_t2v_turbo_v2.py:669,798-816,1262: every parameter trainable, no LoRA):
    d/d(latents), d/d(emb_all) and the gradient of every parameter outside the B-row conditioning branch come from the native gradient
    engine (engine_full.py); torch keeps differentiating the conditioning branch behind ``emb_all``.  With ``native_conditioning`` on
    the engine owns that branch too: ``emb_all`` is None, the conditioning parameters are among the leaves, and the autograd graph
    behind the output is this node and the parameters' AccumulateGrad nodes."""

    @staticmethod
    def backward(ctx, dout):
        dx = ctx.eng.backward(dout, token=ctx.token)
        grads = ctx.eng.full_grads(ctx.leaves)
        return _NativeStudent._grads(ctx, dx, [None if (g is None or not p.requires_grad) else g.to(p.dtype) for p, g in zip(ctx.leaves, grads)])


class _NativeInputGrad(torch.autograd.Function):
    """UNet forward of a FROZEN network whose backward — d/d(latents) of a loss on the output and / or on the recorded temporal
    attention probabilities — runs on the data-gradient engine with nothing bound (motion_prior_sample.py:59-84:
    ``unet(latents.requires_grad_(True), ...)``, ``attn1.attention_probs``, ``autograd.grad(loss, latents)``).  Outputs: the prediction
    and one copy of every recorded probability tensor, in the engine's recording order (the route hangs them on the modules)."""

    @staticmethod
    def forward(ctx, x, eng, args):
        y = eng.forward_tape(x.detach(), *args)
        ctx.eng, ctx.token, ctx.x_dtype = eng, eng.tape_token, x.dtype
        recorded = ctx.token[0]["probs"]
        ctx.attns = [attn for attn, _ in recorded]
        ctx.set_materialize_grads(False)     # a loss on the probabilities alone leaves dout None, and the other way round
        return (y, *[probs.clone() for _, probs in recorded])

    @staticmethod
    def backward(ctx, dout, *dprobs):
        dx = ctx.eng.backward(dout, {attn: g for attn, g in zip(ctx.attns, dprobs) if g is not None}, token=ctx.token)
        return dx.to(ctx.x_dtype), None, None


class _NativeDecodeGrad(torch.autograd.Function):
    """decode(z) with a native backward: forward and dX both run on the HIP engine (engine_vae_bwd.py)."""

    @staticmethod
    def forward(ctx, z, eng):
        out = eng.decode_frames_tape(z.detach().unsqueeze(2), scale=1.0).squeeze(2)
        ctx.eng, ctx.token, ctx.z_dtype = eng, eng.tape_token, z.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return ctx.eng.backward(grad_out.unsqueeze(2), token=ctx.token).squeeze(2).to(ctx.z_dtype), None


# =================================================================================== the routes of UNetModel
_WARNED_ATEN = set()


def _warn_aten_route(why, stacklevel=3):
    """The torch composite path on a CUDA tensor is a fallback (ATen kernels, ~3x slower than the native engines): say so once
    per reason."""
    if why not in _WARNED_ATEN:
        _WARNED_ATEN.add(why)
        import warnings
        warnings.warn(f"t2v_turbo_amd UNetModel: running the torch (ATen) path on a CUDA tensor — {why}; "
                      'set native_mode = "off" to silence, see INTEGRATION.md', RuntimeWarning, stacklevel=stacklevel)


def _live_dropout(mod):
    return isinstance(mod, nn.Dropout) and mod.p > 0 and mod.training


class Call:
    """One call of a ``UNetModel`` as the routes' predicates see it.  The walks over the module tree are made on first use, once:
    none when nothing trains and nothing wants a gradient, one ``walk_modules`` (its parameters read off the same list) otherwise."""

    def __init__(self, model, x, context, timestep_cond, features_adapter=None):
        self.model, self.x, self.context, self.timestep_cond, self.features_adapter = model, x, context, timestep_cond, features_adapter

    @cached_property
    def grad(self):
        return torch.is_grad_enabled() and needs_grad(self.model, self.x, self.context, self.timestep_cond)

    @cached_property
    def mods(self):
        from .nn_util import walk_modules
        return walk_modules(self.model)

    @cached_property
    def dropping(self):
        return self.model.training and any(isinstance(mod, nn.Dropout) and mod.p > 0 for mod in self.mods)

    @cached_property
    def lora_ids(self):
        from .packs import is_lora_leaf
        return {id(w) for mod in self.mods if is_lora_leaf(mod) for w in (mod.lora_up.weight, mod.lora_down.weight)}

    @cached_property
    def params(self):
        from .nn_util import walk_parameters
        return walk_parameters(self.model, self.mods)

    @cached_property
    def any_trainable(self):
        return any(p.requires_grad for p in self.params)

    @cached_property
    def only_tconv_dropouts(self):
        """Every active Dropout(p > 0) sits in a TemporalConvBlock stage (the only ones the inference engine applies)."""
        from .unet3d import TemporalConvBlock
        known = set()
        for blk in self.mods:
            if isinstance(blk, TemporalConvBlock):
                for stg in (blk.conv1, blk.conv2, blk.conv3, blk.conv4):
                    known.update(id(layer) for layer in stg if isinstance(layer, nn.Dropout))
        return all(id(mod) in known for mod in self.mods if _live_dropout(mod))


def _has_context(c):
    return c.context is not None


def _latents_only(c):
    return not (c.context.requires_grad or (c.timestep_cond is not None and c.timestep_cond.requires_grad))


def _frozen_plain(c):
    return not c.lora_ids and not c.any_trainable


def _lora_only(c):
    return not any(p.requires_grad and id(p) not in c.lora_ids for p in c.params)


def _bind_full(model, eng):
    eng.bind_full(eng.engine_parameters(model, conditioning=eng.native_conditioning))


def _bind_lora(model, eng):
    from . import lora
    eng.bind_lora(lora.lora_parameters(model))


def _conditioning(model, eng, x, args):
    """None where the engine runs the conditioning branch itself, else that branch's output from torch (autograd stays behind it)."""
    owns = eng.owns_conditioning(x.shape[0])
    return owns, None if owns else model.conditioning_emb_all(args[0], *args[2:])


def _call_infer(model, x, args, features_adapter):
    return engine(model, "infer")(x, *args)


def _call_train(model, x, args, features_adapter):
    """Two engine instances: one whose tape the backward consumes, one for no-grad forwards in between (the distillation step's
    target forward runs between the student's forward and its backward, train_t2v_turbo_v1_lora.py:1022-1190) — separate buffers,
    same frozen weights."""
    grad = torch.is_grad_enabled()
    eng = engine(model, "train", "grad" if grad else "enc")
    owns, emb_all = _conditioning(model, eng, x, args)
    if not grad:
        return eng.forward_tape(x, *args, emb_all=emb_all)
    leaves = [p for mod in eng.engine_leaves(conditioning=owns) for p in (mod.lora_up.weight, mod.lora_down.weight)]
    return _NativeStudent.apply(x, emb_all, eng, args, *leaves)


def _call_train_full(model, x, args, features_adapter):
    eng = engine(model, "train_full")
    return _NativeStudentFull.apply(x, _conditioning(model, eng, x, args)[1], eng, args, *eng.full_params)


def _call_input_grad(model, x, args, features_adapter):
    eng = engine(model, "input_grad")
    outs = _NativeInputGrad.apply(x, eng, args)
    # what the reference reads after the call (motion_prior_sample.py:40-57) is connected to the graph: the function's own outputs
    for (attn, _), probs in zip(eng._last["probs"], outs[1:]):
        attn.attention_probs = probs
    return outs[0]


def _call_composite(model, x, args, features_adapter):
    timesteps, context, fps, timestep_cond, motion_cond = args
    return model._forward_composite(x, timesteps, context, features_adapter, fps, timestep_cond, motion_cond)


class Route:
    """``label``: how its messages name it.  ``slots``: where its engines sit in the module's ``EngineBox``; ``cls``, ``switches``
    (module attributes pushed to the engine attributes ``SWITCHES`` names, when an engine is built and whenever one is assigned) and
    ``bind`` make them.  ``requires``: (predicate over a ``Call``, exception, message of a forced mode, reason ``auto_route`` gives)
    in the order they are asked.  ``call(model, x, args, features_adapter)`` runs it."""

    def __init__(self, call, label=None, slots=(), cls="engine_unet_bwd.UNetGradEngine", switches=(), bind=None, requires=()):
        self.call, self.label, self.slots, self.cls, self.switches, self.bind, self.requires = call, label, slots, cls, switches, bind, requires

    def refusal(self, c):
        """(exception, message, reason) of the first requirement ``c`` does not meet, or None."""
        return next((rest for pred, *rest in self.requires if not pred(c)), None)


SWITCHES = {"native_checkpoint": "checkpoint_blocks", "native_conditioning": "native_conditioning"}
ROUTES = {
    "infer": Route(_call_infer, slots=("engine",), cls="engine.UNetEngine"),
    "train": Route(_call_train, 'native_mode = "train"', ("grad", "enc"), switches=("native_checkpoint", "native_conditioning"), bind=_bind_lora, requires=(
        (_has_context, ValueError, "native LoRA training needs the text context", "no text context"),
        (_lora_only, RuntimeError, 'native_mode = "train": only LoRA tensors may require grad (the base weights are frozen packs)',
         "trainable parameters besides the LoRA tensors"),
        (_latents_only, RuntimeError, 'native_mode = "train": gradients flow to the latents and the LoRA tensors only',
         "gradients w.r.t. the context / guidance embedding"))),
    "train_full": Route(_call_train_full, "native full fine-tuning", ("full",), switches=("native_checkpoint", "native_conditioning"), bind=_bind_full, requires=(
        (_has_context, ValueError, "native full fine-tuning needs the text context", None),
        (_latents_only, RuntimeError, "native full fine-tuning: gradients flow to the latents and the parameters only", None))),
    "input_grad": Route(_call_input_grad, "the native input-gradient route", ("input",), switches=("native_checkpoint",), requires=(
        (_has_context, ValueError, "the native input-gradient route needs the text context", None),
        (_frozen_plain, RuntimeError, "the native input-gradient route takes a frozen network without LoRA injection "
                                      "(trainable parameters go through the training routes)", None),
        (_latents_only, RuntimeError, "the native input-gradient route: gradients flow to the latents only", None))),
    "composite": Route(_call_composite),
}


def engine(model, route, slot=None):
    """The engine of ``route`` next to ``model`` (its first slot unless ``slot`` names another), built, switched and bound on first use.
    The test hook ``_native_ops_factory`` is honoured by the gradient engines' slots."""
    r = ROUTES[route]

    def setup(eng):
        for switch in r.switches:
            setattr(eng, SWITCHES[switch], getattr(model, switch))
        if r.bind is not None:
            r.bind(model, eng)

    return model._engine_box.get(slot or r.slots[0], r.cls, model, hook=bool(r.switches), setup=setup)


def push_switch(switch):
    """``TriState.changed`` of a module switch: hand the new value to every built engine of the routes that declare it."""
    def changed(model, before):
        for r in ROUTES.values():
            for slot in r.slots if switch in r.switches else ():
                eng = getattr(model._engine_box, slot)
                if eng is not None:
                    setattr(eng, SWITCHES[switch], getattr(model, switch))
    return changed


def auto_route(c):
    """Which engine a CUDA call lands on (``native_mode = "auto"``), as (route, reason when it is the composite path):
      * no gradient wanted, no active dropout            -> "infer": inference engine (LoRA branches merged at pack time);
      * LoRA-injected student, only LoRA tensors trainable, with or without grad, train or eval mode
        (the student and target forwards of train_t2v_turbo_v1_lora.py:1022-1028,1161-1168)
                                                         -> "train": gradient engine (un-merged LoRA branch, counter-based dropout);
      * no gradient wanted, no LoRA, train mode with only the TemporalConvBlock dropouts live (the v1 teacher, which the
        reference never puts in eval mode)               -> "infer": inference engine + counter-based dropout masks;
      * no LoRA, gradients wanted and at least one parameter trainable — FULL fine-tuning, the student of
        train_latent_t2v_turbo_v2.py:669,798-816,1262 (train mode with the TemporalConvBlock dropouts live, or eval)
                                                         -> "train_full": gradient engine with base-weight gradients (engine_full.py);
      * no LoRA, NO parameter trainable, gradients wanted w.r.t. the latents only, no live dropout, and ``native_input_grad`` on —
        the motion-prior score of motion_prior_sample.py:59-84 and preprocess_with_motion_prior.py:246,360 (frozen eval-mode
        network, ``latents.requires_grad_(True)``, a loss on the recorded ``attention_probs`` and / or the output)
                                                         -> "input_grad": data-gradient engine with nothing bound (opt-in);
      * anything else (gradients w.r.t. the context, input gradients of a frozen network with ``native_input_grad`` off or left in
        train mode, adapters, other live dropouts)       -> the torch composite path, with a one-time warning."""
    m = c.model
    if c.features_adapter is not None:
        if not c.grad and not c.dropping:
            raise NotImplementedError("features_adapter is not used by t2v-turbo and not supported natively")
        return "composite", "features_adapter"
    if not c.grad and not c.dropping:
        return "infer", None
    if not c.grad and not c.lora_ids and c.only_tconv_dropouts:
        # a frozen, LoRA-free network left in train mode under no_grad: the v1 distillation teacher as the reference runs it
        # (train_t2v_turbo_v1_lora.py:621-626 never calls .eval(); forwards at :1105-1134) — inference dataflow + the
        # TemporalConvBlock dropouts as counter-based masks
        return "infer", None
    if not c.lora_ids:
        if (c.grad and c.x.requires_grad and m.input_grad_route_on() and ROUTES["input_grad"].refusal(c) is None
                and not any(_live_dropout(mod) for mod in c.mods)):
            return "input_grad", None
        if (c.grad and m.native_full and c.any_trainable and ROUTES["train_full"].refusal(c) is None
                and (not m.training or c.only_tconv_dropouts)):
            return "train_full", None
        return "composite", ("a train-mode network with active Dropout and no LoRA" if not c.grad else
                             "gradients without LoRA injection that the native full fine-tuning route does not take (input gradients only, "
                             "gradients w.r.t. the context, other live dropouts, T2V_NATIVE_FULL=0)")
    for pred, _, _, why in ROUTES["train"].requires:
        if not pred(c) and (c.grad or pred is not _latents_only):    # (a no-grad call is not asked where gradients would flow)
            return "composite", why
    return "train", None


def forward(model, x, timesteps, context, features_adapter, fps, timestep_cond, motion_cond):
    """``UNetModel.forward``: resolve the route — forced by ``native_mode`` = "train" / "input_grad", by ``auto_route`` for a CUDA
    tensor, else the composite path —, raise where a native route cannot run, and call it."""
    mode = getattr(model, "native_mode", "auto")
    c = Call(model, x, context, timestep_cond, features_adapter)
    route, why = "composite", None
    if mode == "train":  # force the native gradient engine (raises where it cannot run)
        route = "train_full" if torch.is_grad_enabled() and not c.lora_ids and c.any_trainable else "train"
    elif mode == "input_grad" and torch.is_grad_enabled() and x.requires_grad:
        route = "input_grad"    # forced as well; a call that asks for no gradient is answered as in "auto"
    elif mode != "off" and x.is_cuda:  # "off": always the torch path
        route, why = auto_route(c)
    r = ROUTES[route]
    if r.requires:
        if not (x.is_cuda or getattr(model, "_native_ops_factory", None) is not None):
            raise RuntimeError(f"{r.label} needs CUDA tensors")
        refusal = r.refusal(c)
        if refusal is not None:
            raise refusal[0](refusal[1])
    if why is not None:
        _warn_aten_route(why, stacklevel=4)
    return r.call(model, x, (timesteps, context, fps, timestep_cond, motion_cond), features_adapter)
