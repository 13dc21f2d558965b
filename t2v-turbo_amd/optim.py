"""The optimizer side of a training step.  ``FlatAdamW`` keeps the LoRA tensors, their gradients (``dist.FlatGradSync``) and the moments
each in ONE contiguous fp32 buffer: a step is one fused kernel (``t2v_adamw_step``) with the clip coefficient of ``clip_grad_norm_``
(train_t2v_turbo_v1_lora.py:1193) folded in, ``update_ema_flat`` its EMA.  Everything else leaves the tensors where the trainer put them
and walks a device table of them in one launch: ``AdamW8bit`` (``t2v_adamw8_step``: the ``bnb.optim.AdamW8bit`` of ``--use_8bit_adam``,
moments block-wise in 8 bits, served as ``bitsandbytes.optim.AdamW8bit`` by ``compat.install()``), ``AdamW`` (``t2v_adamw_multi``:
``torch.optim.AdamW``'s constructor, state and checkpoints), ``clip_grad_norm_`` / ``grad_clip_coef`` (``t2v_sumsq_multi``,
``t2v_scale_multi``: norm and coefficient stay on the device) and ``update_ema`` (``t2v_ema_multi``).  These four share ONE table path,
the section below: the record layouts are the ctypes classes of ``native.py`` (``record_dtype``), ``work_blocks`` gives every tensor its
first work block, ``ema_table`` / ``adamw8_table`` / ``adamw_table`` fill the records, ``upload`` puts them on the device, ``_Recent`` keeps
the plans of the last few tensor lists, ``touch`` tells the engines that a kernel wrote parameters.  CPU tensors: the same arithmetic in torch."""
import contextlib
import operator

import numpy as np
import torch

from . import native as nt
from .native import shared_ops, shared_ops as _shared_ops   # (``_shared_ops``: its name while it lived here)

QBLOCK = nt.ADAMW8_BLOCK       # elements per quantisation block (T2V_ADAMW8_BLOCK)
MAX_HYPER = nt.ADAMW_MAX_HYPER  # T2V_ADAMW_MAX_HYPER

# ------------------------------------------------------------------------------------------------ descriptor tables
_T = torch.Tensor
_dtype_of, _is_cuda = operator.attrgetter("dtype"), operator.attrgetter("is_cuda")


def record_dtype(struct):
    """The numpy record dtype of a ctypes ``Structure`` of ``native.py``: its field names, offsets and size, pointers as ``<u8``."""
    return np.dtype(struct)


def work_blocks(numel, block):
    """-> (work0 of every tensor, total): each tensor takes ceil(numel / block) work blocks of one launch, in order."""
    blocks = (np.asarray(numel, dtype=np.int64) + (block - 1)) // block
    return np.cumsum(blocks) - blocks, int(blocks.sum())


def _ptrs(tensors):
    return np.fromiter(map(_T.data_ptr, tensors), dtype=np.uint64, count=len(tensors))


def _numels(tensors):
    return np.fromiter(map(_T.numel, tensors), dtype=np.int64, count=len(tensors))


def ema_table(targets, sources):
    """The ``t2v_ema_tensor`` records of the pairs, in order -> (numpy record array, work blocks of the launch)."""
    host = np.zeros(len(targets), dtype=record_dtype(nt.EmaTensor))
    host["target"], host["src"], host["n"] = _ptrs(targets), _ptrs(sources), _numels(targets)
    host["work0"], work = work_blocks(host["n"], nt.EMA_BLOCK)
    host["src_dt"] = [nt.BF16 if s.dtype == torch.bfloat16 else nt.F32 for s in sources]
    return host, work


def adamw8_table(params, grads, state_blocks, f32_state, lr=0.0, weight_decay=0.0, launch_of=None):
    """The ``t2v_adamw8_tensor`` records of the tensors, in order -> (numpy record array, launches).  ``state_blocks``: every tensor's
    first block in its state arena; ``f32_state``: fp32 moments? (one value or one per tensor, as ``lr`` and ``weight_decay``);
    ``launch_of``: its launch, non-decreasing (None: one).  ``launches``: ``(first record, end record, work blocks)`` each."""
    n = len(params)
    host = np.zeros(n, dtype=record_dtype(nt.Adamw8Tensor))
    host["param"], host["grad"], host["state_block"], host["n"] = _ptrs(params), _ptrs(grads), state_blocks, _numels(params)
    host["lr"], host["weight_decay"] = lr, weight_decay
    host["flags"] = np.where(f32_state, nt.ADAMW8_F32_STATE, 0)
    launch_of = np.zeros(n, dtype=np.int64) if launch_of is None else np.asarray(launch_of, dtype=np.int64)
    assert n > 0 and bool((launch_of[1:] >= launch_of[:-1]).all())
    bounds = [0] + [int(i) + 1 for i in np.flatnonzero(launch_of[1:] != launch_of[:-1])] + [n]
    launches = []
    for start, end in zip(bounds[:-1], bounds[1:]):
        host["work0"][start:end], work = work_blocks(host["n"][start:end], QBLOCK)
        launches.append((start, end, work))
    return host, launches


def adamw_table(grads, params=None, exp_avgs=None, exp_avg_sqs=None, rows=None):
    """The ``t2v_adamw_tensor`` records of the tensors, in order -> (numpy record array, launches).  ``rows``: the hyper row of every
    tensor, non-decreasing (None: all 0).  A launch takes at most ``MAX_HYPER`` distinct rows: ``launches`` is a list of
    ``(first record, end record, work blocks, first row, rows)``; ``work0`` counts from the launch's first record and ``hyper`` from
    its first row.  Gradients only (``t2v_sumsq_multi`` / ``t2v_scale_multi`` read nothing else): leave the other lists out."""
    n = len(grads)
    host = np.zeros(n, dtype=record_dtype(nt.AdamwTensor))
    host["grad"], host["n"] = _ptrs(grads), _numels(grads)
    for field, lst in (("param", params), ("exp_avg", exp_avgs), ("exp_avg_sq", exp_avg_sqs)):
        if lst is not None:
            host[field] = _ptrs(lst)
    rows = np.zeros(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    assert n > 0 and bool((host["n"] > 0).all()) and bool((rows[1:] >= rows[:-1]).all())
    launches, start = [], 0
    while start < n:
        end = int(np.searchsorted(rows, rows[start] + MAX_HYPER, side="left"))
        host["work0"][start:end], work = work_blocks(host["n"][start:end], nt.ADAMW_BLOCK)
        host["hyper"][start:end] = rows[start:end] - rows[start]
        launches.append((start, end, work, int(rows[start]), int(rows[end - 1] - rows[start]) + 1))
        start = end
    return host, launches


def upload(host, dev, out=None):
    """A record array -> uint8 tensor on ``dev`` (``out``, if given: the table it replaces, of the same size); to a GPU through pinned
    memory, so that the host never waits.  Returns (device tensor, what has to stay alive while the copy may still be reading it)."""
    src = torch.from_numpy(host.view(np.uint8))
    if dev.type != "cuda":
        return (src.clone() if out is None else out.copy_(src)), None
    pinned = src.pin_memory()
    table = torch.empty(host.nbytes, dtype=torch.uint8, device=dev) if out is None else out
    with torch.cuda.device(dev):
        table.copy_(pinned, non_blocking=True)
    return table, pinned


class _Recent(dict):
    """The plans of the few most recently used keys, most recently used last."""
    capacity = 4

    def lookup(self, key, build):
        """The plan of ``key``, made by ``build()`` if it is not here; a ``build()`` that returns None leaves nothing behind."""
        plan = self.pop(key, None)
        if plan is None:
            plan = build()
        if plan is not None:
            self[key] = plan
            while len(self) > self.capacity:
                del self[next(iter(self))]
        return plan


def touch(tensors):
    """The kernels write through raw pointers, behind torch's back: move the version counters of ``tensors`` — no launch — so that
    ``packs.params_fingerprint`` changes and the engines that packed these weights re-fill their packs instead of running on the old ones."""
    torch.autograd.graph.increment_version(tensors)


class FlatAdamW:
    def __init__(self, params, grad_sync, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        self.params = [p for p in params if p.requires_grad]
        self.sync = grad_sync
        assert sum(p.numel() for p in self.params) == grad_sync.numel
        assert len(self.params) == len(grad_sync.params) and all(a is b for a, b in zip(self.params, grad_sync.params)), \
            "FlatAdamW and FlatGradSync must be built from the same parameter list, in the same order"
        dev = self.params[0].device
        self.flat_param = torch.empty(grad_sync.numel, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in self.params:  # parameters become views of the flat buffer
                self.flat_param[off:off + p.numel()].copy_(p.detach().reshape(-1))
                p.data = self.flat_param[off:off + p.numel()].view_as(p)
                off += p.numel()
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.step_count = 0
        self._ops = None
        self._ws = None
        self.after_step_hooks = []   # callables run after every step (engines that cache operand packs of the parameters)

    def _hip(self):
        if self._ops is None:
            self._ops = shared_ops()
            self._ws = torch.empty(1025, dtype=torch.float32, device=self.flat_param.device)
        return self._ops

    @torch.no_grad()
    def grad_norm(self):
        g = self.sync.flat
        if g.is_cuda:
            ops = self._hip()
            ops.sumsq(g, self._ws[:1024], self._ws[1024:])
            return self._ws[1024].sqrt()
        return g.norm(2)

    @torch.no_grad()
    def step(self, max_grad_norm=None):
        """One AdamW step on the (already all-reduced) flat gradient; returns the pre-clip gradient norm."""
        self.step_count += 1
        g = self.sync.flat
        norm = self.grad_norm() if max_grad_norm is not None else None
        scale = 1.0
        if max_grad_norm is not None:
            scale = float(torch.clamp(max_grad_norm / (norm + 1e-6), max=1.0))
        b1, b2 = self.betas
        if g.is_cuda:
            self._hip().adamw_step(self.flat_param, g, self.exp_avg, self.exp_avg_sq, self.lr, b1, b2, self.eps,
                                   self.weight_decay, self.step_count, scale)
        else:
            gr = g * scale
            self.flat_param.mul_(1 - self.lr * self.weight_decay)
            self.exp_avg.mul_(b1).add_(gr, alpha=1 - b1)
            self.exp_avg_sq.mul_(b2).addcmul_(gr, gr, value=1 - b2)
            bc1, bc2 = 1 - b1 ** self.step_count, 1 - b2 ** self.step_count
            self.flat_param.addcdiv_(self.exp_avg, self.exp_avg_sq.sqrt() / bc2 ** 0.5 + self.eps, value=-self.lr / bc1)
        # The parameters are ``.data`` views of flat_param: neither the kernel nor an in-place op on the flat buffer moves THEIR
        # version counters, which the engines key their packed (LoRA-merged) weights on.
        touch(self.params[0])
        for hook in self.after_step_hooks:   # e.g. UNetGradEngine.invalidate_lora_packs (engine_lora.py)
            hook()
        return norm

    def zero_grad(self):
        self.sync.zero_()


@torch.no_grad()
def update_ema_flat(target_flat, source_flat, rate=0.99, target_params=None):
    """EMA of a flat fp32 parameter buffer (utils/common_utils.py:307-319) in one kernel.  ``target_params``: the target
    network's parameters if they are ``.data`` views of ``target_flat`` — one of their version counters is moved so that the
    native engines re-pack the target's weights (see FlatAdamW.step)."""
    if target_flat.is_cuda:
        shared_ops().ema_update(target_flat, source_flat, rate)
    else:
        target_flat.mul_(rate).add_(source_flat, alpha=1 - rate)
    if target_params:
        touch(target_params[0])


# ------------------------------------------------------------------------------------------------ EMA of a module tree
_EMA_TABLES = _Recent()      # key -> cached device table (a target / student pair keeps one)


def _ema_key(targets, sources):
    """What the cached plan of an update depends on: per tensor of both lists the data pointer, the element count, the dtype and
    whether it is contiguous (device pointers are unique across the GPUs of a process, so they name the device too).  Read by C-level
    ``map``s: this runs every step, and a Python loop over the 2 x 1 485 tensors of a UNet costs as much host time as the launch takes
    on the device."""
    return tuple(tuple(map(f, lst)) for lst in (targets, sources) for f in (_T.data_ptr, _T.numel, _dtype_of, _T.is_contiguous))


def _ema_plan(targets, sources):
    """Sort the pairs — the ones ONE t2v_ema_multi launch takes (fp32 contiguous target, fp32 / bf16 contiguous source of the same size,
    all on one GPU) and the rest — and ``upload`` the launch's table, kept until a tensor is re-homed, resized or cast (``_ema_key``)."""
    native, rest, dev = [], [], None
    for i, (t, s) in enumerate(zip(targets, sources)):
        ok = (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and s.device == t.device and s.is_contiguous()
              and s.dtype in (torch.float32, torch.bfloat16) and s.numel() == t.numel() and t.numel() > 0
              and (dev is None or t.device == dev))
        if ok:
            dev = t.device
        (native if ok else rest).append(i)
    plan = dict(native=native, rest=rest, dev=dev)
    if native:
        host, work = ema_table([targets[i] for i in native], [sources[i] for i in native])
        table, pinned = upload(host, dev)
        plan.update(table=table, pinned=pinned, work=work)   # (``pinned`` is kept: the copy may still be reading it)
    return plan


@torch.no_grad()
def update_ema(target_params, source_params, rate=0.99):
    """``update_ema`` of the reference (utils/common_utils.py:307-319; train_latent_t2v_turbo_v2.py:1272-1276 calls it after every
    optimizer step with the target's and the student's ``parameters()``): targ = targ * rate + src * (1 - rate), the parameters left
    where they are.  Pairs on the GPU with an fp32 contiguous target and an fp32 / bf16 contiguous source go into ONE
    ``t2v_ema_multi`` launch; every other pair (CPU tensors, an fp16 target, a non-contiguous tensor) takes the torch expression."""
    targets, sources = list(target_params), list(source_params)
    n = min(len(targets), len(sources))
    targets, sources = targets[:n], sources[:n]
    if not any(map(_is_cuda, targets)):
        for t, s in zip(targets, sources):
            t.detach().mul_(rate).add_(s.to(t.dtype), alpha=1 - rate)
        return
    plan = _EMA_TABLES.lookup(_ema_key(targets, sources), lambda: _ema_plan(targets, sources))
    for i in plan["rest"]:
        t, s = targets[i], sources[i]
        t.detach().mul_(rate).add_(s.to(t.dtype), alpha=1 - rate)
    if plan["native"]:
        with torch.cuda.device(plan["dev"]):
            shared_ops().ema_multi(plan["table"], len(plan["native"]), plan["work"], float(rate))
        touch(targets[plan["native"][0]])


# ------------------------------------------------------------------------------------------------ block-wise 8-bit AdamW

def _dynamic_levels(top, decades):
    """Values in (0, 1), denser toward 0: decade d = 0, 1, ... covers [10^-(d+1), 10^-d] with ``top >> d`` evenly spaced values
    (the centres of that many equal cells) — a decade exponent and a linear fraction whose resolution halves per decade, the
    'dynamic' data type of Dettmers et al. 2021."""
    out = []
    for d in range(decades):
        k = top >> d
        edges = np.linspace(0.1, 1.0, k + 1)
        out += list(0.5 * (edges[:-1] + edges[1:]) * 10.0 ** -d)
    return out


def make_code_books():
    """(signed, unsigned): two tables of 256 strictly increasing fp32 values.  Signed (first moment): -1, 126 negative levels over
    6 decades, 0, 127 positive levels over 7 decades, 1.  Unsigned (second moment): 0, 254 levels over 7 decades, 1.  These are this
    project's OWN tables: they follow the published layout, not bitsandbytes' arrays, which are not available to compare with."""
    signed = [-1.0] + [-x for x in _dynamic_levels(64, 6)] + [0.0] + _dynamic_levels(64, 7) + [1.0]
    unsigned = [0.0] + _dynamic_levels(128, 7) + [1.0]
    books = []
    for vals in (signed, unsigned):
        t = torch.tensor(sorted(vals), dtype=torch.float64).to(torch.float32)
        assert t.numel() == 256 and bool((t[1:] > t[:-1]).all())
        books.append(t)
    return books[0], books[1]


def _midpoints(code):
    return (code[:-1] + code[1:]) * 0.5   # fp32, as the kernel forms them


def quantize_blockwise(x, code):
    """fp32 tensor -> (codes uint8 [ceil(n / 256) * 256], absmax fp32 [ceil(n / 256)]): per block of 256 consecutive elements,
    absmax = max |x| and code = index of the table value nearest to x / absmax (a value exactly between two codes takes the
    lower one; an all-zero block has absmax 0 and the code of 0).  The padding of a last, partial block holds the code of 0."""
    x = x.detach().reshape(-1).float()
    n = x.numel()
    nb = (n + QBLOCK - 1) // QBLOCK
    if x.is_cuda:
        codes = torch.empty(nb * QBLOCK, dtype=torch.uint8, device=x.device)
        absmax = torch.empty(nb, dtype=torch.float32, device=x.device)
        shared_ops().quant8(x.contiguous(), code.to(x.device), codes, absmax)
        return codes, absmax
    xp = torch.zeros(nb * QBLOCK, dtype=torch.float32)
    xp[:n] = x
    xp = xp.view(nb, QBLOCK)
    absmax = xp.abs().amax(dim=1)
    xn = torch.where(absmax[:, None] > 0, xp / absmax[:, None], torch.zeros_like(xp))
    codes = torch.bucketize(xn, _midpoints(code))   # number of midpoints strictly below the value
    return codes.to(torch.uint8).reshape(-1), absmax


def dequantize_blockwise(codes, absmax, code, n):
    """The inverse map: value = code[byte] * absmax[block], the first ``n`` elements."""
    if codes.is_cuda:
        out = torch.empty(n, dtype=torch.float32, device=codes.device)
        shared_ops().dequant8(codes, absmax, code.to(codes.device), out)
        return out
    nb = (n + QBLOCK - 1) // QBLOCK
    return (code[codes[:nb * QBLOCK].long()].view(nb, QBLOCK) * absmax[:nb, None]).reshape(-1)[:n]


def adamw_definition(pf, grad, m, v, lr, betas, eps, wd, step, scale):
    """One AdamW step on flat fp32 tensors in the kernels' operation order, every product and sum rounded separately (the device
    kernels are compiled without fused multiply-adds so that both agree bit for bit on the moments): ``pf`` is updated in place from
    the fresh moments, which are returned ``(m, v)``.  The scalars are formed in fp32 as t2v_adamw8_step / t2v_adamw_multi form them."""
    f32 = np.float32
    b1, b2, lr, wd, eps, scale = f32(betas[0]), f32(betas[1]), f32(lr), f32(wd), f32(eps), f32(scale)
    bc1 = f32(1) - np.power(b1, f32(step), dtype=f32)
    bc2_sqrt = np.sqrt(f32(1) - np.power(b2, f32(step), dtype=f32), dtype=f32)
    decay, step_size = f32(1) - lr * wd, lr / bc1
    gr = grad * float(scale)
    pf.mul_(float(decay))
    m = m * float(b1) + gr * float(f32(1) - b1)
    v = v * float(b2) + (gr * float(f32(1) - b2)) * gr
    pf.sub_((m * float(step_size)) / (v.sqrt() / float(bc2_sqrt) + float(eps)))
    return m, v


class AdamW8bit(torch.optim.Optimizer):
    """AdamW (``torch.optim.AdamW`` semantics: decoupled decay, bias correction) whose two moments are stored in 8 bits, block-wise:
    one byte per element indexing a 256-entry code book, one fp32 absmax per 256 consecutive elements of a tensor (Dettmers et
    al. 2021).  Constructor surface of ``bitsandbytes.optim.AdamW8bit`` as far as the reference's trainers use it
    (train_latent_t2v_turbo_v2.py:833-845: two groups, the second with its own ``lr``).  Tensors with fewer than
    ``min_8bit_size`` elements keep fp32 moments.  Parameters and gradients are not moved: on the GPU one ``t2v_adamw8_step``
    launch walks a device table of every tensor that has a gradient (one launch per distinct ``(betas, eps, step)`` among them);
    on CPU tensors the same arithmetic runs in torch, block for block.

    The code books are this project's own (``make_code_books``).  bitsandbytes is CUDA-only and was not available to compare
    with: neither its tables nor its saved optimizer state are bit-compatible with this class, and no such claim is made.
    ``load_state_dict`` takes this class's own state or a ``torch.optim.AdamW`` state (whose fp32 moments it quantises).
    Not implemented (``NotImplementedError`` when asked for): paged state, percentile clipping, ``block_wise=False``, amsgrad."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, optim_bits=32, args=None,
                 min_8bit_size=4096, percentile_clipping=100, block_wise=True, is_paged=False):
        if amsgrad or optim_bits != 32 or args is not None or percentile_clipping != 100 or not block_wise or is_paged:
            raise NotImplementedError("AdamW8bit: amsgrad / optim_bits / args / percentile_clipping / block_wise=False / is_paged "
                                      "are accepted at their bitsandbytes defaults only")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("AdamW8bit: invalid lr / betas / eps / weight_decay")
        self.min_8bit_size = int(min_8bit_size)
        self.code1, self.code2 = make_code_books()
        self._zero1, self._zero2 = int((self.code1 == 0).nonzero()), int((self.code2 == 0).nonzero())
        self._layout = {}            # parameter -> (8-bit?, first block in its arena, blocks)
        self._arena = None           # dict: s1, s2 (uint8), a1, a2 (fp32 absmax), f1, f2 (fp32 moments of the small tensors)
        self._books = {}             # device -> (code1, code2) there
        self._table = None           # cached descriptor table of the device path
        self.native_ops = None       # a HipOps to run the kernel with; None: the process-wide one for GPU tensors, torch on CPU tensors
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    # -- state arenas ------------------------------------------------------------------------------------------------------
    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _ensure_state(self):
        """Give every parameter its slice of the arenas (append-only: a parameter group added later keeps the others' offsets)."""
        new = [p for p in self._all_params() if p not in self._layout]
        if not new:
            return
        dev = self._all_params()[0].device
        used8 = sum(nb for is8, _, nb in self._layout.values() if is8)
        used32 = sum(nb for is8, _, nb in self._layout.values() if not is8)
        for p in new:
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous() or p.is_sparse:
                raise ValueError("AdamW8bit: parameters must be dense contiguous fp32 tensors on one device")
            nb = (p.numel() + QBLOCK - 1) // QBLOCK
            is8 = p.numel() >= self.min_8bit_size
            self._layout[p] = (is8, used8 if is8 else used32, nb)
            used8, used32 = used8 + (nb if is8 else 0), used32 + (0 if is8 else nb)
        old = self._arena
        a = dict(s1=torch.full((used8 * QBLOCK,), self._zero1, dtype=torch.uint8, device=dev),
                 s2=torch.full((used8 * QBLOCK,), self._zero2, dtype=torch.uint8, device=dev),
                 a1=torch.zeros(used8, device=dev), a2=torch.zeros(used8, device=dev),
                 f1=torch.zeros(used32 * QBLOCK, device=dev), f2=torch.zeros(used32 * QBLOCK, device=dev))
        if old is not None:
            for k in a:
                a[k][:old[k].numel()].copy_(old[k])
        self._arena, self._table = a, None
        for p, (is8, b0, nb) in self._layout.items():   # the per-parameter state: views of the arenas
            st = self.state[p]
            st.setdefault("step", 0)
            if is8:
                st["state1"], st["state2"] = a["s1"][b0 * QBLOCK:(b0 + nb) * QBLOCK], a["s2"][b0 * QBLOCK:(b0 + nb) * QBLOCK]
                st["absmax1"], st["absmax2"] = a["a1"][b0:b0 + nb], a["a2"][b0:b0 + nb]
            else:
                st["state1"] = a["f1"][b0 * QBLOCK:b0 * QBLOCK + p.numel()]
                st["state2"] = a["f2"][b0 * QBLOCK:b0 * QBLOCK + p.numel()]

    def _codes_on(self, dev):
        if dev not in self._books:
            self._books[dev] = (self.code1.to(dev), self.code2.to(dev))
        return self._books[dev]

    def state_bytes(self):
        """Bytes of optimizer state (codes + absmax + the fp32 moments of the small tensors)."""
        self._ensure_state()
        return sum(t.numel() * t.element_size() for t in self._arena.values())

    def moments(self, p):
        """The two moments of one parameter as fp32 tensors (dequantised copies)."""
        self._ensure_state()
        st, (is8, _, _) = self.state[p], self._layout[p]
        if not is8:
            return st["state1"].clone().view_as(p), st["state2"].clone().view_as(p)
        c1, c2 = self._codes_on(p.device)
        return (dequantize_blockwise(st["state1"], st["absmax1"], c1, p.numel()).view_as(p),
                dequantize_blockwise(st["state2"], st["absmax2"], c2, p.numel()).view_as(p))

    def set_moments(self, p, exp_avg, exp_avg_sq, step=None):
        """Overwrite one parameter's moments from fp32 tensors (quantised here unless the parameter keeps fp32 state)."""
        self._ensure_state()
        st, (is8, _, _) = self.state[p], self._layout[p]
        if step is not None:
            st["step"] = int(step)
        m, v = exp_avg.detach().to(p.device, torch.float32).reshape(-1), exp_avg_sq.detach().to(p.device, torch.float32).reshape(-1)
        self._store(st, is8, m, v, *self._codes_on(p.device))

    @staticmethod
    def _store(st, is8, m, v, code1, code2):
        """Fresh fp32 moments into a parameter's state: quantised block by block, or as they are where the state is fp32."""
        for key, amk, x, code in (("state1", "absmax1", m, code1), ("state2", "absmax2", v, code2)):
            if is8:
                x, absmax = quantize_blockwise(x, code)
                st[amk].copy_(absmax)
            st[key].copy_(x)

    # -- the step ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """One AdamW step over every parameter that has a gradient; ``grad_scale`` multiplies the gradients first (a clip
        coefficient).  ``param_groups[i]["lr"]`` is read now, so a scheduler may drive it."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._ensure_state()
        active = []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.device != p.device:
                    raise ValueError("AdamW8bit: gradients must be dense contiguous fp32 tensors on the parameter's device")
                self.state[p]["step"] += 1
                active.append((gi, p))
        if not active:
            return loss
        if active[0][1].is_cuda or self.native_ops is not None:
            self._step_hip(active, float(grad_scale))
        else:
            for gi, p in active:
                g = self.param_groups[gi]
                self._step_cpu(p, g["lr"], g["betas"], g["eps"], g["weight_decay"], float(grad_scale))
        touch(active[0][1])
        return loss

    def _step_cpu(self, p, lr, betas, eps, wd, scale):
        """The definition, vectorised over one tensor: dequantise, AdamW in fp32 with every product and sum rounded separately
        (the device kernel is compiled without fused multiply-adds so that both agree bit for bit on the moments), update the
        parameter from the fresh moments, re-quantise block by block."""
        st, (is8, _, _) = self.state[p], self._layout[p]
        n, step = p.numel(), st["step"]
        if is8:
            m = dequantize_blockwise(st["state1"], st["absmax1"], self.code1, n)
            v = dequantize_blockwise(st["state2"], st["absmax2"], self.code2, n)
        else:
            m, v = st["state1"], st["state2"]
        m, v = adamw_definition(p.view(-1), p.grad.reshape(-1), m, v, lr, betas, eps, wd, step, scale)
        self._store(st, is8, m, v, self.code1, self.code2)

    def _step_hip(self, active, grad_scale):
        groups = self.param_groups
        # one launch per distinct (betas, eps, step); the signature decides whether the cached table still describes this step
        step0 = self.state[active[0][1]]["step"]
        keys = [(groups[gi]["betas"][0], groups[gi]["betas"][1], groups[gi]["eps"], self.state[p]["step"] - step0) for gi, p in active]
        sig = tuple((p.data_ptr(), p.grad.data_ptr(), k) for (gi, p), k in zip(active, keys))
        if self._table is None or self._table["sig"] != sig:
            order = sorted(range(len(active)), key=lambda i: keys[i])   # stable: parameters keep their order inside a launch
            ps = [active[i][1] for i in order]
            layout = [self._layout[p] for p in ps]
            launch_of = np.cumsum([j > 0 and keys[i] != keys[order[j - 1]] for j, i in enumerate(order)])
            host, launches = adamw8_table(ps, [p.grad for p in ps], [b0 for _, b0, _ in layout], [not is8 for is8, _, _ in layout],
                                          launch_of=launch_of)
            self._table = dict(sig=sig, host=host, launches=[(s, e, work, keys[order[s]]) for s, e, work in launches],
                               group=np.array([active[i][0] for i in order]), dev=None, pinned=None, uploaded=None)
        t = self._table
        t["host"]["lr"] = np.array([g["lr"] for g in groups], dtype=np.float32)[t["group"]]
        t["host"]["weight_decay"] = np.array([g["weight_decay"] for g in groups], dtype=np.float32)[t["group"]]
        image = t["host"].tobytes()
        if t["uploaded"] != image:   # lr moves every scheduler step: 56 bytes per tensor, into the table that is there
            t["dev"], t["pinned"] = upload(t["host"], active[0][1].device, out=t["dev"])   # (``pinned`` is kept: the copy may still be reading it)
            t["uploaded"] = image
        a = self._arena
        c1, c2 = self._codes_on(t["dev"].device)
        ops = self.native_ops if self.native_ops is not None else shared_ops()
        opt = lambda x: x if x.numel() else None
        with torch.cuda.device(t["dev"].device) if t["dev"].is_cuda else contextlib.nullcontext():
            for start, end, work, (b1, b2, eps, dstep) in t["launches"]:
                ops.adamw8_step(t["dev"][start * t["host"].itemsize:], end - start, work, opt(a["s1"]), opt(a["s2"]), opt(a["a1"]),
                                opt(a["a2"]), opt(a["f1"]), opt(a["f2"]), c1, c2, b1, b2, eps, step0 + dstep, grad_scale)

    # -- checkpoints ---------------------------------------------------------------------------------------------------------
    def state_dict(self):
        self._ensure_state()
        sd = super().state_dict()
        for s in sd["state"].values():   # own copies: a pickled view would drag the whole arena along, once per tensor
            for k, v in s.items():
                if torch.is_tensor(v):
                    s[k] = v.clone()
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """This class's own state (codes, absmax, step per parameter) or a ``torch.optim.AdamW`` state (``exp_avg`` /
        ``exp_avg_sq`` are quantised block-wise; small tensors keep them in fp32)."""
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups) or any(len(s["params"]) != len(g["params"]) for s, g in zip(saved, self.param_groups)):
            raise ValueError("AdamW8bit.load_state_dict: the parameter groups do not match")
        id_map = {}
        for s, g in zip(saved, self.param_groups):
            id_map.update(zip(s["params"], g["params"]))
            g.update({k: v for k, v in s.items() if k != "params"})
        self._ensure_state()
        for pid, s in state_dict["state"].items():
            p = id_map[pid]
            st, (is8, _, _) = self.state[p], self._layout[p]
            if "exp_avg" in s:
                self.set_moments(p, s["exp_avg"], s["exp_avg_sq"], step=int(s["step"]))
                continue
            if is8 != ("absmax1" in s) or s["state1"].numel() != st["state1"].numel():
                raise ValueError("AdamW8bit.load_state_dict: saved state of another layout (min_8bit_size changed?)")
            st["step"] = int(s["step"])
            for k in ("state1", "state2") + (("absmax1", "absmax2") if is8 else ()):
                st[k].copy_(s[k].to(st[k].dtype))


# ------------------------------------------------------------------------------------------------ fp32 AdamW and clipping, in place
def _check_dense_f32(what, tensors, dev):
    for t in tensors:
        if t.is_sparse or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{what}: parameters and gradients must be dense contiguous fp32 tensors on one device")


class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` — its constructor, its per-parameter state (``step`` a 0-d fp32 CPU tensor, ``exp_avg``, ``exp_avg_sq``),
    its checkpoints in both directions — whose step on the GPU is ONE ``t2v_adamw_multi`` launch over a device table of every tensor
    that has a gradient, parameters, gradients and moments left where they are (one launch per 16 distinct ``(group, step)`` rows).
    The table is uploaded again only when one of its pointers moves; the learning rates travel with the launch.  ``foreach`` and
    ``fused`` are accepted and ignored; ``amsgrad`` / ``maximize`` / ``capturable`` / ``differentiable`` at their defaults only.  CPU
    tensors run the same arithmetic in torch (``adamw_definition``), one tensor at a time.

    ``step(grad_scale=...)`` multiplies the gradients first, without writing them: a float, or a one-element fp32 tensor on the
    parameters' device — the coefficient of ``grad_clip_coef``, which then never visits the host."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        if amsgrad or maximize or capturable or differentiable:
            raise NotImplementedError("AdamW: amsgrad / maximize / capturable / differentiable are accepted at their defaults only")
        if torch.is_tensor(lr) and lr.numel() != 1:
            raise ValueError("AdamW: a tensor lr must have one element")
        if float(lr) < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("AdamW: invalid lr / betas / eps / weight_decay")
        self._plan = None            # cached descriptor table of the device path
        self.table_uploads = 0       # how often a table went to the device (test hook)
        self.native_ops = None       # a HipOps to run the kernel with; None: the process-wide one for GPU tensors, torch on CPU tensors
        super().__init__(params, dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=foreach, capturable=False, differentiable=False, fused=fused,
                                      decoupled_weight_decay=True))

    def add_param_group(self, param_group):
        if any(param_group.get(k) for k in ("amsgrad", "maximize", "capturable", "differentiable")):
            raise NotImplementedError("AdamW: amsgrad / maximize / capturable / differentiable are accepted at their defaults only")
        super().add_param_group(param_group)
        self._plan = None

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plan = None

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """This class's own checkpoints and ``torch.optim.AdamW``'s (any of its foreach / fused forms: a ``step`` saved on a device comes
        to the host here, once)."""
        if any(g.get(k) for g in state_dict["param_groups"] for k in ("amsgrad", "maximize", "capturable", "differentiable")):
            raise NotImplementedError("AdamW.load_state_dict: amsgrad / maximize / capturable / differentiable checkpoints")
        super().load_state_dict(state_dict)
        for s in self.state.values():
            if "step" in s:
                step = s["step"]
                s["step"] = step.detach().to("cpu", torch.float32).reshape(()) if torch.is_tensor(step) else torch.tensor(float(step))
        self._plan = None

    @staticmethod
    def _new_state(p, s):
        s["step"] = torch.tensor(0.0, dtype=torch.float32)
        s["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """One AdamW step over every parameter that has a gradient (only their ``step`` advances).  ``param_groups[i]["lr"]`` is read
        now, so a scheduler may drive it."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        active = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not active:
            return loss
        dev = active[0].device
        if dev.type != "cuda" and self.native_ops is None:
            self._step_torch(float(grad_scale))
            return loss
        grads = [p.grad for p in active]
        states = list(map(self.state.__getitem__, active))
        if not all(states):   # the first gradient of a parameter
            _check_dense_f32("AdamW", active, dev)
            for p, s in zip(active, states):
                if not s:
                    self._new_state(p, s)
        ms, vs = [s["exp_avg"] for s in states], [s["exp_avg_sq"] for s in states]
        key = tuple(tuple(map(_T.data_ptr, lst)) for lst in (active, grads, ms, vs))
        plan = self._plan
        if plan is None or plan["key"] != key or float(plan["steps"][0]) != plan["first_step"] + plan["uses"]:
            plan = self._plan = self._make_plan(active, grads, states, ms, vs, key, dev)
        plan["steps"].add_(1.0)   # every state[p]["step"] of this plan is a 0-d view of this one buffer
        plan["uses"] += 1
        groups = self.param_groups
        rows = [(float(groups[gi]["lr"]), groups[gi]["weight_decay"], groups[gi]["betas"][0], groups[gi]["betas"][1], groups[gi]["eps"],
                 step0 + plan["uses"]) for gi, step0 in plan["rows"]]
        scale, scale_dev = (1.0, grad_scale.detach()) if torch.is_tensor(grad_scale) else (float(grad_scale), None)
        if scale_dev is not None and (scale_dev.device != dev or scale_dev.dtype != torch.float32 or scale_dev.numel() != 1):
            raise ValueError("AdamW.step: a tensor grad_scale must be one fp32 element on the parameters' device")
        ops = self.native_ops if self.native_ops is not None else shared_ops()
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            for start, end, work, row0, n_rows in plan["launches"]:
                hyper = (nt.AdamwHyper * n_rows)(*[nt.AdamwHyper(*r) for r in rows[row0:row0 + n_rows]])
                ops.adamw_multi(plan["table"][start * nt.C.sizeof(nt.AdamwTensor):], end - start, work, hyper, scale, scale_dev)
        touch(active)   # every updated parameter: the fingerprint changes whichever module a parameter belongs to
        return loss

    def _make_plan(self, active, grads, states, ms, vs, key, dev):
        """Sort the tensors by hyper row — one row per (group, step) among them — and put the descriptor table on the device."""
        for lst in (active, grads, ms, vs):
            _check_dense_f32("AdamW", lst, dev)
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
        # The step counts of the plan's tensors move into ONE fp32 CPU buffer and every state[p]["step"] becomes a 0-d view of it (still
        # torch's layout: a 0-d fp32 CPU tensor per parameter): a step then advances all of them with one add instead of one per tensor.
        steps = [int(s["step"]) for s in states]
        step_buf = torch.tensor(steps, dtype=torch.float32)
        for i, s in enumerate(states):
            s["step"] = step_buf[i]
        row_keys = [(group_of[id(p)], st) for p, st in zip(active, steps)]
        uniq = sorted(set(row_keys))
        index = {k: i for i, k in enumerate(uniq)}
        order = sorted(range(len(active)), key=lambda i: index[row_keys[i]])   # stable: parameters keep their order inside a row
        pick = lambda lst: [lst[i] for i in order]   # noqa: E731
        host, launches = adamw_table(pick(grads), pick(active), pick(ms), pick(vs), [index[row_keys[i]] for i in order])
        table, pinned = upload(host, dev)
        self.table_uploads += 1
        return dict(key=key, table=table, pinned=pinned, launches=launches, rows=uniq, steps=step_buf, first_step=steps[0], uses=0)

    def _step_torch(self, grad_scale):
        """The definition in torch, one tensor at a time, in the kernel's operation order."""
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                _check_dense_f32("AdamW", (p, p.grad), p.device)
                s = self.state[p]
                if not s:
                    self._new_state(p, s)
                s["step"] += 1
                m, v = adamw_definition(p.view(-1), p.grad.reshape(-1), s["exp_avg"].view(-1), s["exp_avg_sq"].view(-1), float(g["lr"]),
                                        g["betas"], g["eps"], g["weight_decay"], int(s["step"]), grad_scale)
                s["exp_avg"].view(-1).copy_(m)
                s["exp_avg_sq"].view(-1).copy_(v)


_CLIP_PLANS = _Recent()      # key -> cached device table and workspace


def _clip_plan(parameters):
    """The plan of one norm launch over the gradients of ``parameters`` -> (plan, parameter list); plan None: this call is torch's
    (a gradient that is not a dense contiguous fp32 CUDA tensor, more than one device, or no gradient at all)."""
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    grads = [p.grad for p in params if p.grad is not None]
    if not grads or not all(map(_is_cuda, grads)):
        return None, params
    key = (tuple(map(_T.data_ptr, grads)), tuple(map(_T.numel, grads)), tuple(map(_dtype_of, grads)), tuple(map(_T.is_contiguous, grads)))

    def build():
        dev = grads[0].device
        if any(g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev or g.numel() == 0 for g in grads):
            return None
        host, launches = adamw_table(grads)
        (_, n, work, _, _), = launches
        table, pinned = upload(host, dev)
        return dict(table=table, pinned=pinned, n=n, work=work, dev=dev, ws=torch.empty(work, dtype=torch.float32, device=dev))

    return _CLIP_PLANS.lookup(key, build), params


def _norm_and_coef(plan, max_norm):
    out = torch.empty(2, dtype=torch.float32, device=plan["dev"])   # a buffer of its own: what is returned outlives the next call
    with torch.cuda.device(plan["dev"]):
        shared_ops().sumsq_multi(plan["table"], plan["n"], plan["work"], plan["ws"], float(max_norm), out)
    return out


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_``.  When every gradient present is a dense contiguous fp32 tensor on one GPU and ``norm_type``
    is 2: one ``t2v_sumsq_multi`` (the norm and the coefficient min(1, max_norm / (norm + 1e-6)), left on the device) and one
    ``t2v_scale_multi`` over a cached table of the gradients, no host synchronisation.  Any other call is torch's function, whole.
    Returns the total norm, a 0-d fp32 tensor on the gradients' device."""
    plan, params = _clip_plan(parameters) if float(norm_type) == 2.0 else (None, parameters)
    if plan is None:
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    out = _norm_and_coef(plan, max_norm)
    if error_if_nonfinite and not bool(torch.isfinite(out[0])):   # (the one read of the norm)
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be "
                           "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`")
    with torch.cuda.device(plan["dev"]):
        shared_ops().scale_multi(plan["table"], plan["n"], plan["work"], out[1:])
    return out[0]


@torch.no_grad()
def grad_clip_coef(parameters, max_norm):
    """(total norm, clip coefficient) of the gradients of ``parameters``: two 0-d views of one device buffer, nothing scaled.
    ``AdamW.step(grad_scale=coef)`` then clips inside the optimizer pass, and the scaled gradients are never written.  Gradients that
    ``clip_grad_norm_`` would hand to torch get torch's norm and the same coefficient expression."""
    plan, params = _clip_plan(parameters)
    if plan is not None:
        out = _norm_and_coef(plan, max_norm)
        return out[0], out[1]
    grads = [p.grad for p in params if p.grad is not None]
    norm = torch.nn.utils.get_total_norm(grads, 2.0) if grads else torch.tensor(0.0)
    out = torch.stack([norm.float(), torch.clamp(max_norm / (norm.float() + 1e-6), max=1.0)])
    return out[0], out[1]
