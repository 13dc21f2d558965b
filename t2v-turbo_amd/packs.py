"""Leaf parameters in the layouts the kernels read.  A ``Packer`` caches one entry per pack, and every entry DECLARES how it is re-made
(``Pack``): full fine-tuning re-fills all packs in place after each optimizer step, because the recorded launch lists and the captured
refresh graph hold raw pointers into them."""
import operator
import os

import torch
import torch.nn as nn

from . import native as nt


def is_lora_leaf(mod):
    """A LoraInjected{Linear,Conv2d,Conv3d} (utils/lora.py:19-230) by its children — dictionary lookups, not ``getattr``: a missing
    attribute on an nn.Module costs an exception, and this runs over every module of the UNet on every training-path call."""
    d = mod._modules
    return "lora_up" in d and "lora_down" in d and (d.get("linear") is not None or d.get("conv") is not None)


def effective_weight_bias(mod, merge=True):
    """(weight, bias) of a Linear/Conv leaf; LoRA-injected leaves (utils/lora.py:19-230 layout:
    .linear|.conv, .lora_down, .lora_up, .scale[, .selector]) are merged on the fly:
    W + scale * up @ diag(sel) @ down — what ``collapse_lora`` (utils/lora.py:793-830) would bake in.
    ``merge=False`` (the training engine, which runs the LoRA branch as its own GEMMs): the frozen base only."""
    base = getattr(mod, "linear", None) or getattr(mod, "conv", None)
    if base is not None and hasattr(mod, "lora_up") and hasattr(mod, "lora_down"):
        if not merge:
            return base.weight.detach(), base.bias
        w = base.weight.detach().float()
        up = mod.lora_up.weight.detach().float().flatten(1)
        down = mod.lora_down.weight.detach().float().flatten(1)
        sel = getattr(mod, "selector", None)
        if isinstance(sel, (nn.Linear, nn.Conv2d, nn.Conv3d)):
            up = up @ sel.weight.detach().float().flatten(1)
        delta = (up @ down).reshape(w.shape)
        return w + float(mod.scale) * delta, base.bias
    return mod.weight.detach(), mod.bias


def leaf_out_channels(mod):
    """Output channels of a Linear / Conv leaf (a LoRA-injected leaf has its frozen base's) without merging anything."""
    base = getattr(mod, "linear", None) or getattr(mod, "conv", None)
    if base is not None and hasattr(mod, "lora_up") and hasattr(mod, "lora_down"):
        return base.weight.shape[0]
    return mod.weight.shape[0]


def params_fingerprint(module, skip=()):
    """Changes when any parameter is updated in place (version counter), re-homed (data pointer), added or removed."""
    from .nn_util import walk_parameters
    fp = 0
    for p in walk_parameters(module):
        if id(p) not in skip:
            fp = (fp * 1000003 + p._version + (p.data_ptr() & 0xFFFFFFF)) & 0xFFFFFFFFFFFF
    return fp


def params_fingerprints(module, skip=()):
    """``params_fingerprint`` split in two: (structure, version).  Structure: which parameters there are, where they live (data
    pointer), their shape and dtype — a re-homed, replaced, added or removed parameter and ``.to(dtype)`` change it, and whatever holds
    raw pointers to packs made from the parameters has to be made again.  Version: the version counters — an in-place update
    (an optimizer step, an EMA, ``load_state_dict``) moves only this one, and re-filling the packs in place is enough.
    Runs on every engine call: the tree is walked straight off the ``_modules`` / ``_parameters`` dicts and the five attributes are
    read by C-level ``map``s, which keeps the pair no dearer than the single fingerprint was (~ 1.7 ms of host time for the UNet's
    1 485 parameters)."""
    ps, stack = [], [module]
    while stack:
        mod = stack.pop()
        if mod is not None:
            ps.extend(mod._parameters.values())
            stack.extend(mod._modules.values())
    ps = [p for p in ps if p is not None and id(p) not in skip] if skip else [p for p in ps if p is not None]
    sfp = hash((tuple(map(id, ps)), tuple(map(_data_ptr, ps)), tuple(map(_size, ps)), tuple(map(_dtype, ps))))
    return sfp, hash(tuple(map(_version, ps)))


_data_ptr, _size = torch.Tensor.data_ptr, torch.Tensor.size
_dtype, _version = operator.attrgetter("dtype"), operator.attrgetter("_version")


def _tensors(v):
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, (tuple, list)):
        for e in v:
            yield from _tensors(e)


def _geglu_rows(v):
    """Rows [value | gate] -> 64-row groups [32 value rows | 32 gate rows] (T2V_ACT_GEGLU)."""
    inner = v.shape[0] // 2
    assert inner % 32 == 0
    return torch.cat([v[:inner].reshape(inner // 32, 32, -1), v[inner:].reshape(inner // 32, 32, -1)], dim=1).reshape(2 * inner, -1)


def _put(old, new):
    for o, n in zip(_tensors(old), _tensors(new)):
        if o.data_ptr() != n.data_ptr():
            o.copy_(n)


class Pack:
    """One cache entry.  ``make()`` builds ``value`` (a tensor or a tuple of tensors) from the current parameters and sources;
    ``into(value, ops)``, where given, re-fills the existing tensors in place instead of copying a fresh ``make()`` into them; ``src``: keys
    of the entries this one is derived from (refreshed first; empty: made from parameters); ``param``: the parameter the pack may BE (an
    fp32 parameter on the device is its own pack: nothing to re-make while that holds); ``static``: no weights inside, never re-made."""
    __slots__ = ("key", "value", "make", "into", "src", "param", "static")

    def __init__(self, key, value, make, into, src, param, static):
        self.key, self.value, self.make, self.into, self.src, self.param, self.static = key, value, make, into, src, param, static


class Packer:
    """Packs leaf parameters into kernel layouts; cached until any parameter changes."""

    def __init__(self, wdtype, device, merge_lora=True):
        self.wdtype, self.device, self.merge_lora = wdtype, device, merge_lora
        self._entries = {}   # key -> Pack, in creation order
        self._where = {}     # id(tensor of an entry) -> (key, index in a tuple value or None); the entries keep them alive: the ids are stable

    def __len__(self):
        return len(self._entries)

    def __iter__(self):
        return iter(self._entries)

    def __getitem__(self, key):
        return self._entries[key]

    def wb(self, mod):
        return effective_weight_bias(mod, self.merge_lora)

    def pack(self, key, make, *, src=(), into=None, param=None, static=False):
        """The value of entry ``key``, made and registered at the first request (see ``Pack``)."""
        e = self._entries.get(key)
        if e is None:
            e = self._entries[key] = Pack(key, make(), make, into, tuple(src), param, static)
            for i, t in [(None, e.value)] if isinstance(e.value, torch.Tensor) else enumerate(e.value):
                self._where.setdefault(id(t), (key, i))
        return e.value

    def pointers(self):
        """Device pointer of every pack tensor, in creation order (part of the captured refresh's signature)."""
        return tuple(t.data_ptr() for e in self._entries.values() for t in _tensors(e.value))

    def refresh(self, ops=None):
        """Re-make every pack from the CURRENT parameters into the tensors that are already there (full fine-tuning: the weights move
        every optimizer step, the recorded launch lists keep pointing at the same packs).  Depth first over ``src``, each entry once: a
        derived pack sees its refreshed sources whatever the order they were created in.  ``ops``: the op backend, for the packs the
        library re-makes itself (transposes of a refreshed pack, conv packs).
        (Measured and not kept: the backward-only packs issued behind the forward's launches — 139.1 / 135.9 vs 139.8 / 135.2 ms per
        step, profiles/r06_full_finetune_wgrad_affine_rework_ab.jsonl.)"""
        done = set()

        def visit(e):
            if e is None or e.key in done:     # (None: a declared source that was never made)
                return
            done.add(e.key)
            for k in e.src:
                visit(self._entries.get(k))
            if e.static or (e.param is not None and isinstance(e.value, torch.Tensor) and e.param.data_ptr() == e.value.data_ptr()):
                return
            if e.into is not None:
                e.into(e.value, ops)
            else:
                _put(e.value, e.make())
        for e in list(self._entries.values()):
            visit(e)

    def _source(self, w, method):
        if id(w) not in self._where:
            raise ValueError(f"Packer.{method}: the tensor is not a pack of this Packer (only cached packs have a stable identity)")
        return self._where[id(w)]

    def f32(self, p):
        return None if p is None else self.pack(("f32", id(p)), lambda: p.detach().to(self.device, torch.float32).contiguous(), param=p)

    def bias(self, mod):
        b = self.wb(mod)[1]
        return None if b is None else self.pack(("bias", id(mod)), lambda: b.detach().to(self.device, torch.float32).contiguous(), param=b)

    def cat_biases(self, mods, tag):
        return self.pack((tag,) + tuple(id(m) for m in mods), lambda: torch.cat([self.bias(m) for m in mods]).contiguous(),
                         src=[("bias", id(m)) for m in mods])

    def _w2(self, mod):
        return self.wb(mod)[0].detach().flatten(1)

    def mat(self, mod):
        """[N, K] row-major weight of a Linear / 1x1 conv / k=1 Conv1d.  Refresh: ONE cast-and-copy kernel from the parameter into the pack
        (no cast into a temporary plus a device-to-device copy: 1 100 of the 1 500 packs of the full-width UNet are this or ``mat_t``)."""
        # (``param``: in the weight dtype on the device the pack IS the parameter's storage — an in-place copy onto itself would only move
        # the parameter's version counter, and whoever watches that would refresh again after every refresh)
        return self.pack(("mat", id(mod)), lambda: self._w2(mod).to(self.device, self.wdtype).contiguous(),
                         into=lambda out, ops: out.copy_(self._w2(mod)), param=None if is_lora_leaf(mod) else mod.weight)

    def mat_t(self, mod):
        """[K, N]^T pack of a Linear / 1x1 conv: the weight of its data gradient (dx = dy @ W)."""
        def into(out, ops):
            src = self._entries.get(("mat", id(mod)))      # (present: refreshed before this entry)
            if (src is not None and hasattr(ops, "transpose") and src.value.dtype == out.dtype
                    and (out.dtype == torch.bfloat16 or not out.is_cuda)):   # (the library's transpose is bf16; the emulated backend takes any)
                # bf16 -> bf16 by the library's tiled transpose (the strided fp32 -> bf16 copy: ~ 300 GB/s, 30 us per pack, 7 ms per step)
                ops.transpose(src.value, src.value.shape[0], src.value.shape[1], out)
            else:
                out.copy_(self._w2(mod).t())
        return self.pack(("mat_t", id(mod)), lambda: self._w2(mod).t().to(self.device, self.wdtype).contiguous(),
                         src=[("mat", id(mod))], into=into)

    # ---- conv packs: [rows, -1] of a permuted view of the parameter; kind 0 forward, 1 data gradient (t2v_repack_conv_f32's kinds) ----
    @staticmethod
    def _tap_major(w):
        return w[:, :, :, 0, 0].permute(0, 2, 1) if w.dim() == 5 else w.permute(0, 2, 3, 1)

    def _conv_pack(self, key, mod, kind, view):
        def make(out=None, ops=None):
            w = self.wb(mod)[0]
            if not self._repacked(w, out, ops, kind):
                out = self._permuted_into(view(w), out)
            return out
        return self.pack(key, make, into=make)

    def conv(self, mod):
        """[N, taps*Cin], tap-major: Conv2d [N,C,3,3] -> (ky,kx,c); Conv3d [N,C,3,1,1] -> (kt,c)."""
        return self._conv_pack(("conv", id(mod)), mod, 0, self._tap_major)

    def conv_dgrad(self, mod):
        """3x3 conv data gradient as a 3x3 conv over dy: w'[ci][(ky',kx'), co] = w[co][ci][2-ky'][2-kx']."""
        return self._conv_pack(("conv_dgrad", id(mod)), mod, 1, lambda w: w.flip(2, 3).permute(1, 2, 3, 0))

    def tconv_dgrad(self, mod):
        """(3,1,1) conv data gradient as the same temporal conv over dy: w'[ci][(kt', co)] = w[co][ci][2 - kt']."""
        return self._conv_pack(("tconv_dgrad", id(mod)), mod, 1, lambda w: w[:, :, :, 0, 0].flip(2).permute(1, 2, 0))

    @staticmethod
    def _repacked(w, out, ops, kind):
        """``refresh`` on the device: the conv parameter -> its existing bf16 pack by the library's repack kernel (t2v_repack_conv_f32).
        False where that does not apply (first making, CPU tensors, a merged LoRA weight)."""
        if out is None or ops is None or not hasattr(ops, "repack_conv") or w.dtype != torch.float32 or not w.is_contiguous():
            return False
        if os.environ.get("T2V_REPACK_NATIVE", "1") != "1":     # (A/B switch: torch's permute / flip / cast chain)
            return False
        if w.dim() == 5 and (w.shape[3] != 1 or w.shape[4] != 1):
            return False
        n, c = w.shape[0], w.shape[1]
        taps = w.numel() // (n * c)
        if taps > 9 or tuple(out.shape) != ((n, taps * c) if kind == 0 else (c, taps * n)) or not out.is_contiguous():
            return False
        if out.is_cuda and out.dtype != torch.bfloat16:
            return False
        ops.repack_conv(w, out, kind)
        return True

    def _permuted_into(self, w, out=None):
        """The [rows, -1] pack of the permuted weight view ``w`` — into ``out`` where that is the existing pack (``refresh``: cast and
        permutation as ONE kernel straight into the pack, no temporary and no second copy)."""
        if out is not None and tuple(out.shape) == (w.shape[0], w[0].numel()) and out.is_contiguous():
            out.view(w.shape).copy_(w)
            return out
        return w.reshape(w.shape[0], -1).to(self.device, self.wdtype).contiguous()

    def conv_slab(self, mod):
        """Slab-major pack of a 3x3 conv for t2v_conv_halo: [N][C/32][9][32], rows zero-padded to whole weight stages (native.pack_conv_slab).
        From the tap-major entry where there is one, else from the parameter (no tap-major copy is left behind for a conv the halo kernel takes)."""
        def make():
            e = self._entries.get(("conv", id(mod)))
            return nt.pack_conv_slab(e.value if e is not None else self._permuted_into(self._tap_major(self.wb(mod)[0])))
        return self.pack(("conv_slab", id(mod)), make, src=[("conv", id(mod))])

    def conv_slab_of(self, w):
        """Slab-major pack of a tap-major pack this Packer made (the data-gradient convs' flipped weights), keyed by that entry.  A pack that
        is rewritten every step from outside, like the LoRA groups', is no entry and is refused."""
        key, i = self._source(w, "conv_slab_of")
        return self.pack(("conv_slab_of", key, i), lambda: nt.pack_conv_slab(w), src=[key])

    def lpr(self, w):
        """Fragment pack (native.pack_linear_pr) of an [N, K] pack this Packer made — a plain ``mat`` / ``cat_mats`` matrix or the 64-row
        [value | gate] interleave of ``geglu`` — for t2v_linear_pr; keyed by the source entry, which keeps ``w`` alive."""
        key, i = self._source(w, "lpr")
        return self.pack(("lpr", key, i), lambda: nt.pack_linear_pr(w), src=[key])

    def cat_mats(self, mods, tag):
        return self.pack((tag,) + tuple(id(m) for m in mods), lambda: torch.cat([self.mat(m) for m in mods], dim=0).contiguous(),
                         src=[("mat", id(m)) for m in mods])

    def mats_t(self, mods, tag):
        """Transposed pack of row-concatenated Linear weights: [K, sum N] (dx = d[y0|y1|..] @ cat(W))."""
        return self.pack((tag,) + tuple(id(m) for m in mods), lambda: self.cat_mats(mods, tag + "_fwd").t().contiguous(),
                         src=[(tag + "_fwd",) + tuple(id(m) for m in mods)])

    def geglu(self, proj):
        """GEGLU projection packed in 64-row groups [32 value rows | 32 gate rows] (T2V_ACT_GEGLU)."""
        def make():
            w, b = self.wb(proj)
            return (_geglu_rows(w).to(self.device, self.wdtype).contiguous(),
                    _geglu_rows(b[:, None]).reshape(-1).detach().to(self.device, torch.float32).contiguous())
        return self.pack(("geglu", id(proj)), make)

    def geglu_t(self, proj):
        """The ``geglu`` weight pack transposed: the data gradient of the GEGLU projection in its packed row order."""
        return self.pack(("geglu_t", id(proj)), lambda: self.geglu(proj)[0].t().contiguous(), src=[("geglu", id(proj))])

    def mat_lnf(self, mods, norm, tag):
        """LayerNorm folded into the Linear(s) that consume it (t2v_gemm lnf_*): (W' = cat(W) diag(gamma) in the weight dtype,
        s = row sums of the ROUNDED W' (fp32: what the matrix cores multiply the mean with), t = b + cat(W) beta (fp32))."""
        def make():
            w = torch.cat([self.wb(m)[0].detach().float().reshape(self.wb(m)[0].shape[0], -1) for m in mods], dim=0).to(self.device)
            # (no bias: zeros made ON the device — a host tensor copied up would keep the pack refresh out of a hipGraph)
            b = torch.cat([(self.wb(m)[1].detach().float().to(self.device) if self.wb(m)[1] is not None
                            else torch.zeros(self.wb(m)[0].shape[0], device=self.device)) for m in mods])
            gamma, beta = norm.weight.detach().float().to(self.device), norm.bias.detach().float().to(self.device)
            wp = (w * gamma[None, :]).to(self.wdtype).contiguous()
            return wp, wp.float().sum(dim=1).contiguous(), (b + w @ beta).contiguous()
        return self.pack((tag, id(norm)) + tuple(id(m) for m in mods), make)

    def geglu_lnf(self, proj, norm):
        """``geglu`` pack (64-row groups [32 value | 32 gate]) of the LayerNorm-folded GEGLU projection: (W', s, t)."""
        def make():
            wp, s_vec, t_vec = self.mat_lnf([proj], norm, "geglu_lnf_src")
            return (_geglu_rows(wp).contiguous(), _geglu_rows(s_vec[:, None]).reshape(-1).contiguous(),
                    _geglu_rows(t_vec[:, None]).reshape(-1).contiguous())
        return self.pack(("geglu_lnf", id(proj), id(norm)), make, src=[("geglu_lnf_src", id(norm), id(proj))])

    def ffn(self, ff, norm):
        """Packed operands of t2v_ffn_fused for FeedForward ``ff`` (GEGLU projection + output Linear) behind LayerNorm ``norm``."""
        def make():
            proj, lin = ff.net[0].proj, ff.net[2]
            (w1, b1), (w2, b2) = self.wb(proj), self.wb(lin)
            dev = self.device
            return nt.ffn_pack(w1.detach().to(dev), None if b1 is None else b1.detach().to(dev), w2.detach().to(dev),
                               None if b2 is None else b2.detach().to(dev), norm.weight.detach().to(dev), norm.bias.detach().to(dev),
                               self.wdtype)
        return self.pack(("ffn", id(ff), id(norm)), make)

    def _small_pack(self, key, mod, view, cin_pad, cout_pad=None):
        def make():
            w = view(self.wb(mod)[0].float())
            if cin_pad and cin_pad > w.shape[-1]:
                w = torch.nn.functional.pad(w, (0, cin_pad - w.shape[-1]))
            if cout_pad and cout_pad > w.shape[0]:
                w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, cout_pad - w.shape[0]))
            return w.reshape(w.shape[0], -1).to(self.device).contiguous()
        return self.pack(key, make)

    def small_conv(self, mod, cin_pad=None):
        """fp32 [cout][9][cin] for the direct small-Cin conv."""
        return self._small_pack(("small", id(mod), cin_pad), mod, lambda w: w.permute(0, 2, 3, 1), cin_pad)

    def small_conv_dgrad(self, mod, cin_pad, cout_pad=None):
        """fp32 [cout'][9][cin'] pack for the direct small-channel conv computing the data gradient of ``mod`` ([ci, ky', kx', co]):
        cout' = mod's input channels (optionally zero-padded rows), cin' = mod's output channels padded to cin_pad."""
        return self._small_pack(("small_dgrad", id(mod), cin_pad, cout_pad), mod, lambda w: w.flip(2, 3).permute(1, 2, 3, 0), cin_pad, cout_pad)
