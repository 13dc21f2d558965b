"""The Packer (t2v_turbo_amd/packs.py) on tiny modules, shared by tests/test_packs_cpu.py and tests/test_gpu_packs.py: one builder per pack
kind the class offers, the creation orders they are built in (sources first, dependants first, reversed), an in-place move of every
parameter, and the comparison of a refreshed Packer with a fresh one over the moved parameters."""
import types

import torch
import torch.nn as nn

from t2v_turbo_amd.engine import Packer


def modules(device="cpu"):
    """Linear(64, 128) x 2 (a q | k group), Conv2d(64, 80, 3), Conv3d(64, 64, (3,1,1)), a GEGLU Linear(64, 128) with its LayerNorm(64), a
    Conv2d(4, 64, 3) for the small-channel packs, and the two Linears of a 64-channel FeedForward for the fused-FFN pack."""
    torch.manual_seed(7)
    ff = types.SimpleNamespace(net=[types.SimpleNamespace(proj=nn.Linear(64, 512)), None, nn.Linear(256, 64)])
    m = types.SimpleNamespace(lin=nn.Linear(64, 128), lin2=nn.Linear(64, 128), conv=nn.Conv2d(64, 80, 3, padding=1),
                              tconv=nn.Conv3d(64, 64, (3, 1, 1), padding=(1, 0, 0)), proj=nn.Linear(64, 128), norm=nn.LayerNorm(64),
                              small=nn.Conv2d(4, 64, 3, padding=1), ff=ff)
    m.all = [m.lin, m.lin2, m.conv, m.tconv, m.proj, m.norm, m.small, ff.net[0].proj, ff.net[2]]
    with torch.no_grad():
        m.norm.weight.add_(torch.randn(64) * 0.2)
        m.norm.bias.add_(torch.randn(64) * 0.2)
    for mod in m.all:
        mod.to(device)
    return m


def move(m, seed=5):
    """An optimizer-style step: every parameter moves in place, by far more than a bf16 rounding step."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.all:
            for p in mod.parameters():
                p.add_((torch.randn(p.shape, generator=gen) * 0.1).to(p.device))


BUILD = {
    "f32": lambda pk, m: (pk.f32(m.norm.weight), pk.f32(m.norm.bias)),
    "bias": lambda pk, m: pk.bias(m.lin),
    "mat": lambda pk, m: pk.mat(m.lin),
    "cat_mats": lambda pk, m: pk.cat_mats([m.lin, m.lin2], "qk"),
    "conv": lambda pk, m: pk.conv(m.conv),
    "tconv": lambda pk, m: pk.conv(m.tconv),
    "conv_dgrad": lambda pk, m: pk.conv_dgrad(m.conv),
    "tconv_dgrad": lambda pk, m: pk.tconv_dgrad(m.tconv),
    "geglu": lambda pk, m: pk.geglu(m.proj),
    "mat_lnf": lambda pk, m: pk.mat_lnf([m.lin, m.lin2], m.norm, "qk_lnf"),
    "ffn": lambda pk, m: pk.ffn(m.ff, m.norm),
    "small_conv": lambda pk, m: pk.small_conv(m.small, cin_pad=8),
    "small_conv_dgrad": lambda pk, m: pk.small_conv_dgrad(m.small, 64, 8),
    "static": lambda pk, m: pk.pack(("table", 5), lambda: torch.arange(5, device=pk.device), static=True),
    # ---- derived entries
    "mat_t": lambda pk, m: pk.mat_t(m.lin),
    "conv_slab": lambda pk, m: pk.conv_slab(m.conv),
    "conv_slab_of": lambda pk, m: pk.conv_slab_of(pk.conv_dgrad(m.small)),      # ([4, 9 * 64]: the data-gradient conv's frozen-pack form)
    "lpr_mat": lambda pk, m: pk.lpr(pk.mat(m.lin)),
    "lpr_cat": lambda pk, m: pk.lpr(pk.cat_mats([m.lin, m.lin2], "qk")),
    "lpr_geglu": lambda pk, m: pk.lpr(pk.geglu(m.proj)[0]),
    "mats_t": lambda pk, m: pk.mats_t([m.lin, m.lin2], "qk_t"),
    "geglu_t": lambda pk, m: pk.geglu_t(m.proj),
    "geglu_lnf": lambda pk, m: pk.geglu_lnf(m.proj, m.norm),
    "cat_biases": lambda pk, m: pk.cat_biases([m.lin, m.lin2], "b_all"),
    "caller_derived": lambda pk, m: pk.pack(("head", id(m.conv)), lambda: pk.conv_dgrad(m.conv)[:4].contiguous(),
                                            src=[("conv_dgrad", id(m.conv))]),
}
_DERIVED = list(BUILD)[list(BUILD).index("mat_t"):]
ORDERS = {
    "sources_first": list(BUILD),
    # the slab before the tap-major pack, mat_t before mat, mats_t / the fragment packs before an explicit request of their sources
    "dependants_first": _DERIVED + [k for k in BUILD if k not in _DERIVED],
    "reversed": list(BUILD)[::-1],
}


def build(pk, m, order):
    for name in ORDERS[order]:
        BUILD[name](pk, m)
    return pk


def tensors(v):
    return [v] if isinstance(v, torch.Tensor) else list(v)


def record_refresh(pk, ops):
    """Run ``pk.refresh(ops)`` -> the keys of the entries it re-made, in the order their ``into`` / ``make`` ran."""
    log = []

    def logged(fn, key):
        def run(*a, **k):
            log.append(key)
            return fn(*a, **k)
        return run
    for key in pk:
        e = pk[key]
        e.make = logged(e.make, key)
        if e.into is not None:
            e.into = logged(e.into, key)
    pk.refresh(ops)
    return log


def check_refresh_equals_fresh(device, wdtype, ops, order):
    m = modules(device)
    pk = build(Packer(wdtype, device), m, order)
    keys, ptrs = list(pk), pk.pointers()
    before = {k: [t.clone() for t in tensors(pk[k].value)] for k in pk}
    move(m)
    pk.refresh(ops)
    assert list(pk) == keys and pk.pointers() == ptrs, "a refresh re-fills the tensors that are there: no entry and no address changes"
    fresh = build(Packer(wdtype, device), m, "sources_first")
    assert set(fresh) == set(keys)
    for k in keys:
        got, want = tensors(pk[k].value), tensors(fresh[k].value)
        assert len(got) == len(want), k
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (order, k)
        assert pk[k].static or any(not torch.equal(a, o) for a, o in zip(got, before[k])), ("the move did not reach this pack", k)
