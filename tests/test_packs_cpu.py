"""Unit tests of the Packer (t2v_turbo_amd/packs.py) on tiny modules: what full fine-tuning relies on every optimizer step — a refresh
re-fills every pack in place with the bytes a fresh Packer would make, sources before the packs derived from them whatever order they
were created in — and what keeps the cache honest: derived packs are keyed by their source ENTRY, so a tensor that is not one is refused."""
import pytest
import torch

from t2v_turbo_amd import native as nt
from t2v_turbo_amd.engine import Packer
from tests.emu_ops import EmuOps
from tests.packs_cases import ORDERS, build, check_refresh_equals_fresh, modules, move, record_refresh


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("backend", [None, EmuOps], ids=["no_ops", "emu_ops"])
@pytest.mark.parametrize("wdtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_refresh_equals_a_fresh_packer(wdtype, backend, order):
    """Every pack kind, every parameter moved in place, ``refresh``: each entry equals a new Packer's over the moved parameters and no
    tensor's address changed.  (``dependants_first`` builds the slab-major pack before the tap-major one it is made from: with the
    first-made-order refresh this left the slab one step stale.)"""
    check_refresh_equals_fresh("cpu", wdtype, None if backend is None else backend(), order)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("backend", [None, EmuOps], ids=["no_ops", "emu_ops"])
def test_refresh_runs_sources_before_dependants(backend, order):
    m = modules()
    pk = build(Packer(torch.bfloat16, "cpu"), m, order)
    move(m)
    log = record_refresh(pk, None if backend is None else backend())
    assert len(log) == len(set(log)), "an entry is re-made once per refresh"
    at = {k: i for i, k in enumerate(log)}
    pairs = [(s, k) for k in pk for s in pk[k].src if s in at and k in at]
    # every derived kind of the class is in the set, each with its source present (but the concatenated biases: their sources ARE the
    # fp32 parameters here, which a refresh skips)
    assert {k[0] for _, k in pairs} >= {"mat_t", "conv_slab", "conv_slab_of", "lpr", "qk", "qk_t", "geglu_t", "geglu_lnf", "head"}
    for s, k in pairs:
        assert at[s] < at[k], (order, s, k)


def test_a_slab_without_its_tap_major_entry_is_made_from_the_parameter():
    m = modules()
    pk = Packer(torch.bfloat16, "cpu")
    slab = pk.conv_slab(m.conv)
    assert ("conv", id(m.conv)) not in list(pk)
    move(m)
    pk.refresh(EmuOps())
    assert torch.equal(slab, Packer(torch.bfloat16, "cpu").conv_slab(m.conv))


@pytest.mark.parametrize("method", ["lpr", "conv_slab_of"])
def test_a_tensor_that_is_no_entry_is_refused(method):
    m = modules()
    pk = Packer(torch.bfloat16, "cpu")
    w = pk.mat(m.lin) if method == "lpr" else pk.conv(m.conv)
    derive = getattr(pk, method)
    for foreign in (w.clone(), w[:64], torch.zeros_like(w), Packer(torch.bfloat16, "cpu").mat(m.lin)):
        with pytest.raises(ValueError, match=method):
            derive(foreign)
    n = len(pk)
    first = derive(w)
    assert derive(w) is first and len(pk) == n + 1
    wg = pk.geglu(m.proj)[0]                       # (a member of a tuple entry is a source too, and not the same one)
    if method == "lpr":
        assert pk.lpr(wg) is pk.lpr(wg) and pk.lpr(wg) is not first


def test_aliasing_and_static_entries_are_skipped():
    m = modules()
    pk = Packer(torch.bfloat16, "cpu")
    g = pk.f32(m.norm.weight)
    assert g.data_ptr() == m.norm.weight.data_ptr(), "an fp32 parameter where the Packer lives is its own pack"
    made = []
    table = pk.pack(("table", 1), lambda: made.append(1) or torch.arange(4), static=True)
    assert pk.pack(("table", 1), lambda: made.append(1) or torch.arange(4), static=True) is table
    move(m)
    assert record_refresh(pk, EmuOps()) == [] and made == [1]
    assert torch.equal(g, m.norm.weight.detach()) and torch.equal(table, torch.arange(4))
    # the same parameter in another dtype is a real pack: re-made
    m.norm.half()
    pk2 = Packer(torch.bfloat16, "cpu")
    g2 = pk2.f32(m.norm.weight)
    assert g2.data_ptr() != m.norm.weight.data_ptr()
    move(m)
    assert record_refresh(pk2, None) == [("f32", id(m.norm.weight))] and torch.equal(g2, m.norm.weight.detach().float())


def test_layouts_invert():
    """``lpr`` and ``conv_slab`` entries through native.py's inverse functions: the layouts are the ones the kernels were tested on."""
    m = modules()
    pk = build(Packer(torch.bfloat16, "cpu"), m, "dependants_first")
    move(m)
    pk.refresh(EmuOps())
    bf = lambda w: w.detach().to(torch.bfloat16)                                                   # noqa: E731
    assert torch.equal(nt.unpack_linear_pr(pk.lpr(pk.mat(m.lin))), bf(m.lin.weight))
    assert torch.equal(nt.unpack_linear_pr(pk.lpr(pk.cat_mats([m.lin, m.lin2], "qk"))), bf(torch.cat([m.lin.weight, m.lin2.weight])))
    assert torch.equal(nt.unpack_linear_pr(pk.lpr(pk.geglu(m.proj)[0])), pk.geglu(m.proj)[0])
    tap_major = bf(m.conv.weight).permute(0, 2, 3, 1).reshape(80, -1)
    assert torch.equal(nt.unpack_conv_slab(pk.conv_slab(m.conv), 64), tap_major) and torch.equal(pk.conv(m.conv), tap_major)
    assert torch.equal(nt.pack_linear_pr(bf(m.lin.weight)), pk.lpr(pk.mat(m.lin)))
    assert torch.equal(nt.pack_conv_slab(tap_major), pk.conv_slab(m.conv))
