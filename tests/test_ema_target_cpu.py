"""The EMA target network on the inference engine, on the CPU (tests.emu_ops.ReplayOps: the native backend's record / replay protocol on
the torch emulation).  train_latent_t2v_turbo_v2.py --use_target_unet moves the target's weights in place after every optimizer step
(``update_ema``, :1272-1276) and calls it under ``no_grad`` (:1238-1245): the engine keeps its recorded plans and re-fills the weight
packs their launch lists point at (``Packer.refresh``) instead of packing and recording the network again; only a change of the
parameter STRUCTURE (a replaced or re-homed parameter) drops the plans."""
import pytest
import torch
import torch.nn as nn

from oracle.synth import manifest_of, synth_state_dict
from t2v_turbo_amd import cd_math, optim
from t2v_turbo_amd.engine import UNetEngine
from t2v_turbo_amd.unet3d import UNetModel
from tests.emu_ops import ReplayOps
from tests.util import load, tiny_unet_params


def _model(cfg, seed=1234):
    m = UNetModel(**cfg).eval()
    m.load_state_dict(synth_state_dict(manifest_of(m), seed), strict=True)
    return m.requires_grad_(False)


def _tiny_case():
    g = load("unet_tiny")
    return tiny_unet_params(), (g["x"], g["ts"], g["ctx"], 16, g["tc"], None)


def _mg_b2_case():
    g = load("unet_tiny_mg_b2")
    return tiny_unet_params(motion_cond_proj_dim=256), (g["x"], g["ts"], g["ctx"], 8, g["tc"], g["mc"])


def _w320_case():
    # the configuration of tests/test_engine_cpu.py::test_width_320_transformer_linears_take_the_panel_resident_route
    cfg = tiny_unet_params(model_channels=320, channel_mult=[1, 2], num_res_blocks=1, attention_resolutions=[1, 2], context_dim=64)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, 2, 16, 20, generator=g)
    return cfg, (x, torch.tensor([500]), torch.randn(1, 7, 64, generator=g), 16, None, None)


CASES = {"tiny": _tiny_case, "mg_b2": _mg_b2_case, "w320": _w320_case, "fold_ln": _tiny_case, "bf16_params": _tiny_case}


def _engine(m, name="tiny"):
    eng = UNetEngine(m, ReplayOps())
    if name == "fold_ln":
        eng.fold_ln = True     # (T2V_FOLD_LN=1, whatever the environment says: the ``mat_lnf`` packs)
    return eng


def _fresh(m, args, name="tiny"):
    with torch.no_grad():
        return _engine(m, name)(*args)


def _pack_kinds(eng):
    return {k[0] for k in eng.pk}


@pytest.mark.parametrize("name", list(CASES))
def test_plans_survive_in_place_updates(name):
    """Forward, then three rounds of ``optim.update_ema`` + forward: the plan object stays, nothing is recorded again, the launch list
    is replayed, and every output is bit-equal to a FRESH engine's on the updated weights (rate 0.5: every pack visibly moves)."""
    cfg, args = CASES[name]()
    m, other = _model(cfg), _model(cfg, seed=77)
    if name == "bf16_params":   # the engine's fp32 packs are then COPIES of every parameter (``f32`` / ``bias`` / ``mat`` of a bf16 tensor)
        m, other = m.bfloat16(), other.bfloat16()
    eng = _engine(m, name)
    with torch.no_grad():
        y0 = eng(*args)
    (key, plan), = eng.plans.items()
    assert eng.counters == {"recorded": 1, "refreshed": 0}
    kinds = _pack_kinds(eng)
    assert {"mat", "bias", "f32", "conv", "small", "geglu", "emb_all", "emb_all_bias", "qk", "ctx_k_all"} <= kinds, kinds
    if name == "w320":
        assert "lpr" in kinds   # the panel-resident route's fragment packs (and its ``ln_in`` affines, ``f32``) are among the refreshed
    if name == "fold_ln":
        assert "q_lnf" in kinds
    ptrs, replays, last = eng.pk.pointers(), eng.ops.replays, y0
    for rnd in range(1, 4):   # (the second and third update: "same signature" passes of the refresh)
        optim.update_ema(m.parameters(), other.parameters(), 0.5)
        with torch.no_grad():
            y = eng(*args)
        assert eng.plans[key] is plan and len(eng.plans) == 1
        assert eng.counters == {"recorded": 1, "refreshed": rnd}
        assert eng.ops.replays == replays + rnd and eng.pk.pointers() == ptrs
        assert not torch.equal(y, last)
        assert torch.equal(y, _fresh(m, args, name)), (name, rnd)
        last = y
    with torch.no_grad():       # no update in between: neither a refresh nor a recording
        assert torch.equal(eng(*args), last)
    assert eng.counters == {"recorded": 1, "refreshed": 3}


def test_two_plans_share_the_refreshed_packer():
    cfg, args = _tiny_case()
    x, ts, ctx, fps, tc, _ = args
    args2 = (x, ts, ctx)                      # teacher-style call: another input signature, its own plan
    m, other = _model(cfg), _model(cfg, seed=77)
    eng = _engine(m)
    with torch.no_grad():
        eng(*args)
        eng(*args2)
    assert len(eng.plans) == 2 and eng.counters == {"recorded": 2, "refreshed": 0}
    pk, plans = eng.pk, dict(eng.plans)
    optim.update_ema(m.parameters(), other.parameters(), 0.5)
    with torch.no_grad():
        y1, y2 = eng(*args), eng(*args2)
    assert eng.pk is pk and all(eng.plans[k] is p for k, p in plans.items())
    assert eng.counters == {"recorded": 2, "refreshed": 1}
    assert torch.equal(y1, _fresh(m, args)) and torch.equal(y2, _fresh(m, args2))


def test_a_plan_recorded_after_an_update_adds_packs_to_the_refreshed_packer():
    """The second input signature is first seen AFTER an update: its recording finds the shared Packer already re-filled (the refresh
    runs before the plan lookup), so both plans read current packs and the first plan is not recorded again."""
    cfg, args = _tiny_case()
    m, other = _model(cfg), _model(cfg, seed=77)
    eng = _engine(m)
    with torch.no_grad():
        eng(*args)
    optim.update_ema(m.parameters(), other.parameters(), 0.5)
    args2 = args[:3]
    with torch.no_grad():
        y2 = eng(*args2)
        y1 = eng(*args)
    assert eng.counters == {"recorded": 2, "refreshed": 1}
    assert torch.equal(y2, _fresh(m, args2)) and torch.equal(y1, _fresh(m, args))


def test_a_structural_change_drops_the_plans():
    cfg, args = _tiny_case()
    m = _model(cfg)
    eng = _engine(m)
    with torch.no_grad():
        eng(*args)
    (key, plan), = eng.plans.items()
    pk = eng.pk
    m.out[2].weight = nn.Parameter(m.out[2].weight.detach() * 2.0, requires_grad=False)
    m.out[2].bias = nn.Parameter(m.out[2].bias.detach() * 2.0, requires_grad=False)
    with torch.no_grad():
        y = eng(*args)
    assert eng.plans[key] is not plan and eng.pk is not pk
    assert eng.counters == {"recorded": 2, "refreshed": 0}
    assert torch.equal(y, _fresh(m, args))
    # ... and so does a cast (every parameter re-homed)
    m.bfloat16()
    with torch.no_grad():
        y = eng(*args)
    assert eng.counters == {"recorded": 3, "refreshed": 0} and torch.equal(y, _fresh(m, args))


def test_the_reference_ema_loop_and_load_state_dict_are_answered_by_a_refresh():
    cfg, args = _tiny_case()
    m, other = _model(cfg), _model(cfg, seed=77)
    eng = _engine(m)
    with torch.no_grad():
        eng(*args)
    (key, plan), = eng.plans.items()
    cd_math.update_ema(m.parameters(), other.parameters(), 0.5)
    with torch.no_grad():
        y = eng(*args)
    assert eng.plans[key] is plan and eng.counters == {"recorded": 1, "refreshed": 1}
    assert torch.equal(y, _fresh(m, args))
    with torch.no_grad():       # the reference's loop, spelled out (utils/common_utils.py:307-319)
        for targ, src in zip(m.parameters(), other.parameters()):
            targ.detach().mul_(0.9).add_(src, alpha=0.1)
        y = eng(*args)
    assert eng.plans[key] is plan and eng.counters == {"recorded": 1, "refreshed": 2}
    assert torch.equal(y, _fresh(m, args))
    m.load_state_dict(other.state_dict())
    with torch.no_grad():
        y = eng(*args)
    assert eng.plans[key] is plan and eng.counters == {"recorded": 1, "refreshed": 3}
    assert torch.equal(y, _fresh(other, args))


def test_update_ema_on_cpu_tensors_is_the_torch_expression():
    gen = torch.Generator().manual_seed(0)
    shapes = [(7,), (33, 5), (4, 3, 3, 3), (1,)]
    tg = [torch.randn(s, generator=gen) for s in shapes]
    sr = [torch.randn(s, generator=gen) for s in shapes]
    tg.append(torch.randn(6, 8, generator=gen).t())          # a non-contiguous target
    sr.append(torch.randn(8, 6, generator=gen))
    tg.append(torch.randn(9, generator=gen).half())           # an fp16 target with an fp32 source
    sr.append(torch.randn(9, generator=gen))
    tg.append(torch.randn(12, generator=gen))                 # a bf16 source
    sr.append(torch.randn(12, generator=gen).bfloat16())
    want = [t.clone() for t in tg]
    for t, s in zip(want, sr):
        t.mul_(0.95).add_(s.to(t.dtype), alpha=1 - 0.95)
    before = [t.clone() for t in tg]
    optim.update_ema((t for t in tg), (s for s in sr), 0.95)  # generators, as ``parameters()`` gives them
    for t, w, b in zip(tg, want, before):
        assert torch.equal(t, w) and not torch.equal(t, b)
    # the reference-shaped helper gives the same bits (tests/test_sched_pipeline.py pins its numbers)
    again = [b.clone() for b in before]
    cd_math.update_ema(again, sr, 0.95)
    assert all(torch.equal(a, w) for a, w in zip(again, want))
    # the default rate
    t, s = torch.ones(3), torch.zeros(3)
    optim.update_ema([t], [s])
    assert torch.equal(t, torch.ones(3).mul_(0.99))


@pytest.mark.parametrize("name", ["tiny", "w320", "fold_ln", "bf16_params", "lora_merged", "fold_ln_wide"])
def test_every_pack_of_the_inference_engine_refreshes_to_a_fresh_packers_value(name):
    """Every pack the inference engine makes on a small network — ``mat``, ``cat_mats`` (q | k, q | k | v, the stacked emb_layers and
    context K / V), ``bias``, ``cat_biases``, ``f32``, ``conv``, ``conv_slab``, ``lpr``, ``geglu``, ``mat_lnf``, ``geglu_lnf``,
    ``small_conv`` and the merged-LoRA forms of the leaves: after an in-place move of every parameter, ``refresh`` leaves each entry
    bit-equal to the entry a fresh engine's Packer makes, at the address it had."""
    base = {"lora_merged": "tiny", "fold_ln_wide": "tiny"}.get(name, name)
    cfg, args = CASES[base]()
    m, other = _model(cfg), _model(cfg, seed=77)
    if name == "bf16_params":
        m, other = m.bfloat16(), other.bfloat16()
    if name == "lora_merged":
        from t2v_turbo_amd.lora import inject_trainable_lora_extended
        for net, seed in ((m, 3), (other, 4)):
            inject_trainable_lora_extended(net, r=4)
            gen = torch.Generator().manual_seed(seed)
            with torch.no_grad():
                for n_, p in net.named_parameters():
                    if "lora_up" in n_:          # (zero-initialised: the merge would add nothing)
                        p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
            net.requires_grad_(False).eval()     # (the injected leaves are new modules: born in train mode, with a live Dropout)

    def make():
        eng = _engine(m, base)
        if name == "fold_ln_wide":
            eng.fold_ln = eng.fold_ln_wide = True      # q | k | v and the GEGLU projection folded too: ``qkv_lnf`` and ``geglu_lnf``
            eng.linear_pr = eng.ln_in_fill = False
        with torch.no_grad():
            eng(*args)
        return eng

    eng = make()
    kinds = _pack_kinds(eng)
    need = {"tiny": {"mat", "bias", "f32", "conv", "small", "geglu", "qk", "qkv", "emb_all", "emb_all_bias", "ctx_k_all", "ctx_v_all"},
            "w320": {"lpr", "geglu", "qk", "qkv"}, "fold_ln": {"q_lnf"}, "bf16_params": {"f32", "bias", "mat"},
            "lora_merged": {"mat", "conv", "geglu"}, "fold_ln_wide": {"qkv_lnf", "geglu_lnf", "geglu_lnf_src"}}[name]
    assert need <= kinds, (need - kinds, kinds)
    keys, ptrs = list(eng.pk), eng.pk.pointers()
    before = {k: [t.clone() for t in _tensors(eng.pk[k].value)] for k in keys}
    optim.update_ema(m.parameters(), other.parameters(), 0.5)
    eng.pk.refresh(eng.ops)
    assert list(eng.pk) == keys and eng.pk.pointers() == ptrs
    fresh = make().pk
    assert set(fresh) == set(keys)
    for k in keys:
        got, want = _tensors(eng.pk[k].value), _tensors(fresh[k].value)
        assert len(got) == len(want), k
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (name, k[0])
        assert any(not torch.equal(a, o) for a, o in zip(got, before[k])), ("the update did not reach this pack", k[0])


def _tensors(v):
    return [v] if isinstance(v, torch.Tensor) else list(v)


def test_conv_slab_packs_refresh_through_their_tap_major_source():
    """``conv_slab`` (the halo kernel's pack: made only where the backend offers ``conv_halo_supported``, which the emulation does not)
    on the engine's own Packer, from the tap-major entry and from the parameter."""
    from t2v_turbo_amd.engine import Packer
    cfg, _ = _tiny_case()
    m, other = _model(cfg), _model(cfg, seed=77)
    convs = [m.input_blocks[1][0].in_layers[2], m.input_blocks[1][0].out_layers[3]]
    pk = Packer(torch.bfloat16, "cpu")
    pk.conv(convs[0])
    slabs = [pk.conv_slab(c) for c in convs]
    optim.update_ema(m.parameters(), other.parameters(), 0.5)
    pk.refresh(None)
    fresh = Packer(torch.bfloat16, "cpu")
    for c, s in zip(convs, slabs):
        assert torch.equal(s, fresh.conv_slab(c))
