"""Engine dataflow on CPU: the native engines driven by the torch emulation of the op backend
(tests/emu_ops.py, fp32) must reproduce the oracle to fp32 round-off.  This pins everything the
engine decides — layouts, weight packing orders, virtual concat, folded upsampling, context/emb
dedup, buffer reuse — independently of the HIP kernels (which the -m gpu tests check per op)."""
import torch

from oracle import unet_oracle as uo
from oracle import vae_oracle as vo
from oracle import synth
from oracle.synth import synth_state_dict
from t2v_turbo_amd.engine import UNetEngine
from t2v_turbo_amd.engine_vae import VAEDecodeEngine
from t2v_turbo_amd.unet3d import UNetModel
from t2v_turbo_amd.vae import AutoencoderKL
from tests.emu_ops import EmuOps
from tests.util import VAE_TINY_DD, load, manifest, rel_l2, tiny_unet_params


def test_unet_engine_matches_oracle_and_golden():
    g = load("unet_tiny")
    cfg = tiny_unet_params(record_attn_probs=True)
    sd = synth_state_dict(manifest("unet_tiny"))
    m = UNetModel(**cfg).eval()
    m.load_state_dict(sd, strict=True)
    eng = UNetEngine(m, EmuOps())
    with torch.no_grad():
        y = eng(g["x"], g["ts"], g["ctx"], 16, g["tc"], None)
    assert rel_l2(y, g["y"]) < 2e-5
    probs = dict(m.named_modules())["output_blocks.11.2.transformer_blocks.0.attn1"].attention_probs
    assert rel_l2(probs, g["probs_ob11"]) < 2e-5
    # second call with different inputs goes through the recorded plan (static-buffer refresh)
    x2 = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(9))
    ts2 = torch.tensor([519])
    with torch.no_grad():
        y2 = eng(x2, ts2, g["ctx"], 24, g["tc"], None)
    ref2 = uo.unet_forward(sd, cfg, x2, ts2, g["ctx"], fps=24, timestep_cond=g["tc"])
    assert rel_l2(y2, ref2) < 2e-5
    # teacher-style call (no timestep_cond) is a different signature -> its own plan
    with torch.no_grad():
        y3 = eng(g["x"], g["ts"], g["ctx"])
    assert rel_l2(y3, g["y_nocond"]) < 2e-5
    assert len(eng.plans) == 2


def test_unet_engine_motion_cond_batch2_and_weight_update():
    g = load("unet_tiny_mg_b2")
    cfg = tiny_unet_params(motion_cond_proj_dim=256)
    sd = synth_state_dict(manifest("unet_tiny_mg_b2"))
    m = UNetModel(**cfg).eval()
    m.load_state_dict(sd, strict=True)
    eng = UNetEngine(m, EmuOps())
    with torch.no_grad():
        y = eng(g["x"], g["ts"], g["ctx"], 8, g["tc"], g["mc"])
    assert rel_l2(y, g["y"]) < 2e-5
    # in-place weight change must invalidate packed weights / plans
    with torch.no_grad():
        m.out[2].weight.mul_(2.0)
        m.out[2].bias.mul_(2.0)
        y2 = eng(g["x"], g["ts"], g["ctx"], 8, g["tc"], g["mc"])
    assert rel_l2(y2, 2.0 * g["y"]) < 2e-5


def test_vae_engine_matches_oracle_and_golden():
    g = load("vae_tiny")
    sd = synth_state_dict(manifest("vae_tiny"))
    ae = AutoencoderKL(ddconfig=VAE_TINY_DD, embed_dim=4).eval()
    assert [[k, list(v.shape)] for k, v in ae.state_dict().items()] == manifest("vae_tiny")
    ae.load_state_dict(sd, strict=True)
    eng = VAEDecodeEngine(ae, EmuOps())
    with torch.no_grad():
        v = eng.decode_frames(g["z"], scale=1.0 / 0.18215)
        v_cpu = ae.decode_video(g["z"])
    assert rel_l2(v, g["video"]) < 2e-5
    assert rel_l2(v_cpu, g["video"]) < 2e-5
    assert rel_l2(vo.decode_first_stage_2dae(sd, VAE_TINY_DD, g["z"]), g["video"]) < 1e-5


def test_vae_full_manifest():
    from tests.util import VAE_FULL_DD
    with torch.device("meta"):
        ae = AutoencoderKL(ddconfig=VAE_FULL_DD, embed_dim=4)
    assert [[k, list(v.shape)] for k, v in ae.state_dict().items()] == manifest("vae_full")


def test_vae_encoder_oracle_engine_and_module_vs_reference_golden():
    g = load("vae_tiny_enc")
    sd = synth_state_dict(manifest("vae_tiny"))
    m, mean, std = vo.encode_moments(sd, VAE_TINY_DD, g["x"])
    assert rel_l2(m, g["moments"]) < 1e-5 and rel_l2(mean, g["mean"]) < 1e-5 and rel_l2(std, g["std"]) < 1e-5
    ae = AutoencoderKL(ddconfig=VAE_TINY_DD, embed_dim=4).eval()
    ae.load_state_dict(sd, strict=True)
    with torch.no_grad():
        post = ae.encode(g["x"])
    assert rel_l2(post.parameters, g["moments"]) < 1e-5 and rel_l2(post.std, g["std"]) < 1e-5
    from t2v_turbo_amd.engine_vae import VAEEncodeEngine
    eng = VAEEncodeEngine(ae, EmuOps())
    x5 = g["x"].unsqueeze(0).transpose(1, 2).contiguous()  # (1,3,t=2,H,W): frames = the two images
    with torch.no_grad():
        mom = eng.encode_frames(x5)
    assert mom.shape == (1, 8, 2, 8, 8)
    assert rel_l2(mom[0].transpose(0, 1), g["moments"]) < 2e-5


def test_vae_decode_backward_dataflow_matches_oracle_autograd():
    """Native dX of the VAE decode: the recorded forward + backward launch lists, run by the torch
    emulation of the C-ABI ops, against torch autograd through the pinned fp32 oracle decoder."""
    from oracle import vae_oracle
    from t2v_turbo_amd.engine_vae_bwd import VAEDecodeGradEngine
    dd = dict(VAE_TINY_DD)
    ae = AutoencoderKL(ddconfig=dd, embed_dim=4).eval()
    sd = synth.synth_state_dict(synth.manifest_of(ae))
    ae.load_state_dict(sd)
    g = torch.Generator().manual_seed(3)
    z = torch.randn(1, 4, 2, 8, 8, generator=g)
    dout = torch.randn(1, 3, 2, 64, 64, generator=g)
    eng = VAEDecodeGradEngine(ae, EmuOps())
    out = eng.decode_frames_tape(z, 1.0)
    dz = eng.backward(dout)
    sd32 = {k: v.float() for k, v in sd.items()}
    zz = z.clone().requires_grad_(True)
    frames = []
    with torch.enable_grad():
        for i in range(2):
            zi = torch.nn.functional.conv2d(zz[:, :, i], sd32["post_quant_conv.weight"], sd32["post_quant_conv.bias"])
            frames.append(vae_oracle.decoder_forward.__wrapped__(sd32, dd, zi).unsqueeze(2))
        ref = torch.cat(frames, dim=2)
        (ref * dout).sum().backward()
    assert rel_l2(out, ref.detach()) < 2e-5
    assert rel_l2(dz, zz.grad) < 1e-4
    # replay on new inputs
    z2, dout2 = z * 0.7 + 0.2, dout.flip(-1)
    out2 = eng.decode_frames_tape(z2, 1.0)
    dz2 = eng.backward(dout2)
    zz2 = z2.clone().requires_grad_(True)
    with torch.enable_grad():
        fr = [vae_oracle.decoder_forward.__wrapped__(sd32, dd, torch.nn.functional.conv2d(
            zz2[:, :, i], sd32["post_quant_conv.weight"], sd32["post_quant_conv.bias"])).unsqueeze(2) for i in range(2)]
        ref2 = torch.cat(fr, dim=2)
        (ref2 * dout2).sum().backward()
    assert rel_l2(out2, ref2.detach()) < 2e-5 and rel_l2(dz2, zz2.grad) < 1e-4
    assert "gn_bwd" in eng.ops.calls and "softmax_bwd_rows" in eng.ops.calls and "sumpool2x2" in eng.ops.calls


def test_unet_engine_with_layernorm_fused_into_the_producing_gemm():
    """``fuse_ln`` (opt-in on the device, engine.py): the transformer blocks' LayerNorms as second outputs of proj_in and of the
    attention out-projections — the emulated backend takes the fused form at every width, so the dataflow (shared LN buffer,
    stream-order reuse, first block fed by proj_in) is pinned against the reference golden; fewer launches, same numbers."""
    g = load("unet_tiny")
    cfg = tiny_unet_params()
    m = UNetModel(**cfg).eval()
    m.load_state_dict(synth_state_dict(manifest("unet_tiny")), strict=True)
    counts = {}
    for fuse in (False, True):
        ops = EmuOps()
        eng = UNetEngine(m, ops)
        eng.linear_pr = eng.ln_in_fill = eng.gn_in_fill = False   # (round 6's routes have their own test below; the tiny config's 512-wide init_attn would take them)
        eng.fuse_ln, eng.fold_ln, eng.fuse_ff = fuse, False, False   # (the default since round 3 is the dataflow of the next test)
        with torch.no_grad():
            y = eng(g["x"], g["ts"], g["ctx"], 16, g["tc"], None)
        assert rel_l2(y, g["y"]) < 2e-5, fuse
        counts[fuse] = {name: ops.calls.count(name) for name in ("layernorm", "gemm")}
    n_ln = sum(1 for mod in m.modules() if isinstance(mod, torch.nn.LayerNorm))
    assert counts[False]["layernorm"] == n_ln and counts[True]["gemm"] == counts[False]["gemm"]
    # init_attn's proj_in is a Conv1d (openaimodel3d.py:439-453): its first LayerNorm stays a launch of its own
    assert 0 < counts[True]["layernorm"] <= 2


def test_unet_engine_norm_statistics_from_the_producing_gemms():
    """The inference engine's default dataflow since round 3: GroupNorm statistics come from the column statistics the producing
    GEMMs write (no statistics pass), and every LayerNorm with a single consuming GEMM (temporal q|k|v, text cross-attention q,
    the GEGLU projection) is folded into that GEMM on the raw rows (no LayerNorm launch, no normalised tensor).  Against the
    reference golden on the emulated backend, and launch counts against the un-fused dataflow."""
    from t2v_turbo_amd.unet3d import SpatialTransformer
    for fixture, extra in (("unet_tiny", {}), ("unet_tiny_mg_b2", {"motion_cond_proj_dim": 256})):
        g = load(fixture)
        m = UNetModel(**tiny_unet_params(**extra)).eval()
        m.load_state_dict(synth_state_dict(manifest(fixture)), strict=True)
        kw = dict(fps=g["fps"].item() if "fps" in g else 16)
        args = (g["x"], g["ts"], g["ctx"], 8 if fixture.endswith("b2") else 16, g["tc"], g.get("mc"))
        counts = {}
        for fused in (False, True):
            ops = EmuOps()
            eng = UNetEngine(m, ops)
            eng.linear_pr = eng.ln_in_fill = eng.gn_in_fill = False   # (round 6's routes have their own test below; the tiny config's 512-wide init_attn would take them)
            eng.fuse_gn = eng.fold_ln = eng.fold_ln_wide = fused    # (wide: also q|k|v and the GEGLU projection — off by default on the
            eng.fuse_ff = False                                      #  device, where it measured slower; the dataflow is pinned here)
            with torch.no_grad():
                y = eng(*args)
            assert rel_l2(y, g["y"]) < 2e-5, (fixture, fused)
            counts[fused] = {name: ops.calls.count(name) for name in ("layernorm", "gemm", "group_norm", "group_norm_cs")}
        n_ln = sum(1 for mod in m.modules() if isinstance(mod, torch.nn.LayerNorm))
        n_sp = sum(len(mod.transformer_blocks) for mod in m.modules() if isinstance(mod, SpatialTransformer))
        assert counts[False]["layernorm"] == n_ln and counts[False]["group_norm_cs"] == 0
        assert counts[True]["layernorm"] == n_sp          # only the spatial self-attention's norm1 (two consumers) stays a launch
        assert counts[True]["gemm"] == counts[False]["gemm"]
        # the device default folds only the text cross-attention's q: one LayerNorm per spatial block gone
        ops = EmuOps()
        eng = UNetEngine(m, ops)
        eng.linear_pr = eng.ln_in_fill = eng.gn_in_fill = False   # (round 6's routes have their own test below; the tiny config's 512-wide init_attn would take them)
        assert not eng.fuse_ff      # opt-in on the device (measured slower than three launches); its dataflow is pinned here
        eng.fuse_ff = True
        with torch.no_grad():
            y = eng(*args)
        assert rel_l2(y, g["y"]) < 2e-5 and eng.fold_ln and not eng.fold_ln_wide
        n_blocks = sum(1 for mod in m.modules() if type(mod).__name__ == "BasicTransformerBlock")
        # ... and every feed-forward (LayerNorm + GEGLU projection + output projection + residual) is ONE launch
        assert ops.calls.count("ffn_fused") == n_blocks and ops.calls.count("layernorm") == n_ln - n_sp - n_blocks
        # GroupNorm: every statistics unit of >= 32 rows whose input came out of a GEMM takes the producer's statistics
        n_gn = counts[False]["group_norm"]
        assert counts[True]["group_norm"] + counts[True]["group_norm_cs"] == n_gn and counts[True]["group_norm_cs"] > n_gn // 3


def test_train_mode_frozen_teacher_runs_natively_with_replayed_masks():
    """The v1 distillation teacher as the reference runs it: frozen, LoRA-free, NEVER put in eval mode
    (train_t2v_turbo_v1_lora.py:621-626, forwards under no_grad at :1105-1134), so the Dropout(0.1) of every TemporalConvBlock stage
    (openaimodel3d.py:282-294) is live.  The inference engine applies them as counter-based masks; replaying those masks inside
    the torch module reproduces its output; the route does not fall to the composite path (no RuntimeWarning)."""
    import copy
    import warnings
    from tests.mask_replay import patch_engine_masks
    g = load("unet_tiny")
    cfg = tiny_unet_params()
    sd = synth_state_dict(manifest("unet_tiny"))
    m = UNetModel(**cfg)
    m.load_state_dict(sd, strict=True)
    m.requires_grad_(False)
    m.train()
    ops = EmuOps()
    ops.masks = {}
    eng = UNetEngine(m, ops)
    eng.seed_source = iter([1234, 99, 99])
    with torch.no_grad():
        y = eng(g["x"], g["ts"], g["ctx"])               # teacher-style call: no timestep_cond
    assert len(eng.drop_sites) > 0 and all(kind == "tconv" for _, kind, _ in eng.drop_sites)
    assert rel_l2(y, g["y_nocond"]) > 1e-3                # the masks did something
    ref_m = copy.deepcopy(m)
    patch_engine_masks(ref_m, eng, ops.masks)
    ref_m.native_mode = "off"
    with torch.no_grad():
        ref = ref_m(g["x"], g["ts"], context=g["ctx"])
    assert rel_l2(y, ref) < 2e-5
    # a new seed per call (replayed plan), the same seed -> the same output
    with torch.no_grad():
        y2 = eng(g["x"], g["ts"], g["ctx"])
        y3 = eng(g["x"], g["ts"], g["ctx"])
    assert rel_l2(y2, y) > 1e-4 and torch.equal(y2, y3)
    # the module's own routing sends this call pattern to the inference engine, silently
    route, why = m._auto_route(g["x"], g["ctx"], None, None)
    assert (route, why) == ("infer", None)
    m.eval()
    with torch.no_grad():
        y_eval = eng(g["x"], g["ts"], g["ctx"])          # back in eval mode: a different plan, no masks
    assert rel_l2(y_eval, g["y_nocond"]) < 2e-5
    # any OTHER live dropout still refuses
    m.train()
    m.output_blocks[0][0].out_layers[2].p = 0.5
    try:
        with torch.no_grad():
            eng(g["x"], g["ts"], g["ctx"])
        raise AssertionError("expected a refusal")
    except RuntimeError as e:
        assert "Dropout" in str(e)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert m._auto_route(g["x"], g["ctx"], None, None)[0] == "composite"


def test_width_320_transformer_linears_take_the_panel_resident_route():
    """At model_channels = 320 / 640 the engine sends the GEGLU projection and the q | k | v / q | k launches to t2v_linear_pr with the
    fragment pack of the same matrices (engine._lpr_takes, native.pack_linear_pr); everything else stays on t2v_gemm.  A two-level UNet
    (320 and 640 channels) against the module's own torch forward."""
    for mc, mult in ((320, [1, 2]),):
        cfg = tiny_unet_params(model_channels=mc, channel_mult=mult, num_res_blocks=1, attention_resolutions=[1, 2], context_dim=64)
        torch.manual_seed(3)
        m = UNetModel(**cfg).eval()
        with torch.no_grad():
            for p in m.parameters():   # (zero-initialised output projections would hide the transformer blocks)
                if p.abs().max() == 0:
                    p.normal_(0.0, 0.02)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(1, 4, 2, 16, 20, generator=g)   # (320 tokens per frame: statistics units that are whole 160-row panels, for gn_in)
        ts = torch.tensor([500])
        ctx = torch.randn(1, 7, 64, generator=g)
        ops = EmuOps()
        eng = UNetEngine(m, ops)
        with torch.no_grad():
            y = eng(x, ts, ctx, 16, None, None)
            ref = m(x, ts, context=ctx, fps=16)
        assert rel_l2(y, ref) < 2e-5
        n_lpr = ops.calls.count("linear_pr")
        # per transformer pair: spatial block q|k (320 only: N = 1280 < 1920 at 640) + GEGLU, temporal block 2 x q|k|v + GEGLU
        assert n_lpr >= 12, n_lpr
        # LayerNorm in the panel fill (ln_in): the temporal blocks' norm1 / norm2 and every norm3 at these widths are no launches of their own
        n_ln = ops.calls.count("layernorm")
        eng.ln_in_fill = False
        eng.plans.clear()
        ops.calls.clear()
        with torch.no_grad():
            y1 = eng(x, ts, ctx, 16, None, None)
        assert ops.calls.count("layernorm") >= n_ln + 8 and ops.calls.count("linear_pr") == n_lpr and rel_l2(y1, y) < 1e-6
        # GroupNorm in proj_in's panel fill (gn_in) at the 320-channel level: statistics launch + one linear_pr launch per transformer
        n_gc = ops.calls.count("gn_coef_cs")
        assert n_gc >= 2, n_gc
        eng.ln_in_fill, eng.gn_in_fill = True, False
        eng.plans.clear()
        ops.calls.clear()
        with torch.no_grad():
            y2 = eng(x, ts, ctx, 16, None, None)
        assert ops.calls.count("gn_coef_cs") == 0 and ops.calls.count("linear_pr") == n_lpr - n_gc and rel_l2(y2, y) < 2e-5   # (x a + b against (x - mean) rstd gamma + beta in fp32)
        eng.linear_pr = False
        eng.plans.clear()
        ops.calls.clear()
        with torch.no_grad():
            y0 = eng(x, ts, ctx, 16, None, None)
        assert "linear_pr" not in ops.calls and rel_l2(y0, y) < 2e-5 and rel_l2(y0, y2) < 1e-6


def test_inference_engines_under_the_record_replay_protocol():
    """The UNet, VAE decode / encode and VAE decode gradient engines on the native backend's protocol (tests.emu_ops.ReplayOps:
    launch lists recorded once, later calls refresh the static inputs and re-issue the lists) against the same engines
    re-running their closures (EmuOps): the same launches on the same operands, so every output is bit-equal."""
    from t2v_turbo_amd.engine_vae import VAEEncodeEngine
    from t2v_turbo_amd.engine_vae_bwd import VAEDecodeGradEngine
    from tests.emu_ops import ReplayOps
    backends = (lambda: EmuOps(strict=True), ReplayOps)

    def both(make, run, plan_of, lists, replays):
        outs = []
        for backend in backends:
            ops = backend()
            eng = make(ops)
            with torch.no_grad():
                outs.append(run(eng))
            plan = plan_of(eng)
            if ops.is_native:
                assert all(k in plan for k in lists) and "fn" not in plan and "fn_bwd" not in plan
                assert ops.replays == replays   # the later calls replayed the lists: nothing was recorded twice
                assert len(eng.plans) == 1
            else:
                assert "fn" in plan and "rec" not in plan
        assert len(outs[0]) == len(outs[1])
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        return plan

    only_plan = lambda eng: next(iter(eng.plans.values()))  # noqa: E731
    g = load("unet_tiny")
    m = UNetModel(**tiny_unet_params()).eval()
    m.load_state_dict(synth_state_dict(manifest("unet_tiny")), strict=True)
    x2 = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(9))
    plan = both(lambda ops: UNetEngine(m, ops),
                lambda eng: [eng(g["x"], g["ts"], g["ctx"], 16, g["tc"], None), eng(x2, torch.tensor([519]), g["ctx"], 24, g["tc"], None)],
                only_plan, ("rec",), 1)
    assert len(plan["rec"]) > 500 and "rec_bwd" not in plan

    gv = load("vae_tiny")
    ae = AutoencoderKL(ddconfig=VAE_TINY_DD, embed_dim=4).eval()
    ae.load_state_dict(synth_state_dict(manifest("vae_tiny")), strict=True)
    z2 = torch.randn(gv["z"].shape, generator=torch.Generator().manual_seed(1))
    scale = 1.0 / 0.18215
    both(lambda ops: VAEDecodeEngine(ae, ops), lambda eng: [eng.decode_frames(gv["z"], scale), eng.decode_frames(z2, scale)],
         only_plan, ("rec",), 1)

    x5 = load("vae_tiny_enc")["x"].unsqueeze(0).transpose(1, 2).contiguous()
    x6 = torch.randn(x5.shape, generator=torch.Generator().manual_seed(2))
    both(lambda ops: VAEEncodeEngine(ae, ops), lambda eng: [eng.encode_frames(x5), eng.encode_frames(x6)], only_plan, ("rec",), 1)

    def pairs(eng):
        r = []
        for z in (gv["z"], z2):
            v = eng.decode_frames_tape(z, scale)
            r += [v, eng.backward(torch.ones_like(v))]
        return r

    # recording runs both lists, then the forward list once more (the recorded backward recycled its saved buffers) and the
    # backward list for the first pair; the second pair is one replay of each
    both(lambda ops: VAEDecodeGradEngine(ae, ops), pairs, lambda eng: eng._last, ("rec", "rec_bwd"), 4)


def test_launch_list_cut_at_host_calls():
    """``engine.cut_at_host_calls``: the runs of launches that become one hipGraph each, and the host calls between them."""
    from t2v_turbo_amd.engine import HOST_CALL, cut_at_host_calls

    def launch(i):
        return (print, (i,), f"t2v_launch_{i}")

    def host(i):
        return (len, (i,), HOST_CALL)

    def check(rec):
        runs = cut_at_host_calls(rec)
        flat = []
        for launches, call in runs:
            assert (launches is None) != (call is None)
            if call is None:
                assert len(launches) > 0 and all(e[2] != HOST_CALL for e in launches)
                flat += launches
            else:
                flat.append((call[0], call[1], HOST_CALL))
        assert flat == rec   # the pieces, in order, are the list
        for (a, _), (b, _) in zip(runs, runs[1:]):
            assert a is None or b is None   # two runs of launches are never adjacent: only a host call ends a run
        return runs

    assert cut_at_host_calls([]) == []
    plain = [launch(i) for i in range(5)]
    runs = check(plain)
    assert len(runs) == 1 and runs[0][0] is plain and runs[0][1] is None   # the list itself: its compiled program stays cached
    L, H = launch, host
    assert [r[0] is None for r in check([H(0), L(1), L(2)])] == [True, False]                      # first
    assert [r[0] is None for r in check([L(0), L(1), H(2)])] == [False, True]                      # last
    assert [r[0] is None for r in check([L(0), H(1), H(2), L(3)])] == [False, True, True, False]   # adjacent
    assert [r[0] is None for r in check([H(0)])] == [True]                                         # alone
    runs = check([H(0), L(1), H(2), L(3), L(4), H(5), H(6), L(7), H(8)])
    assert [None if r[0] is None else len(r[0]) for r in runs] == [None, 1, None, 2, None, None, 1, None]
    assert [r[1][1] for r in runs if r[0] is None] == [(0,), (2,), (5,), (6,), (8,)]
