"""-m gpu: the spatial blocks' route on ONE q | k | v Linear + t2v_attn_spatial_rm (engine attribute ``attn_vrow``, environment
T2V_ATTN_VROW) against the q|k + V^T route it replaces: both within the end-to-end bound of tests/test_gpu_engine.py on the tiny
UNet configuration, and the recorded launch lists differ by exactly the launches the new route has no use for.

Launch accounting per spatial block: the V^T GEMM always goes; the zero-fill of the V^T buffer goes where the block had one (token
count not a multiple of 64); the t2v_layernorm launch goes where t2v_linear_pr takes norm1 into its panel fill (the 320- and
640-channel levels of the full-width network: K in ``linear_pr_min_n``).  At the full VideoCrafter2 widths every spatial block has
one of the two — 2 launches fewer per block, asserted on the full-width network below; the tiny configuration's widths (64 .. 256)
are not on the panel-resident kernel and its 256- and 64-token levels need no fill, so there the count follows the accounting."""
import pytest
import torch

from oracle import unet_oracle as uo
from oracle.synth import synth_state_dict
from tests.util import load, manifest, rel_l2, tiny_unet_params

pytestmark = pytest.mark.gpu
E2E_TOL = 3e-2      # tests/test_gpu_engine.py


def _record(model, eng, vrow, call):
    eng.attn_vrow = vrow
    eng.plans.clear()
    with torch.no_grad():
        y = call()
    rec = next(iter(eng.plans.values()))["rec"]
    return y.float().cpu(), [(name, args) for _, args, name in rec]


def _account(new, old):
    """-> (spatial blocks, blocks that had a zero-fill, blocks whose LayerNorm went into the panel fill); asserts the structure."""
    names_new, names_old = [n for n, _ in new], [n for n, _ in old]
    assert "t2v_attn_spatial_rm" not in names_old
    rm = [i for i, n in enumerate(names_new) if n == "t2v_attn_spatial_rm"]
    n_sp = len(rm)
    assert n_sp > 0, "the new route did not run"
    # one text cross-attention (V^T form) per spatial block stays; the self-attentions moved
    assert names_new.count("t2v_attn_spatial") == n_sp and names_old.count("t2v_attn_spatial") == 2 * n_sp
    n_pad = n_ln_in = 0
    for i in rm:
        args = new[i][1]
        seq, heads = args[9], args[10]
        prev, pargs = new[i - 1]
        assert prev in ("t2v_gemm", "t2v_linear_pr"), prev          # the q | k | v Linear feeds the attention directly:
        d = pargs[0]._obj                                            # no fill, no V^T GEMM in between
        assert d.N == 3 * heads * 64
        n_pad += seq % 64 != 0
        n_ln_in += prev == "t2v_linear_pr" and d.ln_in == 1
    # no t2v_fill_zero issued from a spatial block: only the fills that do not belong to one are left (the text V^T buffer)
    assert names_old.count("t2v_fill_zero") - names_new.count("t2v_fill_zero") == n_pad
    assert names_old.count("t2v_layernorm") - names_new.count("t2v_layernorm") == n_ln_in
    assert len(old) - len(new) == n_sp + n_pad + n_ln_in
    return n_sp, n_pad, n_ln_in


def test_tiny_unet_both_routes_and_launch_lists():
    from t2v_turbo_amd.unet3d import UNetModel
    g, cfg = load("unet_tiny"), tiny_unet_params()
    sd = synth_state_dict(manifest("unet_tiny"))
    m = UNetModel(**cfg).eval()
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda")
    x, ts, ctx, tc = g["x"].cuda(), g["ts"].cuda(), g["ctx"].cuda(), g["tc"].cuda()
    eng = m.native_engine()
    assert hasattr(eng.ops, "attn_spatial_rm")
    call = lambda: m(x, ts, context=ctx, fps=16, timestep_cond=tc)   # noqa: E731
    try:
        y_new, rec_new = _record(m, eng, True, call)
        y_old, rec_old = _record(m, eng, False, call)
    finally:
        eng.attn_vrow = type(eng).attn_vrow
        eng.plans.clear()
    ref = uo.unet_forward(sd, cfg, g["x"], g["ts"], g["ctx"], fps=16, timestep_cond=g["tc"])
    for tag, y in (("row-major V", y_new), ("V^T", y_old)):
        err, err_g = rel_l2(y, ref), rel_l2(y, g["y"])
        print(f"tiny UNet, {tag} route: rel-L2 vs oracle {err:.3e}, vs reference golden {err_g:.3e}")
        assert err < E2E_TOL and err_g < E2E_TOL, (tag, err, err_g)
    n_sp, n_pad, n_ln_in = _account(rec_new, rec_old)
    print(f"tiny UNet: {len(rec_old)} -> {len(rec_new)} launches; {n_sp} spatial blocks, {n_pad} zero-fills and {n_ln_in} LayerNorm launches gone")
    assert n_sp == 16 and n_pad >= 1   # (latent 16 x 16: the 16- and 4-token levels are padded)


def test_full_width_two_launches_fewer_per_spatial_block():
    """The VideoCrafter2 widths at the latent the benchmark times: every one of the 16 spatial blocks loses the V^T GEMM and either
    its LayerNorm launch (320 / 640 channels) or its zero-fill (1280 channels: 160 and 40 tokens)."""
    import bench
    dev = torch.device("cuda", 0)
    model = bench.build_model(dev, torch.bfloat16)
    x, ctx, tc = bench.synth_inputs(dev, torch.bfloat16)
    ts = torch.tensor([999], device=dev)
    eng = model.native_engine()
    call = lambda: model(x, ts, context=ctx, fps=16, timestep_cond=tc)   # noqa: E731
    try:
        y_new, rec_new = _record(model, eng, True, call)
        y_old, rec_old = _record(model, eng, False, call)
    finally:
        eng.attn_vrow = type(eng).attn_vrow
        eng.plans.clear()
    n_sp, n_pad, n_ln_in = _account(rec_new, rec_old)
    d = rel_l2(y_new, y_old)
    print(f"full width: {len(rec_old)} -> {len(rec_new)} launches ({n_sp} spatial blocks: {n_pad} zero-fills, {n_ln_in} LayerNorm launches gone); "
          f"rel-L2 between the routes {d:.3e}")
    assert (n_sp, n_pad, n_ln_in) == (16, 6, 10) and len(rec_old) - len(rec_new) == 2 * n_sp
    assert torch.isfinite(y_new).all() and d < E2E_TOL
