"""-m gpu: t2v_attn_spatial_rm on the device — bit-identical to the V^T form of the kernel on the same values, and within the
project's attention tolerance of the fp32 softmax definition (cases and reasoning: tests/attn_rowmajor_cases.py)."""
import pytest

from tests import attn_rowmajor_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from t2v_turbo_amd.native import HipOps
    o = HipOps()
    o.init()
    return o


@pytest.mark.parametrize("n_img,seq,heads,spike", cases.CASES, ids=cases.CASE_IDS)
def test_attn_spatial_rm(ops, n_img, seq, heads, spike):
    cases.run(ops, "cuda", n_img, seq, heads, spike)


def test_attn_spatial_rm_refuses_bad_strides(ops):
    """The argument checks of t2v_attn_spatial: row strides % 8 (out: % 4) and >= heads * 64; refused before any launch."""
    import torch
    from t2v_turbo_amd.native import NativeError
    seq, inner = 64, 128
    qkv = torch.zeros(seq, 3 * inner + 8, dtype=torch.bfloat16, device="cuda")
    out = torch.full((seq, inner + 4), -7.0, dtype=torch.bfloat16, device="cuda")
    p = lambda t: t.data_ptr()   # noqa: E731
    good = dict(ldq=qkv.stride(0), ldk=qkv.stride(0), ldv=qkv.stride(0), ldo=out.stride(0))
    for bad in (dict(ldq=388), dict(ldk=388), dict(ldv=388), dict(ldo=130), dict(ldq=120), dict(ldv=120), dict(ldo=124)):
        a = dict(good, **bad)
        with pytest.raises(NativeError):
            ops._call("t2v_attn_spatial_rm", p(qkv), a["ldq"], p(qkv[:, inner:]), a["ldk"], p(qkv[:, 2 * inner:]), a["ldv"], p(out), a["ldo"],
                      1, seq, 2, 0.125)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote to its output"
