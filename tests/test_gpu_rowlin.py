"""The case table of tests/rowlin_cases.py on the device: t2v_rowlin_fwd / _bwd_data / _wgrad and t2v_timestep_embedding_f32 at the
operand forms the gradient engine hands them (views into NaN-poisoned buffers, sentinel-guarded outputs), fp64 reference, the derived
per-element bound 4 L 2^-24 sum|terms|, two calls bit for bit, refusals before any launch."""
import pytest
import torch

from tests import rowlin_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from t2v_turbo_amd.native import HipOps
    ops = HipOps()
    ops.init()
    return ops


@pytest.mark.parametrize("name", list(rc.LIN_CASES))
def test_rowlin_fwd(hip, name):
    rc.run_fwd(hip, "cuda", name)


@pytest.mark.parametrize("name", list(rc.BWD_CASES))
def test_rowlin_bwd_data(hip, name):
    rc.run_bwd(hip, "cuda", name)


@pytest.mark.parametrize("name", list(rc.LIN_CASES))
def test_rowlin_wgrad(hip, name):
    rc.run_wgrad(hip, "cuda", name)


@pytest.mark.parametrize("name", rc.REFUSALS)
def test_rowlin_refusals(hip, name):
    rc.run_refusal(hip, "cuda", name)


def test_timestep_embedding_f32(hip):
    rc.run_timestep_embedding_f32(hip, "cuda")


def test_dropout_f32(hip):
    rc.run_dropout_f32(hip, "cuda")


def test_the_new_entries_replay_through_t2v_replay(hip):
    """A recorded list with the three entries, replayed by the library's own walker (t2v_replay), gives the bits of the direct calls."""
    B, K, N = 3, 68, 72
    g = torch.Generator().manual_seed(0)
    x, w, dy = (torch.randn(s, generator=g).cuda() for s in ((B, K), (N, K), (B, N)))
    y, dx, dw = torch.zeros(B, N, device="cuda"), torch.zeros(B, K, device="cuda"), torch.zeros(N, K, device="cuda")
    ws = torch.empty(hip.rowlin_ws_floats([dict(w=w, y=dy, dx=dx)], B), device="cuda")
    hip.recording = []
    try:
        hip.rowlin_fwd([dict(x=x, w=w, y=y, silu=True)], B)
        hip.rowlin_bwd_data([dict(w=w, y=dy, dx=dx, x=x, silu=True)], B, ws)
        hip.rowlin_wgrad([dict(x=x, y=dy, dw=dw, silu=True)], B)
    finally:
        rec, hip.recording = hip.recording, None
    first = [t.clone() for t in (y, dx, dw)]
    for t in (y, dx, dw):
        t.fill_(float("nan"))
    hip.replay(rec, hip.stream())
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, (y, dx, dw)))
