"""``t2v_rank_loss`` (csrc/backward_unet.hip: the motion-prior loss between two sets of temporal attention probabilities and its
gradient, every layer in one launch pair) executed thread by thread on the host SIMT simulator, against the float64 closed form of
tests/rank_loss_cases.py under the bounds derived there."""
import ctypes as C
import os
import shutil
import sys

import pytest
import torch

from t2v_turbo_amd import native as nt
from tests import rank_loss_cases as rc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))


@pytest.fixture(scope="module")
def sim():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    return HostSimOps(hostsim_build.build())


def _run(ops, problems, n, k, alpha):
    """One call on NaN-filled outputs -> ([d_gen], loss)."""
    outs = [torch.full_like(ref, float("nan")) for ref, _ in problems]
    ws = torch.full((ops.rank_loss_ws_floats([ref.shape[0] for ref, _ in problems], n),), float("nan"))
    loss = torch.full((len(problems),), float("nan"))
    ops.rank_loss([(ref, gen, o) for (ref, gen), o in zip(problems, outs)], n, k, alpha, ws, loss)
    return outs, loss


@pytest.mark.parametrize("rows,n,k", rc.CASES)
def test_single_problem_matches_the_closed_form_and_repeats_bit_for_bit(sim, rows, n, k):
    ref, gen = rc.make(rows, n, seed=rows + n)
    alpha = 100.0 * 500.0 / 9
    (d0,), l0 = _run(sim, [(ref, gen)], n, k, alpha)
    rc.check(ref, gen, k, alpha, d0, l0[0])
    (d1,), l1 = _run(sim, [(ref, gen)], n, k, alpha)
    assert torch.equal(d0, d1) and torch.equal(l0, l1)


def test_three_problems_in_one_call(sim):
    rows, n, k = rc.MULTI
    problems = [rc.make(r, n, seed=10 + i) for i, r in enumerate(rows)]
    outs, loss = _run(sim, problems, n, k, 0.37)
    for (ref, gen), d, l in zip(problems, outs, loss):
        rc.check(ref, gen, k, 0.37, d, l)
    outs2, loss2 = _run(sim, problems, n, k, 0.37)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2)) and torch.equal(loss, loss2)


def test_ties_go_to_the_higher_index(sim):
    ref = torch.tensor([rc.TIE_ROW, rc.TIE_ROW[::-1]])
    gen = torch.tensor([[0.3, 0.3, 0.3, 0.15], [0.4, 0.1, 0.2, 0.3]])
    for k in (1, 2, 3):
        sel, _, _ = rc.closed_form(ref, gen, k, 1.0)
        (d,), loss = _run(sim, [(ref, gen)], 4, k, 1.0)
        assert bool(torch.isfinite(d).all()) and torch.equal(d != 0, sel)
    (d,), _ = _run(sim, [(ref, gen)], 4, 1, 1.0)
    assert (d != 0).tolist() == [[False, False, True, False], [False, False, True, False]]


def test_bad_sizes_return_the_error_codes(sim):
    ref, gen = rc.make(8, 4, seed=1)
    out, ws, loss = torch.zeros_like(ref), torch.zeros(64), torch.zeros(17)
    arr = (nt.RankLossProblem * 17)()
    for d in arr:
        d.ref, d.gen, d.d_gen, d.rows = ref.data_ptr(), gen.data_ptr(), out.data_ptr(), 8
    table = C.cast(arr, C.c_void_p)

    def call(n_problems=1, n=4, k=1, ws_floats=64, tab=table):
        return sim.lib.t2v_rank_loss(tab, n_problems, n, k, 1.0, ws.data_ptr(), ws_floats, loss.data_ptr(), None)

    EINVAL, ESHAPE = -1, -2
    assert call() == 0
    assert call(n=0) == ESHAPE and call(n=65, k=1) == ESHAPE
    assert call(k=0) == ESHAPE and call(k=5) == ESHAPE
    assert call(n_problems=0) == EINVAL and call(n_problems=17) == EINVAL
    assert call(tab=None) == EINVAL
    assert call(n_problems=16, ws_floats=15) == ESHAPE and call(n_problems=16, ws_floats=16) == 0
    arr[0].rows = 0
    assert call() == EINVAL
