"""``t2v_rank_loss`` on the device: the cases and bounds of tests/rank_loss_cases.py (shared with the host-simulator test), and the
multi-problem call with all outputs carved out of ONE allocation, guard words around each ``d_gen``."""
import pytest
import torch

from tests import rank_loss_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from t2v_turbo_amd.native import HipOps
    return HipOps()


def _run(ops, problems, n, k, alpha):
    """One call on NaN-filled outputs -> ([d_gen], loss), everything on the device."""
    dev = [(ref.cuda(), gen.cuda()) for ref, gen in problems]
    outs = [torch.full_like(ref, float("nan")) for ref, _ in dev]
    ws = torch.full((ops.rank_loss_ws_floats([ref.shape[0] for ref, _ in dev], n),), float("nan"), device="cuda")
    loss = torch.full((len(dev),), float("nan"), device="cuda")
    ops.rank_loss([(ref, gen, o) for (ref, gen), o in zip(dev, outs)], n, k, alpha, ws, loss)
    torch.cuda.synchronize()
    return outs, loss


@pytest.mark.parametrize("rows,n,k", rc.CASES)
def test_single_problem_matches_the_closed_form_and_repeats_bit_for_bit(ops, rows, n, k):
    ref, gen = rc.make(rows, n, seed=rows + n)
    alpha = 100.0 * 500.0 / 9
    (d0,), l0 = _run(ops, [(ref, gen)], n, k, alpha)
    rc.check(ref, gen, k, alpha, d0, l0[0].cpu())
    (d1,), l1 = _run(ops, [(ref, gen)], n, k, alpha)
    assert torch.equal(d0, d1) and torch.equal(l0, l1)


def test_three_problems_in_one_allocation_with_guard_words(ops):
    rows, n, k = rc.MULTI
    problems = [rc.make(r, n, seed=10 + i) for i, r in enumerate(rows)]
    GUARD, MAGIC = 64, -1234.5
    sizes = [r * n for r in rows]
    nws = ops.rank_loss_ws_floats(list(rows), n)
    arena = torch.full((sum(sizes) + GUARD * (len(sizes) + 3) + nws + len(rows),), MAGIC, device="cuda")
    views, off = [], GUARD
    for s in sizes + [nws, len(rows)]:
        views.append(arena[off:off + s])
        off += s + GUARD
    assert off == arena.numel()
    *outs, ws, loss = views
    for o in outs:
        o.fill_(float("nan"))
    dev = [(ref.cuda(), gen.cuda()) for ref, gen in problems]
    ops.rank_loss([(ref, gen, o.view(-1, n)) for (ref, gen), o in zip(dev, outs)], n, k, 0.37, ws, loss)
    torch.cuda.synchronize()
    for (ref, gen), d, l in zip(problems, outs, loss.cpu()):
        rc.check(ref, gen, k, 0.37, d, l)
    keep = torch.ones(arena.numel(), dtype=torch.bool, device="cuda")
    off = GUARD
    for s in sizes + [nws, len(rows)]:
        keep[off:off + s] = False
        off += s + GUARD
    assert bool((arena[keep] == MAGIC).all()), "a write outside the outputs"
    assert int(keep.sum()) == GUARD * (len(sizes) + 3)


def test_ties_go_to_the_higher_index(ops):
    ref = torch.tensor([rc.TIE_ROW, rc.TIE_ROW[::-1]])
    gen = torch.tensor([[0.3, 0.3, 0.3, 0.15], [0.4, 0.1, 0.2, 0.3]])
    for k in (1, 2, 3):
        sel, _, _ = rc.closed_form(ref, gen, k, 1.0)
        (d,), _ = _run(ops, [(ref, gen)], 4, k, 1.0)
        assert bool(torch.isfinite(d).all()) and torch.equal(d.cpu() != 0, sel)
    (d,), _ = _run(ops, [(ref, gen)], 4, 1, 1.0)
    assert (d.cpu() != 0).tolist() == [[False, False, True, False], [False, False, True, False]]


def test_bad_sizes_are_refused_before_any_launch(ops):
    from t2v_turbo_amd.native import NativeError
    ref, gen = (t.cuda() for t in rc.make(8, 4, seed=1))
    out, ws, loss = torch.zeros_like(ref), torch.zeros(64, device="cuda"), torch.zeros(17, device="cuda")
    for n, k, count, nws in [(4, 0, 1, 64), (4, 5, 1, 64), (4, 1, 17, 64), (4, 1, 16, 15)]:
        with pytest.raises(NativeError):
            ops.rank_loss([(ref, gen, out)] * count, n, k, 1.0, ws[:nws], loss)
