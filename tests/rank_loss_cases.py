"""Shared cases of ``t2v_rank_loss`` (csrc/backward_unet.hip) for the host-simulator and the device tests, and its float64
closed form:

    selected  <=> fewer than rank_k entries of the row beat the entry (a larger ref, or an equal ref at a higher index:
                  the last rank_k places of a stable ascending sort)
    loss[p]   =   sum over the selected entries of (gen - ref)^2 / (rows_p * rank_k)
    d_gen     =   alpha * 2 / (rows_p * rank_k) * (gen - ref) on the selected entries, 0 elsewhere

which is ``motion_prior.calculate_motion_rank_new`` and its autograd (checked in tests/test_input_grad_route_cpu.py).

Bounds, from the number formats alone:
  * a selected d_gen value takes three fp32 roundings (the coefficient, gen - ref, their product): 3 * 2^-24 < 1e-6 relative;
  * loss[p] is an fp32 sum of rows * k non-negative terms (the final stage runs in double): at most rows * k * 2^-24 relative.
Ties are a condition, not a tolerance: ``make`` asserts that no reference row of a random case holds two equal values (where the
selection would depend on the tie rule alone); the tie rule has its own hand-made case."""
import torch

# (rows, n, rank_k): several workgroups + a ragged tail | n not a power of two | k = n | one row per wave | the tiny fixture's frames
CASES = [(4099, 16, 1), (37, 12, 3), (130, 5, 5), (64, 64, 2), (256, 4, 1)]
MULTI = ((4099, 37, 256), 4, 1)      # one three-problem call: (rows per problem, n, rank_k)
TIE_ROW = [0.2, 0.5, 0.5, 0.1]       # rank_k = 1 selects index 2: the equal value at the higher index
EPS = 2.0 ** -24


def make(rows, n, seed):
    """(ref, gen): softmax(2 * randn) rows from a seeded generator, fp32."""
    g = torch.Generator().manual_seed(seed)
    ref = torch.softmax(2 * torch.randn(rows, n, generator=g), dim=-1)
    gen = torch.softmax(2 * torch.randn(rows, n, generator=g), dim=-1)
    srt = ref.sort(dim=-1).values
    assert not bool((srt[:, 1:] == srt[:, :-1]).any()), "a reference row with two equal values: pick another seed"
    return ref.contiguous(), gen.contiguous()


def closed_form(ref, gen, rank_k, alpha):
    """-> (selection mask, loss, d_gen) in float64."""
    r, g = ref.double(), gen.double()
    n = r.shape[-1]
    idx = torch.arange(n)
    # beats[.., j, t]: entry t beats entry j
    beats = (r[..., None, :] > r[..., :, None]) | ((r[..., None, :] == r[..., :, None]) & (idx[None, :] > idx[:, None]))
    sel = beats.sum(-1) < rank_k
    count = r.numel() // n * rank_k
    d = g - r
    loss = (d * d)[sel].sum() / count
    return sel, loss, torch.where(sel, alpha * 2.0 / count * d, torch.zeros_like(d))


def check(ref, gen, rank_k, alpha, d_gen, loss):
    """The device / simulator result of one problem against the closed form, under the bounds of the module docstring."""
    sel, loss64, d64 = closed_form(ref, gen, rank_k, alpha)
    d_gen = d_gen.cpu().reshape(ref.shape)
    assert bool(torch.isfinite(d_gen).all()), "d_gen: an element was not written"
    assert not bool((gen == ref).any())      # (a selected entry with gen == ref would have a zero gradient)
    assert torch.equal(d_gen != 0, sel), "the zero pattern of d_gen is not the closed form's selection"
    err = ((d_gen.double() - d64).abs() / d64.abs().clamp_min(1e-300))[sel]
    rows = ref.numel() // ref.shape[-1]
    loss_err = abs(float(loss) - float(loss64)) / float(loss64)
    print(f"rank_loss rows {rows} n {ref.shape[-1]} k {rank_k}: d_gen max rel {float(err.max()):.2e} (bound 1e-6), "
          f"loss rel {loss_err:.2e} (bound {rows * rank_k * EPS:.2e})")
    assert float(err.max()) < 1e-6
    assert loss_err <= rows * rank_k * EPS
