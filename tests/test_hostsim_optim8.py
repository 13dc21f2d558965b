"""``t2v_adamw8_step`` / ``t2v_quant8_blockwise`` / ``t2v_dequant8_blockwise`` — the kernel SOURCE on the host SIMT simulator —
against the CPU restatement of ``optim.AdamW8bit`` on the one-step case list (tests/optim8_util.build_case)."""
import os
import shutil
import sys

import pytest
import torch

from t2v_turbo_amd.optim import QBLOCK, make_code_books, quantize_blockwise, dequantize_blockwise
from tests.optim8_util import build_case, compare_with_restatement, cpu_twin

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))


@pytest.fixture(scope="module")
def sim_ops():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    return HostSimOps(hostsim_build.build_full())


@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_adamw8_kernel_source_matches_the_restatement(sim_ops, grad_scale):
    opt, params = build_case()
    twin, pairs = cpu_twin(opt)
    before = params["no_grad"].detach().clone()
    opt.native_ops = sim_ops
    opt.step(grad_scale=grad_scale)
    twin.step(grad_scale=grad_scale)
    compare_with_restatement(opt, pairs, twin, f"hostsim grad_scale={grad_scale}")
    assert torch.equal(params["no_grad"].detach(), before) and opt.state[params["no_grad"]]["step"] == 3
    assert all(opt.state[p]["step"] == 4 for n, p in params.items() if n != "no_grad")
    z = opt.state[params["zero_block"]]
    assert float(z["absmax1"][1]) == 0.0 and float(z["absmax2"][1]) == 0.0 and torch.isfinite(params["zero_block"]).all()


@pytest.mark.parametrize("n", [256, 1000, 4097])
def test_quant8_and_dequant8_kernel_sources(sim_ops, n):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * torch.rand(n, generator=gen).mul(8).sub(6).exp()
    nb = (n + QBLOCK - 1) // QBLOCK
    for code in make_code_books():
        xx = x if float(code[0]) < 0 else x.abs()
        want_c, want_a = quantize_blockwise(xx, code)
        codes, absmax = torch.full((nb * QBLOCK,), 77, dtype=torch.uint8), torch.zeros(nb)
        sim_ops.quant8(xx, code, codes, absmax)
        assert torch.equal(absmax, want_a)
        d = (codes.int() - want_c.int()).abs()
        assert int(d.max()) <= 1 and int(d.sum()) <= 1e-3 * d.numel() + 1
        out = torch.full((n + 3,), 5.0)
        sim_ops.dequant8(codes, absmax, code, out[:n])
        assert torch.equal(out[:n], dequantize_blockwise(codes, absmax, code, n)) and bool((out[n:] == 5.0).all())


def test_two_evaluation_orders_of_the_restatement_rarely_disagree():
    """The allowance of the kernel comparison (a code may differ by one where the value lies within fp32 rounding of a midpoint, on at
    most 0.1 % of the elements) is far from what rounding alone produces: nearest-code search by midpoints (the definition) against
    nearest-code search by distances, on random blocks."""
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(1 << 20, generator=gen) * torch.rand(1 << 20, generator=gen).mul(8).sub(6).exp()
    for code in make_code_books():
        xx = x if float(code[0]) < 0 else x.abs()
        codes, absmax = quantize_blockwise(xx, code)
        xn = xx.view(-1, QBLOCK) / absmax[:, None]
        other = torch.cat([(chunk[:, None] - code[None, :]).abs().argmin(dim=1) for chunk in xn.reshape(-1).split(1 << 16)])
        d = (codes.long() - other).abs()
        assert int(d.max()) <= 1 and float(d.sum()) / d.numel() < 1e-4
