"""The GEMM-family case table (tests/gemm_form_cases.py) on the device: t2v_gemm on every tile id and store path, its gather modes,
split-K, batching and fused epilogues, t2v_conv_halo, t2v_linear_pr, the wgrad products and the small kernels, at the engines' operand
forms with poisoned padding and guarded outputs.

Not run here, by name: tile ids 24-29 (experimental; with T2V_TEST_EXPERIMENTAL_TILES=1 they run), and the experimental entry points
t2v_ffn_fused and gemm2 (t2v_gemm2_enable), which the product library does not export.

Measured on an MI355X: the whole file (532 tests run, the 2 experimental entries skipped) takes 4.1 s; the slowest test is
gemm-dropout-p0.1-cfg4 at 0.09 s (it also launches t2v_dropout_bf16 over the full matrix), then dropout-inplace0-resid0 0.06 s,
wgrad-300x250x380-s0 0.04 s; module set-up (loading the library) 0.14 s."""
import os

import pytest
import torch

from tests import gemm_form_cases as cases

pytestmark = pytest.mark.gpu

_EXP = os.environ.get("T2V_TEST_EXPERIMENTAL_TILES") == "1"
CASES = cases.table(cases.VALIDATED + (cases.EXPERIMENTAL if _EXP else []), cases.DMA_REPS + (cases.RS_IDS if _EXP else []))


@pytest.fixture(scope="module")
def ops():
    from t2v_turbo_amd import native as nt
    o = nt.HipOps()
    o.init()
    return o


@pytest.mark.parametrize("name,fn,kw", CASES, ids=[c[0] for c in CASES])
def test_case(ops, name, fn, kw):
    cases.run(ops, "cuda", name, fn, kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,fn,kw", cases.experimental_cases(), ids=[c[0] for c in cases.experimental_cases()])
def test_experimental_entry(ops, name, fn, kw):
    if not hasattr(ops.lib, cases.EXPERIMENTAL_ENTRIES[kw["which"]]):
        pytest.skip("experimental entry point: not exported by the product library")
    cases.run(ops, "cuda", name, fn, kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", cases.REFUSAL_IDS)
def test_refusal(ops, name):
    cases.run_refusal(ops, "cuda", name, cases.gemm_refusal_cases)
