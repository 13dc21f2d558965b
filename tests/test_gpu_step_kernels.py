"""The flat step kernel case table (tests/step_kernel_cases.py) on the device: poisoned padding, guarded outputs and bounds from an fp64
reference written out from the definitions in include/t2v_hip.h."""
import pytest
import torch

from tests import step_kernel_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from t2v_turbo_amd import native as nt
    o = nt.HipOps()
    o.init()
    return o


@pytest.mark.parametrize("name,fn,kw", cases.CASES, ids=cases.CASE_IDS)
def test_case(ops, name, fn, kw):
    cases.run(ops, "cuda", name, fn, kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", cases.REFUSAL_IDS)
def test_refusal(ops, name):
    cases.run_refusal(ops, "cuda", name)
