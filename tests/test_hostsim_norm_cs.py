"""The column-statistics GroupNorm case table (tests/norm_cs_cases.py) on the host SIMT simulator: every source of the library built by
tests/hostsim/build.py: build_full(), run on the CPU.  Proves the cases and their fp64 references without a GPU; the same table runs on
the device in tests/test_gpu_norm_cs.py."""
import os
import shutil
import sys

import pytest

from tests import norm_cs_cases as cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))


@pytest.fixture(scope="module")
def sim():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    ops = HostSimOps(hostsim_build.build_full())
    ops.tune, ops._ws = {}, {}
    ops.init()
    return ops


@pytest.mark.parametrize("name,fn,kw", cases.CASES, ids=cases.CASE_IDS)
def test_case(sim, name, fn, kw):
    cases.run(sim, "cpu", name, fn, kw)


@pytest.mark.parametrize("name", cases.REFUSAL_IDS)
def test_refusal(sim, name):
    cases.run_refusal(sim, "cpu", name)
