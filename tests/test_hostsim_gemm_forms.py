"""The GEMM-family case table (tests/gemm_form_cases.py) on the host SIMT simulator: every source of the library built by
tests/hostsim/build.py: build_full() (with the experimental tile ids and entry points), run on the CPU.  Proves the cases and their fp64
references without a GPU; the same table runs on the device in tests/test_gpu_gemm_forms.py.

The tile / store-path sweep runs here on ONE id per tile class (gemm_form_cases.CLASS_REPS: ids of a class share workgroup tile, K step and
staging path, hence the load / store index code).  Measured in one pytest run over both files on one machine, per-test durations summed,
libraries already built: with all 33 ids this file takes 97.5 s next to 36.9 s of tests/test_hostsim_gemm.py — longer, which is the
condition for the reduction; reduced (18 ids) it takes 78.4 s next to 29.7 s in another such run (35 conv_halo cases are 23 s of it, the
324 t2v_gemm tile cases 39 s).  The device file runs every id."""
import os
import shutil
import sys

import pytest

from tests import gemm_form_cases as cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))

CASES = cases.table(cases.CLASS_REPS, cases.CLASS_REPS) + cases.experimental_cases()


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


@pytest.mark.parametrize("name,fn,kw", CASES, ids=[c[0] for c in CASES])
def test_case(sim, name, fn, kw):
    cases.run(sim, "cpu", name, fn, kw)


@pytest.mark.parametrize("name", cases.REFUSAL_IDS)
def test_refusal(sim, name):
    cases.run_refusal(sim, "cpu", name, cases.gemm_refusal_cases)
