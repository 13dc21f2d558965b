"""t2v_attn_spatial_rm on the host SIMT simulator (the whole library, tests/hostsim/build.py: build_full(), which compiles
csrc/attention.hip): the cases of tests/attn_rowmajor_cases.py on the CPU — the transposing LDS read is simulated with the lane
mapping measured on the device (tools/probes/tr_b16_probe.cpp), so the tile layout, the read addresses, the zero-page rows and the
contraction order are checked before any device run.  The same cases run on the device in tests/test_gpu_attn_rowmajor.py."""
import os
import shutil
import sys

import pytest

from tests import attn_rowmajor_cases as cases

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


@pytest.mark.parametrize("n_img,seq,heads,spike", cases.CASES, ids=cases.CASE_IDS)
def test_attn_spatial_rm(sim, n_img, seq, heads, spike):
    cases.run(sim, "cpu", n_img, seq, heads, spike)
