"""``t2v_ema_multi`` — the kernel SOURCE on the host SIMT simulator — on the shared case table (tests/ema_cases.py): bit-identical to
``t2v_ema_update`` of the same build per tensor, nothing written outside the targets, refusals of a malformed call."""
import os
import shutil
import sys

import pytest
import torch

from t2v_turbo_amd import native as nt
from tests.ema_cases import EmaCase, RATE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))


@pytest.fixture(scope="module")
def sim_ops():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    return HostSimOps(hostsim_build.build_full())


def test_ema_multi_kernel_source_on_the_case_table(sim_ops):
    case = EmaCase("cpu")
    table, n, work = case.table()
    sim_ops.ema_multi(table, n, work, RATE)
    case.check(sim_ops)


def test_ema_multi_work_blocks_nobody_owns_touch_nothing(sim_ops):
    """A launch that covers more work blocks than the table's tensors own (a gap after the last tensor) leaves everything else alone."""
    case = EmaCase("cpu", seed=12)
    table, n, work = case.table()
    sim_ops.ema_multi(table, n, work + 3, RATE)
    case.check(sim_ops)


def test_ema_multi_refuses_a_malformed_call(sim_ops):
    case = EmaCase("cpu", seed=13)
    table, n, work = case.table()
    lib = sim_ops.lib
    assert lib.t2v_ema_multi(None, n, work, RATE, None) == -1                       # T2V_EINVAL
    for bad_n, bad_work in ((0, work), (-1, work), (n, 0), (n, -5)):
        assert lib.t2v_ema_multi(table.data_ptr(), bad_n, bad_work, RATE, None) == -1
    assert all(torch.equal(t, b) for t, b in zip(case.targets, case.before))
    assert nt.C.sizeof(nt.EmaTensor) == 40 and table.numel() == 40 * n
