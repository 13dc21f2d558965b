"""The B-row linear family (t2v_rowlin_fwd / _bwd_data / _wgrad, t2v_timestep_embedding_f32: csrc/full_grad.hip) on the host SIMT simulator:
the case table of tests/rowlin_cases.py — NaN-poisoned operand views, sentinel-guarded outputs, an fp64 reference with the derived
per-element bound, every case twice bit for bit, refusals — through the real C-ABI and the real ``native.HipOps`` wrappers."""
import os
import shutil
import sys

import pytest

from tests import rowlin_cases as rc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))


@pytest.fixture(scope="module")
def sim():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    return HostSimOps(hostsim_build.build())


@pytest.mark.parametrize("name", list(rc.LIN_CASES))
def test_rowlin_fwd(sim, name):
    rc.run_fwd(sim, "cpu", name)


@pytest.mark.parametrize("name", list(rc.BWD_CASES))
def test_rowlin_bwd_data(sim, name):
    rc.run_bwd(sim, "cpu", name)


@pytest.mark.parametrize("name", list(rc.LIN_CASES))
def test_rowlin_wgrad(sim, name):
    rc.run_wgrad(sim, "cpu", name)


@pytest.mark.parametrize("name", rc.REFUSALS)
def test_rowlin_refusals(sim, name):
    rc.run_refusal(sim, "cpu", name)


def test_timestep_embedding_f32(sim):
    rc.run_timestep_embedding_f32(sim, "cpu")


def test_dropout_f32(sim):
    rc.run_dropout_f32(sim, "cpu")


def test_the_new_entries_are_bound_and_named_in_the_replay_table():
    """What a recorded list needs of the new entries (the replay itself runs on the device, tests/test_gpu_rowlin.py): every one has a signature in ``native._SIGS`` with the stream last, so
    ``compile_recording`` can lay out its argument slots (csrc/replay.hip's table is checked against the library by tests/test_abi.py)."""
    from t2v_turbo_amd import native as nt
    for name in ("t2v_rowlin_fwd", "t2v_rowlin_bwd_data", "t2v_rowlin_wgrad", "t2v_timestep_embedding_f32", "t2v_dropout_f32"):
        assert name in nt.EXPORTED and nt._SIGS[name][1][-1] is nt.C.c_void_p
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "t2v-turbo_amd", "csrc", "replay.hip")).read()
    for name in ("t2v_rowlin_fwd", "t2v_rowlin_bwd_data", "t2v_rowlin_wgrad", "t2v_timestep_embedding_f32", "t2v_dropout_f32"):
        assert f"T2V_ENTRY({name})" in text
