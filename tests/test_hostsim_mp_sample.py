"""The motion-prior sampler's kernels (csrc/train.hip: ``t2v_mp_guided_step``; csrc/elementwise.hip: ``t2v_video_to_u8``) executed thread by
thread on the host SIMT simulator, through ``HostSimOps``: the case table and bounds of tests/mp_sample_cases.py.  The uint8 kernel lives
in csrc/elementwise.hip, which only the whole-library build of the simulator holds (tests/test_hostsim_full.py builds the same one)."""
import os
import shutil
import sys

import pytest
import torch

from tests import cd_head_cases as cc
from tests import mp_sample_cases as mc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))


@pytest.fixture(scope="module")
def sim():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    return HostSimOps(hostsim_build.build())


@pytest.fixture(scope="module")
def sim_full():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    return HostSimOps(hostsim_build.build_full())


@pytest.mark.parametrize("geom,i,dtype,with_score,with_x0,outs,lp,pd", mc.HEAD_PARAMS)
def test_guided_step_on_the_case_table(sim, geom, i, dtype, with_score, with_x0, outs, lp, pd):
    case = mc.head_case(geom, i, dtype, with_score, with_x0)
    first = mc.run_head(sim, "cpu", case, outs, cc.DTYPES[lp], cc.DTYPES[pd])
    assert all((first[k] is not None) == (c in outs) for k, c in (("x_lp", "l"), ("pred_x0", "p"), ("rec", "r")))
    mc.check_head(case, first)
    again = mc.run_head(sim, "cpu", case, outs, cc.DTYPES[lp], cc.DTYPES[pd])
    assert all(first[k] is None or mc.same_bits(first[k], again[k]) for k in first)


@pytest.mark.parametrize("dtype", list(cc.DTYPES))
@pytest.mark.parametrize("with_x0", [False, True])
def test_bases_off_a_16_byte_boundary_take_the_scalar_path(sim, dtype, with_x0):
    case = mc.head_case("misaligned", 24, dtype, True, with_x0)
    got = mc.run_head(sim, "cpu", case, "lpr", torch.bfloat16, cc.DTYPES[dtype], misalign=True)
    mc.check_head(case, got, " (unaligned)")
    # the scalar and the 16-byte paths round alike
    aligned = mc.run_head(sim, "cpu", case, "lpr", torch.bfloat16, cc.DTYPES[dtype])
    assert all(mc.same_bits(got[k], aligned[k]) for k in got)


def test_guided_step_refusals_return_the_error_codes_before_any_launch(sim):
    mc.check_head_refusals(sim, "cpu")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_uint8_equals_the_torch_expression_on_every_16_bit_pattern(sim_full, dtype):
    video = mc.u8_patterns(dtype)
    out = mc.run_u8(sim_full, "cpu", video)
    mc.check_u8(video, out, dtype)
    nan = torch.isnan(video.float()).permute(0, 2, 3, 4, 1)
    assert bool(nan.any()) and not bool(out[nan].any()), "NaN gives 0"
    assert mc.same_bits(out, mc.run_u8(sim_full, "cpu", video))


def test_uint8_on_the_fp32_boundary_values(sim_full):
    video = mc.u8_boundaries()
    mc.check_u8(video, mc.run_u8(sim_full, "cpu", video), "boundaries")


@pytest.mark.parametrize("dtype", list(cc.DTYPES))
def test_uint8_batch_frame_and_channel_addressing_and_a_misaligned_base(sim_full, dtype):
    video = mc.u8_batch(dtype)
    out = mc.run_u8(sim_full, "cpu", video)
    assert out.shape == (2, 3, 5, 7, 3)
    mc.check_u8(video, out, dtype)
    mc.check_u8(video, mc.run_u8(sim_full, "cpu", video, misalign=True), dtype + " (unaligned)")
    # H * W a multiple of 4 on aligned bases: every lane takes the 16-byte path
    wide = video[..., :4].contiguous()
    mc.check_u8(wide, mc.run_u8(sim_full, "cpu", wide), dtype + " (vector)")
    mc.check_u8(wide, mc.run_u8(sim_full, "cpu", wide, misalign=True), dtype + " (vector shape, unaligned)")


def test_uint8_refusals(sim_full):
    mc.check_u8_refusals(sim_full, "cpu")
