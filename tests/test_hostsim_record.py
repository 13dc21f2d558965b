"""The record-producer kernels of csrc/train.hip (``t2v_cd_add_noise``, ``t2v_ddim_reverse_step``, ``t2v_pack_f16_multi``) executed thread by
thread on the host SIMT simulator, through ``HostSimOps``: the case table and bounds of tests/record_cases.py."""
import os
import shutil
import sys

import pytest
import torch

from tests import cd_head_cases as cc
from tests import record_cases as rc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))


@pytest.fixture(scope="module")
def sim():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import build as hostsim_build
    from tests.test_hostsim_kernels import HostSimOps
    return HostSimOps(hostsim_build.build())


@pytest.mark.parametrize("geom,in_dtype,lp_dtype", rc.ADD_NOISE_PARAMS)
def test_add_noise_on_the_case_table(sim, geom, in_dtype, lp_dtype):
    case = rc.add_noise_case(geom, in_dtype)
    z, z_lp = rc.run_add_noise(sim, "cpu", case, cc.DTYPES[lp_dtype])
    rc.check_add_noise(case, z, z_lp)
    z2, z_lp2 = rc.run_add_noise(sim, "cpu", case, cc.DTYPES[lp_dtype])
    assert rc.same_bits(z, z2) and rc.same_bits(z_lp, z_lp2)


def test_add_noise_without_the_copy_and_with_mixed_input_dtypes(sim):
    case = rc.add_noise_case("misaligned", "bf16")
    z, z_lp = rc.run_add_noise(sim, "cpu", case, None)
    assert z_lp is None
    rc.check_add_noise(case, z, None)
    # bf16 latents with fp32 noise (the same values): the same result
    z32, _ = rc.run_add_noise(sim, "cpu", case, None, noise=case["noise"].float())
    assert rc.same_bits(z, z32)


@pytest.mark.parametrize("geom,i,eps_dtype,with_prev", rc.REVERSE_PARAMS)
def test_reverse_step_on_the_case_table(sim, geom, i, eps_dtype, with_prev):
    case = rc.reverse_case(geom, i, eps_dtype)
    first = rc.run_reverse(sim, "cpu", case, with_prev, torch.bfloat16 if eps_dtype == "bf16" else torch.float16)
    rc.check_reverse(case, *first)
    again = rc.run_reverse(sim, "cpu", case, with_prev, torch.bfloat16 if eps_dtype == "bf16" else torch.float16)
    assert all(a is None or rc.same_bits(a, b) for a, b in zip(first, again))


def test_reverse_step_without_the_copy(sim):
    case = rc.reverse_case("misaligned", 24, "fp32")
    x, prev, x_lp = rc.run_reverse(sim, "cpu", case, True, None)
    assert x_lp is None
    rc.check_reverse(case, x, prev, None)


@pytest.mark.parametrize("in_dtype", list(cc.DTYPES))
def test_bases_off_a_16_byte_boundary_take_the_scalar_path(sim, in_dtype):
    case = rc.add_noise_case("misaligned", in_dtype)
    rc.check_add_noise(case, *rc.run_add_noise(sim, "cpu", case, torch.bfloat16, misalign=True), " (unaligned)")
    rcase = rc.reverse_case("misaligned", 24, "fp32" if in_dtype == "fp32" else "bf16")
    rc.check_reverse(rcase, *rc.run_reverse(sim, "cpu", rcase, True, misalign=True), " (unaligned)")


def test_an_index_outside_the_tables_behaves_as_the_nearest_valid_one(sim):
    case = rc.add_noise_case("tail", "fp32")
    hi = rc.run_add_noise(sim, "cpu", dict(case, index=torch.tensor([49])), torch.bfloat16)
    assert all(rc.same_bits(a, b) for a, b in zip(rc.run_add_noise(sim, "cpu", dict(case, index=torch.tensor([1 << 40])), torch.bfloat16), hi))
    lo = rc.run_add_noise(sim, "cpu", dict(case, index=torch.tensor([0])), torch.bfloat16)
    assert all(rc.same_bits(a, b) for a, b in zip(rc.run_add_noise(sim, "cpu", dict(case, index=torch.tensor([-7])), torch.bfloat16), lo))
    # the reverse step: index 1 << 40 is index 49 (step 30 is taken), index -7 is index 0 (step 0 is the clip's last, step 1 is not taken)
    for i, far, near in ((30, 1 << 40, 49), (0, -7, 0), (1, -7, 0)):
        a = rc.run_reverse(sim, "cpu", rc.reverse_case("tail", i, "fp32", index=(far,)), True)
        b = rc.run_reverse(sim, "cpu", rc.reverse_case("tail", i, "fp32", index=(near,)), True)
        rc.check_reverse(rc.reverse_case("tail", i, "fp32", index=(far,)), *a)
        assert all(rc.same_bits(u, v) for u, v in zip(a, b))


def test_pack_equals_the_torch_conversion_bit_for_bit(sim):
    dst, spans = rc.run_pack(sim, "cpu")
    rc.check_pack(dst, spans)
    dst2, _ = rc.run_pack(sim, "cpu")
    assert rc.same_bits(dst, dst2)
    # another phase of the destination against the 16-byte grid, and entries that touch
    for first_off, gap in ((0, 0), (5, 1), (8, 0)):
        d, s = rc.run_pack(sim, "cpu", gap=gap, first_off=first_off)
        rc.check_pack(d, s)


def test_pack_rows_into_a_clip_by_clip_layout(sim):
    assert rc.same_bits(rc.run_pack_rows(sim, "cpu"), rc.run_pack_rows(sim, "cpu"))


def test_refusals_return_the_error_codes_before_any_launch(sim):
    rc.check_refusals(sim, "cpu")
