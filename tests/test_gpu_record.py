"""-m gpu: the record-producer kernels on the device — the case table and bounds of tests/record_cases.py (shared with the host-simulator
test) — and ``preprocess.make_latent_records`` on the tiny bf16 UNet against the record the REFERENCE computed in fp32
(tests/golden/record_tiny.npz).

Bounds of the producer against the fixture, for the native path and for ``T2V_NATIVE_RECORD=0`` alike:
  * z_t: per element ulp_fp16 / 2 + 1e-5 * max |ref| (fp32 arithmetic and one fp16 rounding: tests/test_record_producer_cpu.py);
  * cond_teacher_out, uncond_teacher_out: rel-L2 < E2E_TOL (tests/test_gpu_engine.py: the bf16 engine against the fp32 reference);
  * score: rel-L2 < 0.15 (``test_ddim_inversion_and_motion_prior_score_on_device``: the same loss on bf16 probabilities);
  * z_example, z_example_prev: e_new <= 1.1 * e_old + 2^-11, with e_new the rel-L2 against the fixture and e_old the same number for
    the existing ``motion_prior.reverse_ddim_loop`` on the same inputs in this test — the new path rounds the state less often, so it
    should be no further from the fp32 reference; 10 % for rounding points that fall differently, 2^-11 for the record's fp16 rounding;
  * the clip with index 0: z_example_prev is its fp16-rounded input latent, bit for bit."""
import copy
import os
import warnings

import pytest
import torch

from t2v_turbo_amd import cd_math, latent_io, preprocess
from t2v_turbo_amd import native as nt
from t2v_turbo_amd.scheduler import T2VTurboScheduler
from tests import cd_head_cases as cc
from tests import record_cases as rc
from tests.test_record_producer_cpu import TENSORS, check_against_fixture, golden_inputs
from tests.util import rel_l2, tiny_unet_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return nt.HipOps()


# --------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("geom,in_dtype,lp_dtype", rc.ADD_NOISE_PARAMS)
def test_add_noise_on_the_case_table(ops, geom, in_dtype, lp_dtype):
    case = rc.add_noise_case(geom, in_dtype)
    z, z_lp = rc.run_add_noise(ops, "cuda", case, cc.DTYPES[lp_dtype])
    rc.check_add_noise(case, z, z_lp)
    z2, z_lp2 = rc.run_add_noise(ops, "cuda", case, cc.DTYPES[lp_dtype])
    assert rc.same_bits(z, z2) and rc.same_bits(z_lp, z_lp2)


def test_add_noise_without_the_copy_and_with_mixed_input_dtypes(ops):
    case = rc.add_noise_case("misaligned", "bf16")
    z, z_lp = rc.run_add_noise(ops, "cuda", case, None)
    assert z_lp is None
    rc.check_add_noise(case, z, None)
    z32, _ = rc.run_add_noise(ops, "cuda", case, None, noise=case["noise"].float())
    assert rc.same_bits(z, z32)


@pytest.mark.parametrize("geom,i,eps_dtype,with_prev", rc.REVERSE_PARAMS)
def test_reverse_step_on_the_case_table(ops, geom, i, eps_dtype, with_prev):
    case = rc.reverse_case(geom, i, eps_dtype)
    lp = torch.bfloat16 if eps_dtype == "bf16" else torch.float16
    first = rc.run_reverse(ops, "cuda", case, with_prev, lp)
    rc.check_reverse(case, *first)
    again = rc.run_reverse(ops, "cuda", case, with_prev, lp)
    assert all(a is None or rc.same_bits(a, b) for a, b in zip(first, again))


def test_reverse_step_without_the_copy(ops):
    case = rc.reverse_case("misaligned", 24, "fp32")
    x, prev, x_lp = rc.run_reverse(ops, "cuda", case, True, None)
    assert x_lp is None
    rc.check_reverse(case, x, prev, None)


@pytest.mark.parametrize("in_dtype", list(cc.DTYPES))
def test_bases_off_a_16_byte_boundary_take_the_scalar_path(ops, in_dtype):
    case = rc.add_noise_case("misaligned", in_dtype)
    rc.check_add_noise(case, *rc.run_add_noise(ops, "cuda", case, torch.bfloat16, misalign=True), " (unaligned)")
    rcase = rc.reverse_case("misaligned", 24, "fp32" if in_dtype == "fp32" else "bf16")
    rc.check_reverse(rcase, *rc.run_reverse(ops, "cuda", rcase, True, misalign=True), " (unaligned)")


def test_an_index_outside_the_tables_behaves_as_the_nearest_valid_one(ops):
    case = rc.add_noise_case("tail", "fp32")
    for far, near in ((1 << 40, 49), (-7, 0)):
        a = rc.run_add_noise(ops, "cuda", dict(case, index=torch.tensor([far])), torch.bfloat16)
        b = rc.run_add_noise(ops, "cuda", dict(case, index=torch.tensor([near])), torch.bfloat16)
        assert all(rc.same_bits(u, v) for u, v in zip(a, b))
    for i, far, near in ((30, 1 << 40, 49), (0, -7, 0), (1, -7, 0)):
        a = rc.run_reverse(ops, "cuda", rc.reverse_case("tail", i, "fp32", index=(far,)), True)
        b = rc.run_reverse(ops, "cuda", rc.reverse_case("tail", i, "fp32", index=(near,)), True)
        rc.check_reverse(rc.reverse_case("tail", i, "fp32", index=(far,)), *a)
        assert all(rc.same_bits(u, v) for u, v in zip(a, b))


def test_pack_equals_the_torch_conversion_bit_for_bit(ops):
    dst, spans = rc.run_pack(ops, "cuda")
    rc.check_pack(dst, spans)
    dst2, _ = rc.run_pack(ops, "cuda")
    assert rc.same_bits(dst, dst2)
    for first_off, gap in ((0, 0), (5, 1), (8, 0)):
        d, s = rc.run_pack(ops, "cuda", gap=gap, first_off=first_off)
        rc.check_pack(d, s)


def test_pack_rows_into_a_clip_by_clip_layout(ops):
    assert rc.same_bits(rc.run_pack_rows(ops, "cuda"), rc.run_pack_rows(ops, "cuda"))


def test_refusals_return_the_error_codes_before_any_launch(ops):
    rc.check_refusals(ops, "cuda")
    acp, solver = cc.schedule()
    x = torch.randn(2, 40, device="cuda")
    sched = ops.cd_sched(acp.cuda(), solver.ddim_timesteps.cuda(), solver.ddim_alpha_cumprods_prev.float().cuda(), torch.tensor([3, 4], device="cuda"),
                         0, 1.0)
    for call in (lambda: ops.cd_add_noise(sched, x.double(), x.double(), x.clone()),                      # dtype code
                 lambda: ops.ddim_reverse_step(sched, 50, 20, x.clone(), x),                               # step outside the grid
                 lambda: ops.ddim_reverse_step(sched, 1, 20, x.clone(), x.half()),                         # eps fp16
                 lambda: ops.pack_f16_multi([(x, 41)], torch.empty(80, dtype=torch.float16, device="cuda"))):   # past the end
        with pytest.raises(nt.NativeError):
            call()


# --------------------------------------------------------------------------------------------------------------- the producer
@pytest.fixture(scope="module")
def produced():
    """(fixture, records of the native path, records with T2V_NATIVE_RECORD=0, z_example / z_example_prev of the existing loop)."""
    from t2v_turbo_amd import motion_prior as mp
    from tests.test_gpu_engine import _unet
    m = _unet(tiny_unet_params(record_attn_probs=True), "unet_tiny", torch.bfloat16)
    m.dtype = torch.bfloat16
    m.requires_grad_(False)
    dev = torch.device("cuda", 0)
    sched = T2VTurboScheduler(linear_start=0.00085, linear_end=0.012)
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=50)
    g, inputs = golden_inputs("cuda")
    kw = dict(motion=True, fps=int(g["fps"]), temp_loss_scale=float(g["temp_loss_scale"]), rng=dict(index=g["index"], noise=g["noise"]))
    ops = preprocess_ops()
    calls = {"cd_add_noise": 0, "ddim_reverse_step": 0, "pack_f16_multi": 0}
    real = {name: getattr(ops, name) for name in calls}
    for name in calls:
        setattr(ops, name, (lambda nm: lambda *a, **k: (calls.__setitem__(nm, calls[nm] + 1), real[nm](*a, **k))[1])(name))
    out = {}
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)          # the composite UNet path must not be taken
            out["native"] = preprocess.make_latent_records(m, solver, sched, **inputs, **kw)
        native_calls = dict(calls)
        os.environ["T2V_NATIVE_RECORD"] = "0"
        try:
            out["twin"] = preprocess.make_latent_records(m, solver, sched, **inputs, **kw)
        finally:
            del os.environ["T2V_NATIVE_RECORD"]
        assert calls == native_calls, "T2V_NATIVE_RECORD=0 launched a record kernel"
        # the existing loop on the same inputs, one clip per call as the script runs it
        view = copy.copy(solver).to(dev)
        old_ex, old_prev = [], []
        for b in range(2):
            lat = inputs["latents"][b:b + 1].bfloat16()
            ctx = {"context": inputs["prompt_embeds"][b:b + 1].bfloat16(), "fps": kw["fps"]}
            inter = mp.reverse_ddim_loop(lat, m, ctx, view, int(g["index"][b]) + 1, dev)
            old_ex.append(inter[-1].float().cpu())
            old_prev.append((inter[-2] if int(g["index"][b]) > 0 else lat).float().cpu())
    finally:
        for name in calls:
            delattr(ops, name)
    torch.cuda.synchronize()
    return g, out, native_calls, (torch.cat(old_ex), torch.cat(old_prev)), m


def preprocess_ops():
    return nt.shared_ops()


def _stack(blobs):
    recs = [latent_io.unpack_latent_record(b) for b in blobs]
    return {k: torch.stack([r[k] for r in recs]) for k in latent_io.RECORD_KEYS}, recs


@pytest.mark.parametrize("path", ["native", "twin"])
def test_producer_on_the_device_against_the_reference_record(produced, path):
    """Measured on MI355X (this test prints the figures), native / ``T2V_NATIVE_RECORD=0``: cond_teacher_out 2.17e-2 / 2.17e-2,
    uncond_teacher_out 2.11e-2 / 2.11e-2, score 9.05e-2 / 9.08e-2; z_example e_new 2.14e-3 / 2.71e-3 against e_old 2.70e-3 (bound
    3.46e-3); z_example_prev e_new 1.64e-3 / 2.01e-3 against e_old 2.32e-3 (bound 3.04e-3)."""
    from tests.test_gpu_engine import E2E_TOL
    g, out, native_calls, (old_ex, old_prev), _ = produced
    blobs, info = out[path]
    assert info["native"] is (path == "native") and len(blobs) == 2
    if path == "native":
        # four inversion steps for index [3, 0]: one launch each, one add_noise, one pack, one copy
        assert native_calls == {"cd_add_noise": 1, "ddim_reverse_step": 4, "pack_f16_multi": 1}, native_calls
        assert info["device_to_host_copies"] == 1 and info["forwards"] == 4 + 1 + 2
    rec, recs = _stack(blobs)
    assert torch.equal(rec["index"], g["index"]) and all(r["index"].dim() == 0 and r["index"].dtype == torch.int64 for r in recs)
    for k in TENSORS:
        assert rec[k].dtype == torch.float16 and rec[k].device.type == "cpu" and bool(torch.isfinite(rec[k]).all()), k
    for b, blob in enumerate(blobs):
        assert len(blob) <= 2 * sum(recs[b][k].numel() for k in TENSORS) + 8192
    check_against_fixture(f"z_t ({path})", rec["z_t"], g["z_t"])
    check_against_fixture(f"prompt_emb ({path})", rec["prompt_emb"], g["prompt_emb"])
    e_c, e_u = rel_l2(rec["cond_teacher_out"].float(), g["cond_teacher_out"]), rel_l2(rec["uncond_teacher_out"].float(), g["uncond_teacher_out"])
    e_s = rel_l2(rec["score"].float(), g["score"])
    print(f"{path}: cond_teacher_out {e_c:.3e}, uncond_teacher_out {e_u:.3e} (bound {E2E_TOL:.0e}); score {e_s:.3e} (bound 0.15)")
    assert e_c < E2E_TOL and e_u < E2E_TOL and e_s < 0.15
    for k, old in (("z_example", old_ex), ("z_example_prev", old_prev)):
        e_new, e_old = rel_l2(rec[k].float(), g[k]), rel_l2(old, g[k])
        print(f"{path}: {k} e_new {e_new:.4e}, e_old (motion_prior.reverse_ddim_loop) {e_old:.4e}, bound {1.1 * e_old + 2.0 ** -11:.4e}")
        assert e_new <= 1.1 * e_old + 2.0 ** -11, (k, e_new, e_old)
    assert rc.same_bits(rec["z_example_prev"][1], g["latents"][1].half()), "index 0: z_example_prev is the input latent"


def test_one_v2_step_trains_on_the_produced_records(produced):
    from t2v_turbo_amd.distill import distill_step_v2
    from tests.test_unet_full_grad_cpu import _student
    g, out, _, _, _ = produced
    rec, _ = _stack(out["native"][0])
    batch = dict(rec, use_motion_guide=torch.tensor([True, True]), txt=["a cat", "a dog"])
    student = _student("unet_tiny").cuda().requires_grad_(True)
    sched = T2VTurboScheduler(linear_start=0.00085, linear_end=0.012)
    solver = cd_math.DDIMSolver(sched.alphas_cumprod.numpy(), ddim_timesteps=50)
    loss, info = distill_step_v2(student, solver, sched, batch, optimizer=None, topk=20, motion_gs=0.8, percentage=0.5, fps=int(g["fps"]),
                                 weight_dtype=torch.bfloat16, rng=dict(w=torch.tensor([6.0, 11.5])))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0 and bool(torch.isfinite(info["x_prev"]).all())
