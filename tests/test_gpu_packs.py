"""The Packer's refresh on the device: bf16 packs re-filled through ``HipOps`` — the smallest case that runs t2v_transpose_bf16 and
t2v_repack_conv_f32 from the entries' own ``into`` writers — against a fresh Packer over the moved parameters (tests/packs_cases.py).
Eager; the captured refresh is covered by tests/test_gpu_train_parity.py and tests/test_gpu_full_ckpt.py."""
import pytest
import torch

from tests.packs_cases import check_refresh_equals_fresh

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("order", ["sources_first", "dependants_first"])
def test_refresh_equals_a_fresh_packer_on_device(order):
    from t2v_turbo_amd.native import HipOps
    ops = HipOps()
    calls = []
    for name in ("transpose", "repack_conv"):
        def counted(*a, _fn=getattr(ops, name), _name=name, **k):
            calls.append(_name)
            return _fn(*a, **k)
        setattr(ops, name, counted)
    check_refresh_equals_fresh(torch.device("cuda", 0), torch.bfloat16, ops, order)
    torch.cuda.synchronize()
    # mat_t from the refreshed mat; conv (2-D and temporal), conv_dgrad x 2 (the 64- and the 4-channel conv) and tconv_dgrad repacked
    assert sorted(calls) == ["repack_conv"] * 5 + ["transpose"]
