"""One outstanding tape per input shape: a second grad-mode forward of the same shape overwrites what the first one saved, so the
backward of the first output is refused and the backward of the second runs.  The three UNet routes through the module call
(emulated ops behind the record / replay protocol), and the VAE decode gradient engine by its tokens."""
import pytest
import torch

from tests.emu_ops import EmuOps, ReplayOps
from tests.util import load


def _full():
    from tests.test_unet_full_grad_cpu import _student
    return _student(), "train"


def _lora():
    from tests.test_unet_lora_grad_cpu import _student
    return _student("unet_tiny", 64)[0], "train"


def _frozen():
    from tests.test_input_grad_route_cpu import _frozen
    return _frozen(), "input_grad"


@pytest.mark.parametrize("make", [_full, _lora, _frozen], ids=["train_full", "train", "input_grad"])
def test_backward_of_an_overwritten_forward_is_refused_and_the_next_one_runs(make):
    g = load("unet_tiny")
    m, mode = make()
    m._native_ops_factory = lambda: ReplayOps(EmuOps(strict=True))
    m.native_mode = mode
    xs = [g["x"].clone().requires_grad_(True) for _ in range(2)]
    ys = [m(x, g["ts"], context=g["ctx"], fps=16, timestep_cond=g["tc"]) for x in xs]
    with pytest.raises(RuntimeError, match="another grad-mode forward of the same shape"):
        ys[0].sum().backward()
    ys[1].sum().backward()
    assert xs[0].grad is None and torch.isfinite(xs[1].grad).all() and float(xs[1].grad.abs().max()) > 0


def test_vae_decode_gradient_engine_refuses_the_token_of_an_overwritten_decode():
    from oracle import synth
    from t2v_turbo_amd.engine_vae_bwd import VAEDecodeGradEngine
    from t2v_turbo_amd.vae import AutoencoderKL
    from tests.util import VAE_TINY_DD
    ae = AutoencoderKL(ddconfig=dict(VAE_TINY_DD), embed_dim=4).eval()
    ae.load_state_dict(synth.synth_state_dict(synth.manifest_of(ae)))
    z = torch.randn(1, 4, 1, 8, 8, generator=torch.Generator().manual_seed(3))
    eng = VAEDecodeGradEngine(ae, ReplayOps(EmuOps()))
    tokens = []
    for _ in range(2):
        v = eng.decode_frames_tape(z, 1.0)
        tokens.append(eng.tape_token)
    with pytest.raises(RuntimeError, match="keeps ONE outstanding decode per input shape"):
        eng.backward(torch.ones_like(v), token=tokens[0])
    dz = eng.backward(torch.ones_like(v), token=tokens[1])
    assert dz.shape == z.shape and torch.isfinite(dz).all() and float(dz.abs().max()) > 0
