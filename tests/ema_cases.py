"""One table of ``t2v_ema_multi`` cases, shared by tests/test_hostsim_ema.py (the kernel source on the host SIMT simulator) and
tests/test_gpu_ema_target.py (the device): tensor sizes around the lane, workgroup and work-block edges, targets and sources that are
views 4 bytes (fp32) / 2 bytes (bf16) off 16-byte alignment (the kernel's scalar path), bf16 sources — all targets in ONE arena with
64 poisoned floats between neighbours, so that a write outside ``[target, target + n)`` is seen."""
import numpy as np
import torch

from t2v_turbo_amd import native as nt
from t2v_turbo_amd.optim import ema_table

B = nt.EMA_BLOCK
POISON = 0x7FC0DEAD            # a quiet NaN with a recognisable payload
GUARD = 64
RATE = 0.95                    # (the rate of tests/test_gpu_engine.py::test_flat_adamw_and_ema_kernels_match_torch, whose tolerance is used)
# (elements, target offset from 16-byte alignment in elements, source offset in elements, source dtype)
CASES = [(1, 0, 0, torch.float32), (255, 0, 0, torch.float32), (256, 0, 0, torch.float32), (257, 0, 0, torch.float32),
         (4097, 0, 0, torch.float32), (3 * B + 5, 0, 0, torch.float32),
         (4097, 1, 0, torch.float32),            # the target 4 bytes off: scalar accesses
         (3 * B + 5, 0, 1, torch.float32),       # the source 4 bytes off
         (257, 1, 1, torch.float32),
         (3 * B + 5, 0, 0, torch.bfloat16), (255, 0, 0, torch.bfloat16), (1, 0, 0, torch.bfloat16),
         (4097, 1, 0, torch.bfloat16),           # bf16 source, scalar path
         (2 * B + 9, 0, 1, torch.bfloat16)]      # bf16 source 2 bytes off


def _arena(sizes_offsets, dtype, device, gen):
    """One poisoned arena -> (arena, [(start, n)]): every tensor starts ``off`` elements past a 16-byte boundary, ``GUARD`` poisoned
    elements (at least) before the first, between neighbours and after the last."""
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    spans, pos = [], GUARD
    for n, off in sizes_offsets:
        start = (pos + per16 - 1) // per16 * per16 + off
        spans.append((start, n))
        pos = start + n + GUARD
    arena = torch.zeros(pos, dtype=dtype)
    for start, n in spans:
        arena[start:start + n] = torch.randn(n, generator=gen).to(dtype)
    return arena.to(device), spans


def _poison(arena, spans):
    bits = arena.view(torch.int32 if arena.dtype == torch.float32 else torch.int16)
    mask = torch.ones(arena.numel(), dtype=torch.bool, device=arena.device)
    for start, n in spans:
        mask[start:start + n] = False
    bits[mask] = POISON if arena.dtype == torch.float32 else (POISON >> 16)
    return mask


class EmaCase:
    def __init__(self, device="cpu", seed=11):
        gen = torch.Generator().manual_seed(seed)
        self.t_arena, self.t_spans = _arena([(n, to) for n, to, _, _ in CASES], torch.float32, device, gen)
        self.s32_arena, s32 = _arena([(n, so) for n, _, so, dt in CASES if dt == torch.float32], torch.float32, device, gen)
        self.s16_arena, s16 = _arena([(n, so) for n, _, so, dt in CASES if dt == torch.bfloat16], torch.bfloat16, device, gen)
        self.t_mask = _poison(self.t_arena, self.t_spans)
        _poison(self.s32_arena, s32)
        _poison(self.s16_arena, s16)
        assert self.t_arena.data_ptr() % 16 == 0 and self.s32_arena.data_ptr() % 16 == 0 and self.s16_arena.data_ptr() % 16 == 0
        self.targets = [self.t_arena[a:a + n] for a, n in self.t_spans]
        it32, it16 = iter(s32), iter(s16)
        self.sources = []
        for _, _, _, dt in CASES:
            a, n = next(it32 if dt == torch.float32 else it16)
            self.sources.append((self.s32_arena if dt == torch.float32 else self.s16_arena)[a:a + n])
        for (n, to, so, dt), t, s in zip(CASES, self.targets, self.sources):
            assert t.numel() == s.numel() == n and s.dtype == dt
            assert t.data_ptr() % 16 == 4 * to and s.data_ptr() % 16 == s.element_size() * so
        self.before = [t.clone() for t in self.targets]
        self.sources_before = (self.s32_arena.clone(), self.s16_arena.clone())

    def table(self):
        """(uint8 tensor of the records on the tensors' device, number of tensors, work blocks)."""
        host, work = ema_table(self.targets, self.sources)
        assert work == sum((n + B - 1) // B for n, _, _, _ in CASES)
        return torch.from_numpy(host.view(np.uint8).copy()).to(self.t_arena.device), len(self.targets), work

    def check(self, ops):
        """After ONE ``ops.ema_multi`` over ``table()``: every tensor bit-identical to ``ops.ema_update`` (the single-buffer kernel of the
        same build) on a copy (a bf16 source widened first), within the single-buffer kernel's tolerance of the torch expression, every
        poisoned element and every source bit-unchanged."""
        bits = lambda x: x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)   # noqa: E731
        for case, t, s, b in zip(CASES, self.targets, self.sources, self.before):
            want = b.clone()
            ops.ema_update(want, s.float().contiguous(), RATE)
            assert torch.equal(bits(t.contiguous()), bits(want)), case
            ref = b * RATE + s.float() * (1 - RATE)
            assert torch.allclose(t, ref, rtol=1e-6, atol=1e-7), case
            assert not torch.equal(t, b), case
        guards = bits(self.t_arena)[self.t_mask]
        assert guards.numel() >= GUARD * (len(CASES) + 1) and bool((guards == POISON).all()), "a write outside [target, target + n)"
        assert torch.equal(bits(self.s32_arena), bits(self.sources_before[0])) and torch.equal(bits(self.s16_arena), bits(self.sources_before[1]))
