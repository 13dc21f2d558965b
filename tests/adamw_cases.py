"""One table of ``t2v_adamw_multi`` / ``t2v_sumsq_multi`` / ``t2v_scale_multi`` cases, shared by tests/test_hostsim_adamw.py (the kernel
source on the host SIMT simulator) and tests/test_gpu_optim_adamw.py (the device): tensor sizes around the lane, float4 and work-block
edges, tensors whose parameter, gradient or moments are views 4 bytes off 16-byte alignment (the kernels' scalar path), three hyper
rows in one launch, one parameter without a gradient.  All parameters sit in ONE arena, all gradients in another, each moment in its
own, with 64 guard floats before, between and after: a read past a gradient poisons the norm, a write past anything is seen bit for
bit."""
import numpy as np
import torch

from t2v_turbo_amd import native as nt
from t2v_turbo_amd.optim import AdamW, adamw_definition, adamw_table

B = nt.ADAMW_BLOCK
POISON = 0x7FC0DEAD            # a quiet NaN with a recognisable payload
GUARD = 64
RTOL, ATOL = 1e-6, 1e-7        # fp32 rounding: the constants of tests/optim8_util.py
# (elements, offsets from 16-byte alignment in elements of: parameter, gradient, exp_avg, exp_avg_sq)
CASES = [(1, 0, 0, 0, 0), (3, 0, 0, 0, 0), (4, 0, 0, 0, 0), (5, 0, 0, 0, 0), (255, 0, 0, 0, 0), (256, 0, 0, 0, 0), (257, 0, 0, 0, 0),
         (B - 1, 0, 0, 0, 0), (B, 0, 0, 0, 0), (B + 1, 0, 0, 0, 0), (3 * B + 5, 0, 0, 0, 0),
         (B + 1, 1, 0, 0, 0),            # the parameter 4 bytes off: scalar accesses
         (3 * B + 5, 0, 1, 0, 0),        # the gradient off
         (257, 0, 0, 0, 1),              # one moment off
         (5, 1, 1, 1, 1),                # all four off
         (B + 7, 0, 0, 0, 0)]            # the parameter WITHOUT a gradient
NO_GRAD = len(CASES) - 1
# (lr, weight_decay, beta1, beta2, eps), the step count BEFORE the step under test (the launch takes steps 4, 4 and 7)
ROWS = [((1e-3, 1e-2, 0.9, 0.999, 1e-8), 3), ((1e-5, 0.0, 0.9, 0.999, 1e-8), 3), ((2e-3, 1e-2, 0.8, 0.95, 1e-6), 6)]
GROUP_OF = [i % 3 for i in range(len(CASES))]   # tensor -> group (= hyper row)


def bits(x):
    return x.contiguous().view(torch.int32)


def _arena(sizes_offsets):
    """(poisoned fp32 CPU arena, [(start, n)], guard mask): every tensor starts ``off`` elements past a 16-byte boundary, ``GUARD``
    poisoned elements (at least) before the first, between neighbours and after the last."""
    spans, pos = [], GUARD
    for n, off in sizes_offsets:
        start = (pos + 3) // 4 * 4 + off
        spans.append((start, n))
        pos = start + n + GUARD
    arena = torch.zeros(pos)
    mask = torch.ones(pos, dtype=torch.bool)
    for start, n in spans:
        mask[start:start + n] = False
    arena.view(torch.int32)[mask] = POISON
    return arena, spans, mask


class AdamwCase:
    """The case list as an ``optim.AdamW`` over views of the four arenas on ``device``, warmed up to the step counts of ``ROWS``."""

    def __init__(self, device="cpu", seed=5, native_ops=None):
        gen = self.gen = torch.Generator().manual_seed(seed)
        arenas = {}
        for k, col in (("p", 1), ("g", 2), ("m", 3), ("v", 4)):
            arenas[k] = _arena([(c[0], c[col]) for c in CASES])
        for s, n in arenas["p"][1]:
            arenas["p"][0][s:s + n] = torch.randn(n, generator=gen) * 0.1
        for k in "mv":
            for s, n in arenas[k][1]:
                arenas[k][0][s:s + n] = 0.0

        def build(dev):
            self.arena = {k: a.to(dev) for k, (a, _, _) in arenas.items()}
            self.mask = {k: m.to(dev) for k, (_, _, m) in arenas.items()}
            view = lambda k, i: self.arena[k][arenas[k][1][i][0]:arenas[k][1][i][0] + arenas[k][1][i][1]]   # noqa: E731
            self.params = [torch.nn.Parameter(view("p", i)) for i in range(len(CASES))]
            for i, p in enumerate(self.params):
                if i != NO_GRAD:
                    p.grad = view("g", i)
            groups = [dict(params=[p for p, g in zip(self.params, GROUP_OF) if g == gi], lr=h[0], weight_decay=h[1], betas=(h[2], h[3]),
                           eps=h[4]) for gi, (h, _) in enumerate(ROWS)]
            opt = AdamW(groups)
            for i, p in enumerate(self.params):
                opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=view("m", i), exp_avg_sq=view("v", i))
            return opt

        # "a few warm-up steps" with the definition on the CPU: 3 for every tensor (the one without a gradient had one then), 3 more
        # for the third group
        opt = build("cpu")
        self.params[NO_GRAD].grad = torch.zeros(CASES[NO_GRAD][0])
        for s in range(6):
            for p, g in zip(self.params, GROUP_OF):
                p.grad = (torch.randn(p.numel(), generator=gen) * 0.3) if (s < 3 or g == 2) and p.grad is not None else None
            opt.step()
        steps = [float(opt.state[p]["step"]) for p in self.params]
        for k, (a, _, _) in arenas.items():
            a.copy_(self.arena[k])
        self.opt = build(device)
        self.opt.native_ops = native_ops
        for p, s in zip(self.params, steps):
            self.opt.state[p]["step"] = torch.tensor(s)
        self.new_grads()
        self.check_layout()

    def check_layout(self):
        for i, (c, p) in enumerate(zip(CASES, self.params)):
            st = self.opt.state[p]
            assert p.numel() == c[0] and p.data_ptr() % 16 == 4 * c[1] and st["exp_avg"].data_ptr() % 16 == 4 * c[3]
            assert st["exp_avg_sq"].data_ptr() % 16 == 4 * c[4] and float(st["step"]) == ROWS[GROUP_OF[i]][1]
            assert (p.grad is None) == (i == NO_GRAD) and (p.grad is None or p.grad.data_ptr() % 16 == 4 * c[2])

    def new_grads(self):
        for p in self.params:
            if p.grad is not None:
                p.grad.copy_((torch.randn(p.numel(), generator=self.gen) * 0.3).to(p.device))

    @property
    def active(self):
        return [i for i in range(len(CASES)) if i != NO_GRAD]

    def snapshot(self):
        return {k: a.clone() for k, a in self.arena.items()}

    def restore(self, snap):
        for k, a in self.arena.items():
            a.copy_(snap[k])

    def tensors(self, i):
        p = self.params[i]
        st = self.opt.state[p]
        return p.detach(), p.grad, st["exp_avg"], st["exp_avg_sq"]

    def check_guards(self, grads_equal_to=None):
        """Every guard float of the four arenas still holds the poison; with ``grads_equal_to`` (a snapshot) the whole gradient arena
        is bit-unchanged."""
        for k, a in self.arena.items():
            guards = bits(a)[self.mask[k]]
            assert guards.numel() >= GUARD * (len(CASES) + 1) and bool((guards == POISON).all()), f"a write outside a tensor of arena {k}"
        if grads_equal_to is not None:
            assert torch.equal(bits(self.arena["g"]), bits(grads_equal_to["g"])), "the gradients were written"

    def table(self):
        """The launch of the whole case list, made directly: (uint8 table on the device, tensors, work blocks, hyper rows for the step
        AFTER the current state, the tensor index of every record)."""
        order = sorted(self.active, key=lambda i: GROUP_OF[i])
        cols = list(zip(*[self.tensors(i) for i in order]))
        host, launches = adamw_table(list(cols[1]), list(cols[0]), list(cols[2]), list(cols[3]), [GROUP_OF[i] for i in order])
        (start, end, work, row0, n_rows), = launches
        assert (start, end, row0, n_rows) == (0, len(order), 0, 3) and work == sum((CASES[i][0] + B - 1) // B for i in order)
        hyper = [h + (s + 1,) for h, s in ROWS]
        return torch.from_numpy(host.view(np.uint8).copy()).to(self.arena["p"].device), len(order), work, hyper, order

    def definition(self, snap, i, grad_scale=1.0, step=None):
        """(param, exp_avg, exp_avg_sq) of tensor ``i`` after one step of the torch definition from the state in ``snap``."""
        p, g, m, v = (self._span(snap, k, i).cpu().clone() for k in "pgmv")
        h, s = ROWS[GROUP_OF[i]]
        m, v = adamw_definition(p, g, m, v, h[0], (h[2], h[3]), h[4], h[1], s + 1 if step is None else step, grad_scale)
        return p, m, v

    def check_against_definition(self, snap, grad_scale=1.0, steps=None, label=""):
        """After one step from ``snap``: the moments bit-equal to the definition (they are only products and sums with contraction
        off), the parameters within fp32 rounding."""
        for i in self.active:
            p, m, v = self.definition(snap, i, grad_scale, None if steps is None else steps[i])
            tp, _, tm, tv = (t.detach().cpu() for t in self.tensors(i))
            assert torch.equal(bits(tm), bits(m)) and torch.equal(bits(tv), bits(v)), (label, CASES[i])
            assert torch.allclose(tp, p, rtol=RTOL, atol=ATOL), (label, CASES[i], float((tp - p).abs().max()))
            assert not torch.equal(tp, self._span(snap, "p", i).cpu()), (label, CASES[i])

    def _span(self, snap, k, i):
        """Tensor ``i`` of arena ``k`` as it was in the snapshot."""
        t = self.tensors(i)["pgmv".index(k)]
        off = (t.data_ptr() - self.arena[k].data_ptr()) // 4
        return snap[k][off:off + t.numel()]

    def no_grad_unchanged(self, snap, step):
        p = self.params[NO_GRAD]
        return torch.equal(bits(p.detach()), bits(self._span(snap, "p", NO_GRAD))) and float(self.opt.state[p]["step"]) == step


def adamw8_f32_state(ops, case, snap, grad_scale):
    """{tensor: (param, exp_avg, exp_avg_sq)} after ``t2v_adamw8_step`` on COPIES of the snapshot's data, every tensor under
    T2V_ADAMW8_F32_STATE (fp32 moments in an arena padded to whole 256-element blocks), one launch per hyper row."""
    from t2v_turbo_amd.optim import QBLOCK, adamw8_table, make_code_books, work_blocks
    dev = case.arena["p"].device
    code1, code2 = (c.to(dev) for c in make_code_books())
    got = {}
    for row, (h, step0) in enumerate(ROWS):
        idx = [i for i in case.active if GROUP_OF[i] == row]
        p = [case._span(snap, "p", i).clone() for i in idx]
        g = [case._span(snap, "g", i).clone() for i in idx]
        first, total = work_blocks([CASES[i][0] for i in idx], QBLOCK)   # every tensor's first block in the state arena: its work0 too
        f1, f2 = torch.zeros(total * QBLOCK, device=dev), torch.zeros(total * QBLOCK, device=dev)
        spans = [slice(int(b0) * QBLOCK, int(b0) * QBLOCK + CASES[i][0]) for b0, i in zip(first, idx)]
        for sp, i in zip(spans, idx):
            f1[sp] = case._span(snap, "m", i)
            f2[sp] = case._span(snap, "v", i)
        host, ((_, _, work),) = adamw8_table(p, g, first, True, lr=h[0], weight_decay=h[1])
        assert work == total and np.array_equal(host["work0"], first)
        table = torch.from_numpy(host.view(np.uint8).copy()).to(dev)
        ops.adamw8_step(table, len(idx), work, None, None, None, None, f1, f2, code1, code2, h[2], h[3], h[4], step0 + 1, grad_scale)
        for sp, pj, i in zip(spans, p, idx):
            got[i] = (pj, f1[sp].clone(), f2[sp].clone())
    return got


def check_against_adamw8(ops, case, snap, grad_scale):
    """After one ``adamw_multi`` over ``case.table()`` from ``snap``: parameter and both moments bit-identical to the fp32-state branch
    of ``t2v_adamw8_step`` — the same build, the same expressions, so nothing but equality is acceptable."""
    want = adamw8_f32_state(ops, case, snap, grad_scale)
    for i in case.active:
        tp, _, tm, tv = case.tensors(i)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), (tp, tm, tv), want[i]):
            assert torch.equal(bits(a), bits(b)), (CASES[i], name)


def many_groups(device="cpu", native_ops=None, seed=6):
    """17 groups of tiny tensors with 17 distinct learning rates: more hyper rows than one launch takes."""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter((torch.randn(1 + 3 * i, generator=gen) * 0.1).to(device)) for i in range(17)]
    for p in params:
        p.grad = (torch.randn(p.numel(), generator=gen) * 0.3).to(device)
    opt = AdamW([dict(params=[p], lr=1e-3 * (1 + i)) for i, p in enumerate(params)], weight_decay=1e-2)
    opt.native_ops = native_ops
    return opt, params


def twin_step(opt, grad_scale=1.0):
    """What the torch definition makes of ``opt``'s next step, from ``opt``'s present state: {parameter: (param, exp_avg, exp_avg_sq)}
    as CPU tensors.  Call BEFORE ``opt.step()``."""
    want = {}
    for g in opt.param_groups:
        for p in g["params"]:
            if p.grad is None:
                continue
            st = opt.state.get(p) or dict(step=torch.tensor(0.0), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
            pf = p.detach().cpu().clone().view(-1)
            m, v = adamw_definition(pf, p.grad.detach().cpu().reshape(-1), st["exp_avg"].cpu().reshape(-1), st["exp_avg_sq"].cpu().reshape(-1),
                                    float(g["lr"]), g["betas"], g["eps"], g["weight_decay"], int(st["step"]) + 1, grad_scale)
            want[p] = (pf, m, v)
    return want


def check_twin(opt, want, label=""):
    for p, (pf, m, v) in want.items():
        st = opt.state[p]
        assert torch.equal(bits(st["exp_avg"].cpu().reshape(-1)), bits(m)), (label, tuple(p.shape), "exp_avg")
        assert torch.equal(bits(st["exp_avg_sq"].cpu().reshape(-1)), bits(v)), (label, tuple(p.shape), "exp_avg_sq")
        got = p.detach().cpu().reshape(-1)
        assert torch.allclose(got, pf, rtol=RTOL, atol=ATOL), (label, tuple(p.shape), float((got - pf).abs().max()))


def norm_bound(k=23):
    """Relative error allowed between the kernel's sum of squares and the float64 one: (k + 2) * 2**-24, doubled for margin.  k = 23
    is the longest chain of fp32 additions in a block partial of ``sumsq_multi_kernel``: 15 serial additions of a lane's 16 squares,
    6 levels of the wave shuffle tree, 2 levels over the four waves; the finishing sum is in double."""
    return 2 * (k + 2) * 2.0 ** -24
