"""Helpers of the native-conditioning tests (CPU and device): the emulated op backend with the three B-row entries written out in torch
from include/t2v_hip.h, and the autograd-graph walk."""
import torch

from tests.emu_ops import EmuOps


class CondEmuOps(EmuOps):
    """``EmuOps`` + t2v_rowlin_fwd / _bwd_data / _wgrad and t2v_timestep_embedding_f32 (problem dicts as ``native.HipOps`` takes them).
    No ``torch.nn.functional.linear``: the tests patch that to raise."""

    @staticmethod
    def _f(x, silu):
        return x * torch.sigmoid(x) if silu else x

    @torch.no_grad()      # (the live parameters are the operands)
    def rowlin_fwd(self, problems, B):
        self._log("rowlin_fwd")
        assert 1 <= B <= 8
        for q in problems:
            y = q.get("alpha", 1.0) * (self._f(q["x"].float(), q.get("silu")) @ q["w"].float().t())
            if q.get("bias") is not None:
                y = y + q["bias"]
            if q.get("res") is not None:
                y = y + q["res"]
            q["y"].copy_(y)

    def rowlin_ws_floats(self, problems, B):
        return sum((q["y"].shape[1] + 63) // 64 * B * q["w"].shape[1] for q in problems)

    @torch.no_grad()      # (the live parameters are the operands)
    def rowlin_bwd_data(self, problems, B, ws):
        self._log("rowlin_bwd_data")
        assert ws.numel() >= self.rowlin_ws_floats(problems, B)
        done = []
        for q in problems:
            if any(q["dx"].data_ptr() == d.data_ptr() for d in done):
                continue
            done.append(q["dx"])
            tot = sum(p.get("alpha", 1.0) * (p["y"].float() @ p["w"].float()) for p in problems if p["dx"].data_ptr() == q["dx"].data_ptr())
            if q.get("silu"):
                sg = torch.sigmoid(q["x"].float())
                tot = tot * (sg * (1 + q["x"].float() * (1 - sg)))
            q["dx"].copy_(q["dx"] + tot if q.get("accumulate") else tot)

    @torch.no_grad()      # (the live parameters are the operands)
    def rowlin_wgrad(self, problems, B):
        self._log("rowlin_wgrad")
        for q in problems:
            dw = q.get("alpha", 1.0) * (q["y"].float().t() @ self._f(q["x"].float(), q.get("silu")))
            q["dw"].copy_(q["dw"] + dw if q.get("accumulate") else dw)
            if q.get("db") is not None:
                db = q["y"].float().sum(0)
                q["db"].copy_(q["db"] + db if q.get("accumulate") else db)

    def timestep_embedding_f32(self, t, dim, guidance_style, out):
        assert out.dtype == torch.float32
        self.timestep_embedding(t, dim, guidance_style, out)


def graph_nodes(t):
    """Names of every node of the autograd graph behind ``t`` (walks ``grad_fn.next_functions``)."""
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names


def assert_engine_node_only(t, engine_node):
    """The graph behind the output is the engine's Function and AccumulateGrad nodes only."""
    names = graph_nodes(t)
    other = sorted({n for n in names if n not in (engine_node, "AccumulateGrad")})
    assert names.count(engine_node) == 1 and not other, f"autograd nodes besides {engine_node} and AccumulateGrad: {other}"


# ---------------------------------------------------------------------------------------------------------------- LoRA route bodies
def lora_step_owned(eng, params, x, ts, ctx, tc, r_out, seed=None, dev="cpu"):
    """One engine-level step with the conditioning branch on the engine: no emb_all in, every LoRA gradient out of the flat arena."""
    y = eng.forward_tape(x.to(dev), ts.to(dev), ctx.to(dev), 16, tc.to(dev), None, seed=seed)
    flat = torch.zeros(eng.lora_numel, device=dev)
    dx = eng.backward(r_out.to(dev), flat_grad=flat, accumulate=False)
    grads, off = [], 0
    for p in params:
        grads.append(flat[off:off + p.numel()].view_as(p).float().cpu().clone())
        off += p.numel()
    return y.float().cpu(), dx.float().cpu(), grads


def cond_slots_before_their_segments(eng, names):
    """The recorded backward sends no piece of the arena that holds a conditioning leaf's gradient slots before the last B-row weight
    gradient was launched.  ``names``: the entry names of the recorded backward list, segment markers as "allreduce_segment"."""
    cond_end = max(int(eng.g_idx[eng.lora_off[id(w)] + w.numel() - 1]) + 1 for mod in eng.cond_lora_leaves() for w in (mod.lora_up.weight, mod.lora_down.weight))
    bounds = eng._seg_bounds()
    last_w = max(i for i, n in enumerate(names) if "rowlin_wgrad" in n)
    marks = [i for i, n in enumerate(names) if n == "allreduce_segment"]
    assert len(marks) == len(bounds) - 1
    # (markers are emitted from the top of the arena down: the k-th marker carries segment len - 1 - k)
    for k, i in enumerate(marks):
        lo = bounds[len(marks) - 1 - k]
        assert lo >= cond_end or i > last_w, (k, lo, cond_end, i, last_w)
    assert marks[-1] > last_w and cond_end > 0


def run_lora_train_masks(dev, ops, out_tol, dx_tol, cos_min, ratio_tol):
    """tests/test_gpu_train_parity.run_train_mode_with_replayed_masks with the conditioning branch ON THE ENGINE: its LoRA dropouts stay
    live (sites of kind "rows"), their masks are replayed into the torch module with every other site's."""
    import copy
    from t2v_turbo_amd import lora
    from t2v_turbo_amd.engine_unet_bwd import UNetGradEngine
    from tests.mask_replay import SiteGeometrySpy, patch_engine_masks
    from tests.test_gpu_train_parity import _cos, _report, _tiny_student
    from tests.test_unet_lora_grad_cpu import _autograd
    from tests.util import load, rel_l2

    def draw(params):
        gen = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for p in params:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)

    g = load("unet_tiny")
    ref, rparams = _tiny_student(64, draw)
    m = copy.deepcopy(ref).to(dev)
    params = lora.lora_parameters(m)
    m.train(); ref.train()
    spy = SiteGeometrySpy(ops)
    eng = UNetGradEngine(m, ops)
    eng.native_conditioning = True
    eng.bind_lora(params)
    x, ts, ctx, tc = g["x"], g["ts"], g["ctx"], g["tc"]
    r_out = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
    seed = 0x5EED_1234_ABCD
    y, dx, grads = lora_step_owned(eng, params, x, ts, ctx, tc, r_out, seed=seed, dev=dev)       # recording pass
    y2, dx2, grads2 = lora_step_owned(eng, params, x, ts, ctx, tc, r_out, seed=seed, dev=dev)    # replayed lists, same seed
    assert torch.equal(y, y2) and rel_l2(dx2, dx) < 1e-6 and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    sites = eng.drop_sites
    n_cond = len(eng.cond_lora_leaves())
    kinds = [k for _, k, _ in sites[:n_cond]]     # the MLP leaves see B rows; emb_layers one mask per clip for all its frames ("ctx", L = 1)
    assert n_cond == 27 and set(kinds) == {"rows", "ctx"} and kinds.count("rows") == 5 and set(spy.sites) == set(range(len(sites)))
    masks = spy.masks(seed)
    patch_engine_masks(ref, eng, masks)
    y_ref, dx_ref, g_ref = _autograd(ref, rparams, x, ts, ctx, 16, tc, None, r_out)
    e_out, e_dx = rel_l2(y, y_ref), rel_l2(dx, dx_ref)
    print(f"[train mode, native conditioning] out {e_out:.3e} dx {e_dx:.3e}", flush=True)
    names = {id(p): n for n, p in m.named_parameters()}
    rows = []
    for p, gq, r in zip(params, grads, g_ref):
        rn = float(r.double().norm())
        if rn == 0.0:
            assert float(gq.abs().max()) < 1e-6
            continue
        rows.append((names[id(p)], _cos(gq, r), float(gq.double().norm()) / rn, rn))
    _report("train mode, tiny, native conditioning", rows, cos_min, ratio_tol)
    assert e_out < out_tol and e_dx < dx_tol
    return eng
