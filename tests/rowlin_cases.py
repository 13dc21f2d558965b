"""Kernel cases of the B-row linear family (t2v_rowlin_fwd / t2v_rowlin_bwd_data / t2v_rowlin_wgrad, csrc/full_grad.hip) — one table, two
backends: ``tests/test_hostsim_rowlin.py`` runs it on the host SIMT simulator, ``tests/test_gpu_rowlin.py`` on the device.

Operand forms and guards are those of ``tests/operand_form_cases.py``: every operand is a view into a larger buffer whose unread bytes
(stride gaps, spare rows before and after — among them row B, the first one past the batch) hold NaN; every output allocation is a
sentinel outside the region the header says is written and is compared bit for bit there; the workspace has a guarded tail.

Reference: fp64, written out here from the text of include/t2v_hip.h.  The kernels are fp32 end to end, so the bound is per ELEMENT and
derived, not tuned:  |got - ref| <= 4 L 2^-24 sum|terms|,  L the contraction length (K for fwd, the N of all problems that share the dx
for bwd_data, B for wgrad) and sum|terms| the fp64 sum of the absolute values of everything that is added into the element (products,
bias, residual, the old value under ``accumulate``; for bwd_data times |g|).  With bf16 weights the reference uses the bf16 values.
Every case runs twice on fresh outputs and must give the same bits."""
import ctypes as C

import torch

from tests.operand_form_cases import Out, inbuf

F32, BF = torch.float32, torch.bfloat16
U = 2.0 ** -24
REPORT = []   # (case, tensor, worst |got - ref| / bound)


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(F32)


def _silu(v):
    return v / (1.0 + torch.exp(-v))


def _dsilu(v):
    sg = 1.0 / (1.0 + torch.exp(-v))
    return sg * (1.0 + v * (1.0 - sg))


def _weights(N, K, bf16, seed):
    w = _rand(N, K, seed=seed, scale=K ** -0.5)
    return w.to(BF) if bf16 else w


def _bits(t):
    return t.contiguous().view(torch.int32)


def _within(name, what, got, ref, terms, L):
    bound = 4.0 * L * U * terms
    err = (got.double() - ref).abs()
    ok = err <= bound
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    REPORT.append((name, what, worst))
    assert bool(ok.all()), (f"{name} {what}: |got - ref| = {float(err[~ok].max()):.3e} above 4 L 2^-24 sum|terms| at "
                            f"{(~ok).nonzero()[0].tolist()} (worst ratio {worst:.2f}, L = {L})")


# ---------------------------------------------------------------------------------------------------------------- the tables
# fwd / wgrad problem: (K, N, flags); flags: b = bias / db, r = residual, s = SiLU, h = bf16 weights, a = accumulate, o = odd strides
# (element loads and stores: ldw, ldo not a multiple of 16 bytes)
def _table25():
    return [(16 + 4 * (i % 3), (64, 128, 256)[i % 3], "bs"[i % 2] + ("h" if i % 5 == 0 else "") + ("r" if i % 4 == 0 else "") + ("a" if i % 3 == 0 else ""))
            for i in range(25)]


LIN_CASES = {
    "b1_k4_n1": (1, [(4, 1, "b")]),
    "b3_k68_n72_silu_res": (3, [(68, 72, "bsr")]),
    "b8_k256_n64_bf16": (8, [(256, 64, "h")]),
    "b8_k1280_n320_silu": (8, [(1280, 320, "bsa")]),
    "b3_k68_n72_bf16_odd": (3, [(68, 72, "hro")]),
    "b1_k6_n5_tail_odd": (1, [(6, 5, "bao")]),
    "b8_k68_n1_acc": (8, [(68, 1, "bra")]),
    "b3_table25": (3, _table25()),
    "b2_real_3x1280": (2, [(1280, 1280, "bs"), (1280, 1280, "b"), (1280, 1280, "sa")]),
}

# bwd_data: (B, [group]); group = (K, flags, [(N, problem flags)]): its problems share one dx.  flags: s = g is silu'(pre), a = accumulate;
# problem flags: h = bf16, o = odd ldw
BWD_CASES = {
    "b1_k4_n1": (1, [(4, "", [(1, "")])]),
    "b3_k68_shared_n72_130_1_silu": (3, [(68, "s", [(72, ""), (130, "h"), (1, "o")])]),
    "b8_k256_n64_bf16_acc": (8, [(256, "a", [(64, "h")])]),
    "b8_k1280_n320_silu_acc": (8, [(1280, "sa", [(320, "")])]),
    "b3_k6_n72_tail_odd": (3, [(6, "", [(72, "o")])]),
    "b3_table25": (3, [(16, "s", [((64, 128, 256)[i % 3], "h" if i % 5 == 0 else "") for i in range(13)]),
                       (24, "a", [((64, 128, 256)[i % 3], "") for i in range(12)])]),
    "b2_real_3x1280": (2, [(1280, "s", [(1280, ""), (1280, ""), (1280, "")])]),
}


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- forward
def _fwd_once(ops, dev, B, probs, seed):
    table, outs, refs = [], [], []
    for i, (K, N, fl) in enumerate(probs):
        s = seed + 10 * i
        x, w = _rand(B, K, seed=s), _weights(N, K, "h" in fl, s + 1)
        bias = _rand(N, seed=s + 2) if "b" in fl else None
        res = _rand(B, N, seed=s + 3) if "r" in fl else None
        vec = 8 if "h" in fl else 4
        ldw = K + 3 if "o" in fl else K + vec
        y = Out(B, N + 5, [(2, 2 + N)], dev, dtype=F32)
        alpha = 0.625 if i % 2 else 1.0
        q = dict(x=inbuf(x, K + 4, dev, F32), w=inbuf(w, ldw, dev, w.dtype), y=y.views[0], silu="s" in fl, alpha=alpha)
        if bias is not None:
            q["bias"] = inbuf(bias.view(1, N), N, dev, F32).view(N)
        if res is not None:
            q["res"] = inbuf(res, N + 3, dev, F32, col0=1)
        table.append(q)
        outs.append(y)
        fx = _silu(x.double()) if "s" in fl else x.double()
        prod = fx[:, None, :] * w.double()[None, :, :]
        ref, terms = alpha * prod.sum(-1), alpha * prod.abs().sum(-1)
        if bias is not None:
            ref, terms = ref + bias.double(), terms + bias.double().abs()
        if res is not None:
            ref, terms = ref + res.double(), terms + res.double().abs()
        refs.append((ref, terms, K))
    ops.rowlin_fwd(table, B)
    _sync(dev)
    return outs, refs


def run_fwd(ops, dev, name):
    B, probs = LIN_CASES[name]
    probs = [(K, N, fl.replace("a", "")) for K, N, fl in probs]
    outs, refs = _fwd_once(ops, dev, B, probs, 100)
    got = [o.check(f"{name} y[{i}]")[0] for i, o in enumerate(outs)]
    for i, (g, (ref, terms, L)) in enumerate(zip(got, refs)):
        _within(name, f"y[{i}]", g, ref, terms, L)
    again = [o.check(name)[0] for o in _fwd_once(ops, dev, B, probs, 100)[0]]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again)), f"{name}: two calls with the same arguments differ"


# ---------------------------------------------------------------------------------------------------------------- weight gradient
def _wgrad_once(ops, dev, B, probs, seed):
    table, outs, refs = [], [], []
    for i, (K, N, fl) in enumerate(probs):
        s = seed + 10 * i
        x, dy = _rand(B, K, seed=s), _rand(B, N, seed=s + 1)
        acc, alpha = "a" in fl, (0.625 if i % 2 else 1.0)
        old_w = _rand(N, K, seed=s + 2) if acc else None
        old_b = _rand(N, seed=s + 3) if acc else None
        ldo = K + 3 if "o" in fl else K + 4
        dw = Out(N, ldo, [(0, K)], dev, dtype=F32, init=[old_w])
        q = dict(x=inbuf(x, K + 4, dev, F32), y=inbuf(dy, N + 3, dev, F32, col0=1), dw=dw.views[0], silu="s" in fl, accumulate=acc, alpha=alpha)
        db = None
        if "b" in fl:
            db = Out(1, N, [(0, N)], dev, dtype=F32, init=[None if old_b is None else old_b.view(1, N)])
            q["db"] = db.views[0].view(N)
        table.append(q)
        outs.append((dw, db))
        fx = _silu(x.double()) if "s" in fl else x.double()
        prod = dy.double().t()[:, None, :] * fx.t()[None, :, :]          # [N, K, B]
        rw, tw = alpha * prod.sum(-1), alpha * prod.abs().sum(-1)
        rb, tb = dy.double().sum(0), dy.double().abs().sum(0)
        if acc:
            rw, tw, rb, tb = rw + old_w.double(), tw + old_w.double().abs(), rb + old_b.double(), tb + old_b.double().abs()
        refs.append((rw, tw, rb, tb))
    ops.rowlin_wgrad(table, B)
    _sync(dev)
    return outs, refs


def run_wgrad(ops, dev, name):
    B, probs = LIN_CASES[name]
    probs = [(K, N, fl.replace("r", "")) for K, N, fl in probs]

    def collect(outs):
        return [(dw.check(f"{name} dw[{i}]")[0], None if db is None else db.check(f"{name} db[{i}]")[0]) for i, (dw, db) in enumerate(outs)]

    outs, refs = _wgrad_once(ops, dev, B, probs, 200)
    got = collect(outs)
    for i, ((gw, gb), (rw, tw, rb, tb)) in enumerate(zip(got, refs)):
        _within(name, f"dw[{i}]", gw, rw, tw, B)
        if gb is not None:
            _within(name, f"db[{i}]", gb.view(-1), rb, tb, B)
    again = collect(_wgrad_once(ops, dev, B, probs, 200)[0])
    for (a, b), (c, d) in zip(got, again):
        assert torch.equal(_bits(a), _bits(c)) and (b is None or torch.equal(_bits(b), _bits(d))), f"{name}: two calls with the same arguments differ"


# ---------------------------------------------------------------------------------------------------------------- data gradient
def _bwd_once(ops, dev, B, groups, seed):
    table, outs, refs = [], [], []
    for gi, (K, gfl, members) in enumerate(groups):
        s = seed + 100 * gi
        acc, silu = "a" in gfl, "s" in gfl
        pre = _rand(B, K, seed=s)
        old = _rand(B, K, seed=s + 1) if acc else None
        dx = Out(B, K + 6, [(3, 3 + K)], dev, dtype=F32, init=[old])
        pre_v = inbuf(pre, K + 4, dev, F32) if silu else None
        tot, terms, L = torch.zeros(B, K, dtype=torch.float64), torch.zeros(B, K, dtype=torch.float64), 0
        for j, (N, fl) in enumerate(members):
            w, dy = _weights(N, K, "h" in fl, s + 10 * j + 2), _rand(B, N, seed=s + 10 * j + 3)
            vec = 8 if "h" in fl else 4
            q = dict(w=inbuf(w, K + 3 if "o" in fl else K + vec, dev, w.dtype), y=inbuf(dy, N + 3, dev, F32, col0=2), dx=dx.views[0], silu=silu,
                     accumulate=acc, alpha=0.75 if j % 2 else 1.0)
            if silu:
                q["x"] = pre_v
            table.append(q)
            prod = (0.75 if j % 2 else 1.0) * dy.double()[:, :, None] * w.double()[None, :, :]       # [B, N, K]
            tot, terms, L = tot + prod.sum(1), terms + prod.abs().sum(1), L + N
        g = _dsilu(pre.double()) if silu else torch.ones(B, K, dtype=torch.float64)
        ref, terms = g * tot, g.abs() * terms
        if acc:
            ref, terms = ref + old.double(), terms + old.double().abs()
        outs.append(dx)
        refs.append((ref, terms, L))
    # (interleave the groups' problems: the sum over a dx must not depend on its problems being neighbours in the table)
    order = sorted(range(len(table)), key=lambda i: (i % 3, i)) if len(groups) > 1 else list(range(len(table)))
    if len(order) > 24:   # a table longer than one launch: the spilled problem belongs to the SiLU group that does NOT accumulate, so the
        order.append(order.pop(order.index(0)))   # second launch pair must add to the first one's dx by itself, with g(pre) on both halves
        assert not table[order[-1]]["accumulate"] and table[order[-1]]["silu"]
    table = [table[i] for i in order]
    need = ops.rowlin_ws_floats(table, B)
    assert need > 0
    ws = Out(1, need + 64, [(0, need)], dev, dtype=F32)
    ops.rowlin_bwd_data(table, B, ws.views[0].view(-1))
    _sync(dev)
    ws.guard("workspace tail")
    return outs, refs


def run_bwd(ops, dev, name):
    B, groups = BWD_CASES[name]
    outs, refs = _bwd_once(ops, dev, B, groups, 300)
    got = [o.check(f"{name} dx[{i}]")[0] for i, o in enumerate(outs)]
    for i, (g, (ref, terms, L)) in enumerate(zip(got, refs)):
        _within(name, f"dx[{i}]", g, ref, terms, L)
    again = [o.check(name)[0] for o in _bwd_once(ops, dev, B, groups, 300)[0]]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again)), f"{name}: two calls with the same arguments differ"


# ---------------------------------------------------------------------------------------------------------------- refusals
EINVAL, ESHAPE = -1, -2
REFUSALS = ["fwd_short_ldw", "fwd_short_ldx", "fwd_short_ldy", "fwd_short_ldr", "fwd_lds_limit", "fwd_b9", "fwd_null_x", "fwd_null_table",
            "bwd_short_ldo", "bwd_short_ldx", "bwd_null_ws", "bwd_b9", "bwd_null_dx", "wgrad_short_ldo", "wgrad_short_ldx", "wgrad_null_dw", "wgrad_b0"]


def run_refusal(ops, dev, name):
    """Nothing is launched for a refused table: every output allocation comes back bit for bit, and the SECOND problem is the bad one."""
    B, K, N = 3, 8, 6
    x, w, dy = _rand(B, K, seed=1), _rand(N, K, seed=2), _rand(B, N, seed=3)
    y, dx, dw, ws = (Out(B, N + 2, [(0, N)], dev, dtype=F32), Out(B, K + 2, [(0, K)], dev, dtype=F32), Out(N, K + 2, [(0, K)], dev, dtype=F32),
                     Out(1, 4096, [(0, 4096)], dev, dtype=F32))
    entry = name.split("_")[0]
    if entry == "fwd":
        q = dict(x=inbuf(x, K + 4, dev, F32), w=inbuf(w, K + 4, dev, F32), y=y.views[0], res=inbuf(dy, N + 2, dev, F32))
    elif entry == "bwd":
        q = dict(w=inbuf(w, K + 4, dev, F32), y=inbuf(dy, N + 2, dev, F32), dx=dx.views[0], x=inbuf(x, K + 4, dev, F32), silu=True)
    else:
        q = dict(x=inbuf(x, K + 4, dev, F32), y=inbuf(dy, N + 2, dev, F32), dw=dw.views[0])
    arr = ops.rowlin_table([q, q], B)
    bad, n, rows, wsp, want = arr[1], 2, B, ws.full.data_ptr(), ESHAPE
    what = name[len(entry) + 1:]
    if what.startswith("short_"):
        setattr(bad, what[6:], (N if what[6:] in ("ldy", "ldr") else K) - 1)
    elif what == "lds_limit":      # B * K = 3 * 6000 > 16384 input floats (every stride long enough: only the LDS limit refuses it)
        bad.K = bad.ldx = bad.ldw = 6000
    elif what in ("b9", "b0"):
        rows, want = (9 if what == "b9" else 0), EINVAL
    elif what == "null_table":
        arr, want = None, EINVAL
    elif what == "null_ws":
        wsp, want = None, EINVAL
    else:
        setattr(bad, what[5:], None)
        want = EINVAL
    table = None if arr is None else C.cast(arr, C.c_void_p)
    if entry == "fwd":
        rc = ops.lib.t2v_rowlin_fwd(table, n, rows, ops.stream())
    elif entry == "bwd":
        rc = ops.lib.t2v_rowlin_bwd_data(table, n, rows, wsp, 4096, ops.stream())
    else:
        rc = ops.lib.t2v_rowlin_wgrad(table, n, rows, ops.stream())
    _sync(dev)
    assert rc == want, (name, rc, want)
    assert y.untouched() and dx.untouched() and dw.untouched() and ws.untouched(), f"{name}: a refused call wrote something"


def run_timestep_embedding_f32(ops, dev):
    """cos || sin of t * exp(-ln(1e4) i / half), fp32 (utils_diffusion.py:8-32); the guidance form sin || cos of 1000 t with (half - 1)."""
    import math
    for t, guidance, dim in ((torch.tensor([999, 0, 17], dtype=torch.int64), False, 32), (torch.tensor([7.5, 0.25]), True, 16)):
        out = Out(t.numel(), dim, [(0, dim)], dev, dtype=F32)
        ops.timestep_embedding_f32(t.to(dev), dim, guidance, out.views[0])
        _sync(dev)
        got = out.check("timestep_embedding_f32")[0].double()
        half = dim // 2
        i = torch.arange(half, dtype=torch.float64)
        if guidance:
            a = t.double()[:, None] * 1000.0 * torch.exp(-i * math.log(10000.0) / (half - 1))[None]
            ref = torch.cat([a.sin(), a.cos()], 1)
        else:
            a = t.double()[:, None] * torch.exp(-math.log(10000.0) * i / half)[None]
            ref = torch.cat([a.cos(), a.sin()], 1)
        # the angle is formed in fp32 (|a| up to 7 500: one rounding of it moves sin / cos by |a| 2^-24), as in the bf16 entry and the reference
        assert float((got - ref).abs().max()) <= 8 * float(a.abs().max() + 1) * U, float((got - ref).abs().max())


def run_dropout_f32(ops, dev):
    """t2v_dropout_f32: the mask of t2v_dropout_bf16 bit for bit (tests.emu_ops.EmuOps.dropout_keep is the device mask) on fp32 rows, with and
    without the residual, on strided views; kept values x / (1 - p') (+ resid) within one rounding of the fused multiply-add."""
    from t2v_turbo_amd import native as nt
    from tests.emu_ops import EmuOps
    B, N, p, site, seed = 3, 70, 0.1, 5, 0x1234_5678_9ABC
    x, res = _rand(B, N, seed=1), _rand(B, N, seed=2)
    seed_t = torch.tensor([seed], dtype=torch.int64).to(dev)
    keep = EmuOps.dropout_keep(seed, site, B, N, p)
    assert 0 < int(keep.sum()) < B * N
    for with_res in (False, True):
        out = Out(B, N + 4, [(1, 1 + N)], dev, dtype=F32)
        ops.dropout(inbuf(x, N + 2, dev, F32), inbuf(res, N + 6, dev, F32, col0=3) if with_res else None, out.views[0], N, p, seed_t, site)
        _sync(dev)
        got = out.check("dropout_f32")[0].double()
        kept = torch.where(keep, x.double() * nt.dropout_inv_keep(p), torch.zeros((), dtype=torch.float64))
        ref = kept + (res.double() if with_res else 0.0)
        assert bool(((got != (res.double() if with_res else 0.0)) == (keep & (x != 0))).all()), "mask differs from the bf16 entry's"
        assert bool(((got - ref).abs() <= 2 * U * (kept.abs() + (res.double().abs() if with_res else 0.0))).all())
