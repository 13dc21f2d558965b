"""The one descriptor-table path of ``optim.py``: the record dtypes against the ctypes classes of ``native.py``, the three table
builders against the constructions they replaced (restated here as they were, hand-typed dtypes and Python loops included), the
recently-used plan cache and ``touch``."""
import ctypes
import random

import numpy as np
import pytest
import torch

from t2v_turbo_amd import native as nt
from t2v_turbo_amd import optim
from t2v_turbo_amd.packs import params_fingerprint

SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 10561]   # around the 256-element and the 4096-element block edges, several blocks


def _shuffled(seed, n=len(SIZES)):
    sizes = [SIZES[i % len(SIZES)] for i in range(n)]
    random.Random(seed).shuffle(sizes)
    assert sizes != sorted(sizes)
    return sizes


# ---- the record layouts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("struct, size", [(nt.EmaTensor, 40), (nt.Adamw8Tensor, 56), (nt.AdamwTensor, 56)])
def test_record_dtype_is_the_ctypes_layout(struct, size):
    dt = optim.record_dtype(struct)
    assert dt.itemsize == ctypes.sizeof(struct) == size
    assert list(dt.names) == [f[0] for f in struct._fields_]
    for name, ctype in struct._fields_:
        assert dt.fields[name][1] == getattr(struct, name).offset, name
        assert dt.fields[name][0].itemsize == ctypes.sizeof(ctype), name
        assert dt.fields[name][0].kind == {ctypes.c_void_p: "u", ctypes.c_longlong: "i", ctypes.c_int: "i", ctypes.c_float: "f"}[ctype], name


# ---- the constructions the builders replaced, as they were ----------------------------------------------------------------------------
_OLD_EMA = np.dtype([("target", "<u8"), ("src", "<u8"), ("n", "<i8"), ("work0", "<i8"), ("src_dt", "<i4"), ("reserved", "<i4")])
_OLD_ADAMW8 = np.dtype([("param", "<u8"), ("grad", "<u8"), ("state_block", "<i8"), ("n", "<i8"), ("work0", "<i8"), ("lr", "<f4"),
                        ("weight_decay", "<f4"), ("flags", "<i4"), ("reserved", "<i4")])
_OLD_ADAMW = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("n", "<i8"), ("work0", "<i8"),
                       ("hyper", "<i4"), ("reserved", "<i4")])


def _old_ema_table(targets, sources):
    host = np.zeros(len(targets), dtype=_OLD_EMA)
    work = 0
    for i, (t, s) in enumerate(zip(targets, sources)):
        host[i] = (t.data_ptr(), s.data_ptr(), t.numel(), work, nt.BF16 if s.dtype == torch.bfloat16 else nt.F32, 0)
        work += (t.numel() + nt.EMA_BLOCK - 1) // nt.EMA_BLOCK
    return host, work


def _old_adamw8_table(opt, active):
    """The loop ``AdamW8bit._step_hip`` had: (host with lr / weight_decay still zero, launches)."""
    groups = opt.param_groups
    step0 = opt.state[active[0][1]]["step"]
    keys = [(groups[gi]["betas"][0], groups[gi]["betas"][1], groups[gi]["eps"], opt.state[p]["step"] - step0) for gi, p in active]
    order = sorted(range(len(active)), key=lambda i: keys[i])
    host = np.zeros(len(active), dtype=_OLD_ADAMW8)
    launches, work, start = [], 0, 0
    for j, i in enumerate(order):
        gi, p = active[i]
        if j > 0 and keys[i] != keys[order[j - 1]]:
            launches.append((start, j, work, keys[order[j - 1]]))
            start, work = j, 0
        is8, b0, nb = opt._layout[p]
        host[j] = (p.data_ptr(), p.grad.data_ptr(), b0, p.numel(), work, 0.0, 0.0, 0 if is8 else 1, 0)
        work += nb
    launches.append((start, len(order), work, keys[order[-1]]))
    group = np.array([active[i][0] for i in order])
    host["lr"] = np.array([g["lr"] for g in groups], dtype=np.float32)[group]
    host["weight_decay"] = np.array([g["weight_decay"] for g in groups], dtype=np.float32)[group]
    return host, launches


def _old_adamw_table(grads, params=None, exp_avgs=None, exp_avg_sqs=None, rows=None):
    ptrs = lambda ts: np.array([t.data_ptr() for t in ts], dtype=np.uint64)   # noqa: E731
    n = len(grads)
    host = np.zeros(n, dtype=_OLD_ADAMW)
    host["grad"] = ptrs(grads)
    for field, lst in (("param", params), ("exp_avg", exp_avgs), ("exp_avg_sq", exp_avg_sqs)):
        if lst is not None:
            host[field] = ptrs(lst)
    numel = np.array([g.numel() for g in grads], dtype=np.int64)
    blocks = (numel + nt.ADAMW_BLOCK - 1) // nt.ADAMW_BLOCK
    rows = np.zeros(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    host["n"] = numel
    launches, start = [], 0
    while start < n:
        end = int(np.searchsorted(rows, rows[start] + 16, side="left"))
        host["work0"][start:end] = np.cumsum(blocks[start:end]) - blocks[start:end]
        host["hyper"][start:end] = rows[start:end] - rows[start]
        launches.append((start, end, int(blocks[start:end].sum()), int(rows[start]), int(rows[end - 1] - rows[start]) + 1))
        start = end
    return host, launches


def _same_image(new, old):
    assert new.dtype.itemsize == old.dtype.itemsize and new.shape == old.shape
    assert new.tobytes() == old.tobytes()


# ---- the builders --------------------------------------------------------------------------------------------------------------------
def test_work_blocks():
    work0, total = optim.work_blocks([1, 256, 257, 0, 4096], 256)
    assert work0.tolist() == [0, 1, 2, 4, 4] and total == 20 and isinstance(total, int) and work0.dtype == np.int64


def test_ema_table_is_the_image_it_was():
    sizes = _shuffled(1)
    targets = [torch.zeros(n) for n in sizes]
    sources = [torch.zeros(n, dtype=torch.bfloat16 if i % 3 == 1 else torch.float32) for i, n in enumerate(sizes)]
    new, work = optim.ema_table(targets, sources)
    old, old_work = _old_ema_table(targets, sources)
    _same_image(new, old)
    assert work == old_work == sum((n + 4095) // 4096 for n in sizes) and isinstance(work, int)


class _Capture:
    """Stands in for ``HipOps`` under ``AdamW8bit``: keeps every launch's table bytes and scalars, computes nothing."""

    def __init__(self):
        self.calls = []

    def adamw8_step(self, table, n, work, *rest):
        self.calls.append((bytes(table.numpy().tobytes()), n, work, rest[8:]))


def test_adamw8_step_builds_the_image_and_the_launches_it_did():
    """Two groups with their own betas (two launches) and learning rates, tensors on both sides of ``min_8bit_size``, one parameter
    without a gradient; the second step moves one lr and uploads again, the third changes nothing and does not."""
    sizes = _shuffled(2)
    params = [torch.nn.Parameter(torch.zeros(n)) for n in sizes + [300]]
    for p in params[:-1]:
        p.grad = torch.zeros_like(p)
    opt = optim.AdamW8bit([dict(params=params[0::2], betas=(0.8, 0.95), lr=3e-4), dict(params=params[1::2], weight_decay=0.1)], lr=1e-3)
    opt.native_ops = cap = _Capture()
    uploads = []
    for step, lr in enumerate((3e-4, 7e-4, 7e-4)):
        opt.param_groups[0]["lr"] = lr
        opt.step()
        active = [(gi, p) for gi, g in enumerate(opt.param_groups) for p in g["params"] if p.grad is not None]
        old, launches = _old_adamw8_table(opt, active)
        t = opt._table
        _same_image(t["host"], old)
        assert t["launches"] == launches and len(launches) == 2
        assert bytes(t["dev"].numpy().tobytes()) == old.tobytes()
        whole = old.tobytes()
        assert [(c[0], c[1], c[2]) for c in cap.calls[-2:]] == [(whole[s * 56:], e - s, w) for s, e, w, _ in launches]
        assert [c[3][:3] for c in cap.calls[-2:]] == [k[:3] for _, _, _, k in launches]
        uploads.append(t["uploaded"])
    assert uploads[0] != uploads[1] and uploads[1] is uploads[2]
    assert {int(f) for f in opt._table["host"]["flags"]} == {0, 1} and params[-1]._version == 0


def test_adamw8_table_with_given_state_blocks():
    """As tests/adamw_cases.py calls it: one launch, every tensor under fp32 state, the state blocks the caller's."""
    sizes = _shuffled(3)
    p, g = [torch.zeros(n) for n in sizes], [torch.zeros(n) for n in sizes]
    old = np.zeros(len(sizes), dtype=_OLD_ADAMW8)
    b0 = 0
    for j, n in enumerate(sizes):
        old[j] = (p[j].data_ptr(), g[j].data_ptr(), b0, n, b0, 1e-3, 1e-2, nt.ADAMW8_F32_STATE, 0)
        b0 += (n + 255) // 256
    first, total = optim.work_blocks(sizes, optim.QBLOCK)
    new, launches = optim.adamw8_table(p, g, first, True, lr=1e-3, weight_decay=1e-2)
    _same_image(new, old)
    assert launches == [(0, len(sizes), b0)] and total == b0


def test_adamw_table_is_the_image_it_was_and_17_rows_take_two_launches():
    sizes = _shuffled(4, 17)
    cols = [[torch.zeros(n) for n in sizes] for _ in range(4)]
    for rows in (None, [i // 6 for i in range(17)], list(range(17))):
        new, launches = optim.adamw_table(*cols, rows)
        old, old_launches = _old_adamw_table(*cols, rows)
        _same_image(new, old)
        assert launches == old_launches
    assert [(e - s, rows) for s, e, _, _, rows in launches] == [(16, 16), (1, 1)]
    new, launches = optim.adamw_table(cols[0])          # gradients only: the clipping kernels' table
    old, old_launches = _old_adamw_table(cols[0])
    _same_image(new, old)
    assert launches == old_launches and len(launches) == 1


def test_upload_into_the_table_that_is_there():
    host, _ = optim.adamw_table([torch.zeros(5), torch.zeros(4097)])
    table, keep = optim.upload(host, torch.device("cpu"))
    assert keep is None and table.dtype == torch.uint8 and table.numpy().tobytes() == host.tobytes()
    host["work0"][1] = 7
    again, _ = optim.upload(host, torch.device("cpu"), out=table)
    assert again is table and table.numpy().tobytes() == host.tobytes()


# ---- the plan cache and the version counters --------------------------------------------------------------------------------------
def test_recent_keeps_four_plans_most_recently_used_last():
    plans, built = optim._Recent(), []

    def build(k):
        built.append(k)
        return dict(key=k)

    for k in "abcd":
        plans.lookup(k, lambda: build(k))
    assert list(plans) == list("abcd") and built == list("abcd")
    again = plans.lookup("b", lambda: build("b"))
    assert again["key"] == "b" and list(plans) == list("acdb") and built == list("abcd")     # moved to the end, nothing built
    plans.lookup("e", lambda: build("e"))
    assert list(plans) == list("cdbe") and built == list("abcde")                             # the fifth evicts the oldest
    assert plans.lookup("f", lambda: None) is None and list(plans) == list("cdbe")            # a refused build leaves nothing
    assert isinstance(optim._EMA_TABLES, optim._Recent) and isinstance(optim._CLIP_PLANS, optim._Recent)
    assert optim._EMA_TABLES.capacity == optim._CLIP_PLANS.capacity == 4


def test_touch_moves_each_version_by_one_and_the_fingerprint():
    holder = torch.nn.Linear(3, 2)
    before = [p._version for p in holder.parameters()]
    prints = [params_fingerprint(holder)]
    optim.touch(list(holder.parameters()))
    assert [p._version for p in holder.parameters()] == [v + 1 for v in before]
    prints.append(params_fingerprint(holder))
    optim.touch(holder.weight)                       # one tensor, as FlatAdamW, update_ema and AdamW8bit touch
    assert holder.weight._version == before[0] + 2 and holder.bias._version == before[1] + 1
    prints.append(params_fingerprint(holder))
    assert len(set(prints)) == 3
