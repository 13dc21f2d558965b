"""Cases of t2v_attn_spatial_rm (spatial self-attention with V read from its token rows), shared by the device test
(tests/test_gpu_attn_rowmajor.py) and the host-simulator test (tests/test_hostsim_attn_rowmajor.py).

Oracle: the V^T form of the same kernel.  The row-major form keeps the key order of the K rows, the order the score registers come
out and the contraction enumeration of the PV product, so the same products are summed in the same MFMA k-order: for equal operands
the two entry points must agree bit for bit.  On top of that the fp32 softmax definition at the project's tolerance for this kernel
(``ATTN_TOL`` of tests/operand_form_cases.py, worst row).

Operands as the engine passes them: q | k | v are the three column ranges of ONE [M, 3 inner + 8] buffer; its eight padding columns
and the rows behind M are NaN, so a key tile that reads past the image (the zero-page rows of K and V) or past the head columns
shows up as a non-finite output."""
import torch

from tests.operand_form_cases import ATTN_TOL, BF, NAN, Out, exact, rnd, row_err

#        n_img seq heads spike
CASES = [(2, 40, 1, False),     # one partial tile: zero-page rows for both K and V
         (2, 160, 2, False),    # two full tiles + a 32-key tail; two heads: the per-head column offsets into the q | k | v buffer
         (1, 256, 1, True)]     # four full tiles; one late key spiked: the running-max rescale across tiles
CASE_IDS = ["-".join(map(str, c[:3])) for c in CASES]
POST_ROWS = 3


def run(ops, dev, n_img, seq, heads, spike):
    inner, M, scale = heads * 64, n_img * seq, 0.125
    q, k, v = rnd(M, inner, seed=1, scale=0.8), rnd(M, inner, seed=2, scale=0.8), rnd(M, inner, seed=3)
    if spike:   # (tests/test_gpu_kernels.py::test_attn_spatial_online_softmax_rescale) a large dot with many queries, in the 4th tile
        k[200] = 6.0 * torch.sign(q[0])
    ld = 3 * inner + 8
    buf = torch.full((M + POST_ROWS, ld), NAN, dtype=torch.float64)
    buf[:M, :inner], buf[:M, inner:2 * inner], buf[:M, 2 * inner:3 * inner] = q, k, v
    qkv = buf.to(BF).to(dev)
    q_d, k_d, v_d = qkv[:M, :inner], qkv[:M, inner:2 * inner], qkv[:M, 2 * inner:3 * inner]
    # the reference operand: V^T per image, [n_img * inner, kp], zero in the padding keys
    kp = (seq + 63) // 64 * 64
    vt = torch.zeros(n_img * inner, kp, dtype=BF)
    for img in range(n_img):
        vt[img * inner:(img + 1) * inner, :seq] = v[img * seq:(img + 1) * seq].t().to(BF)
    o_vt, o_rm = Out(M, inner + 4, [(0, inner)], dev), Out(M, inner + 4, [(0, inner)], dev)
    ops.attn_spatial(q_d, k_d, vt.to(dev), kp, o_vt.views[0], n_img, seq, seq, heads, 1, scale)
    ops.attn_spatial_rm(q_d, k_d, v_d, o_rm.views[0], n_img, seq, heads, scale)
    got_vt, got_rm = o_vt.check("V^T form")[0], o_rm.check("row-major form")[0]
    exact("row-major form vs V^T form", got_rm, got_vt)
    ref = torch.zeros(M, inner, dtype=torch.float32)
    qf, kf, vf = q.float(), k.float(), v.float()
    for img in range(n_img):
        r = slice(img * seq, (img + 1) * seq)
        for hd in range(heads):
            c = slice(hd * 64, hd * 64 + 64)
            ref[r, c] = (qf[r, c] @ kf[r, c].t() * scale).softmax(dim=1) @ vf[r, c]
    err = row_err(got_rm, ref)
    print(f"attn_spatial_rm {n_img}x{seq}x{heads}: worst row vs fp32 softmax {err:.3e} (tolerance {ATTN_TOL:.1e})")
    assert err < ATTN_TOL, err
