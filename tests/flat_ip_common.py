"""Shared by the inner-product flat k-NN tests (test_flat_ip.py, test_flat_ip_bound.py): the exact
reference and a float64 restatement of the shortlist bound for inner products (flat_ip_slack in
alayalite_amd/csrc/flat_bound.h).  The scan modes, the device entry and the near-tie inputs are
flat_common's."""

import numpy as np

from flat_common import FLT_MAX, _f16_exp, contraction_of

U = 2.0 ** -24


def exact_ip(orc, base, q, k, valid=None):
    """The reference: orc_ip_f32 (the ip_sqr_avx2 order, -(q.b), bit-identical to the device's
    exact rescoring) on every valid row, then (distance, id) order.  Slots past the valid rows hold
    (0xffffffff, FLT_MAX), as the device's."""
    lib = orc.lib()
    base = np.ascontiguousarray(base, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    live = np.arange(len(base)) if valid is None else np.nonzero(valid)[0]
    out_i = np.full((len(q), k), 0xFFFFFFFF, np.uint32)
    out_d = np.full((len(q), k), FLT_MAX, np.float32)
    d = base.shape[1]
    ptrs = [base[i].ctypes.data for i in live]
    f = lib.orc_ip_f32
    for a in range(len(q)):
        qp = q[a].ctypes.data
        dist = np.array([f(qp, p, d) for p in ptrs], np.float32)
        o = np.lexsort((live, dist))[:k]
        out_i[a, :len(o)], out_d[a, :len(o)] = live[o], dist[o]
    return out_i, out_d


def ip_slack64(mode, base, q):
    """flat_ip_slack restated in float64 for every query: the merge proves a query when its k-th
    reference distance is below (approximate cutoff) / 2 - slack.  The constants are flat_bound.h's;
    max|b| is capi.cpp's ensure_norms value; the query scale 2^t is per query in the
    warp-specialised scan and per wave of 32 queries in the single-role scan."""
    d = base.shape[1]
    stride = (d + 31) // 32 * 32
    contraction = contraction_of(mode, d)
    k_acc = float(stride)  # the slab widths 64/96/128 divide 960, the only wide row here
    assert stride <= 224 or stride == 960
    b64 = base.astype(np.float64)
    q64 = q.astype(np.float64)
    bmax = np.sqrt((b64 * b64).sum(1).max()) * 1.0001
    qnorm = np.sqrt((q64 * q64).sum(1))
    qb = qnorm * bmax
    acc = 2.0 * k_acc * (3.1 if contraction == 1 else 1.01)
    ref = float(int(stride) // 32 + 16)
    s = (acc + ref) * U * qb
    if contraction == 2:
        se = _f16_exp(bmax)
        qmax = np.abs(q).max(1)
        if "-ws" in mode:
            t = np.array([_f16_exp(m) for m in qmax])
        else:
            t = np.array([_f16_exp(qmax[a // 32 * 32:a // 32 * 32 + 32].max()) for a in range(len(q))])
        ec = ((9.7680283e-4 + 2.4e-7) * qb + 1.0005 * np.sqrt(k_acc) * (qnorm * 2.0 ** (-14 - se) + bmax * 2.0 ** (-14.0 - t))
              + k_acc * 2.0 ** (-28.0 - se - t))
        s = s + 1.0001 * ec
    elif contraction == 1:
        s = s + 3.05 * 2.0 ** -16 * qb
    return (s + 1e-30) * (1.0 + 2.0 * k_acc * U)


def ip_gap64(base, q, k):
    """Exact float64 gap between the k-th inner-product distance -(q.b) and the last one a merged
    shortlist can hold: the 32nd, or the 128th of the big merge's list (k > 24)."""
    last = 32 if k <= 24 else 128
    dd = -(q.astype(np.float64) @ base.astype(np.float64).T)
    dd = np.partition(dd, (k - 1, last - 1), axis=1)
    return dd[:, last - 1] - dd[:, k - 1]
