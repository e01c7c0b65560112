"""Shared by the flat exact k-NN tests (test_flat.py, test_flat_bound.py): the eight scan modes,
the exact reference, the device entry, the near-tie inputs and a float64 restatement of the
shortlist bound (shortlist_eps in alayalite_amd/csrc/flat_kernels.hip)."""

import numpy as np

FLAT_MODES = ["f16", "split", "f32", "f16-prescan2", "f32-prescan3", "f16-ws", "f16-ws1", "split-ws1"]
_FLAT_ENV = ("ALAYA_FLAT_F32", "ALAYA_FLAT_PRESCAN", "ALAYA_FLAT_WS2", "ALAYA_FLAT_CONTRACTION", "ALAYA_FLAT_TILES")
FLT_MAX = np.finfo(np.float32).max


def apply_flat_mode(monkeypatch, mode):
    """Every shortlist contraction: the single-pass f16 on power-of-two-scaled operands (the default
    for rows of <= 224 floats), the bf16 hi/lo split (ALAYA_FLAT_CONTRACTION=bf16x3; the default for
    wider rows) and the f32 MFMA (ALAYA_FLAT_CONTRACTION=f32).  The exact rescoring and the bound
    check make the answer identical.  The single pass runs the single-role scan over the index's
    cached f16 tile records by default; -ws modes force the warp-specialised scan
    (ALAYA_FLAT_TILES=0), which converts the f32 rows itself.  The prescan (a scan over every S-th
    row -- every S-th tile record in the single-role scan -- that seeds each chunk's threshold;
    ALAYA_FLAT_PRESCAN=S) is forced on by the -prescanS modes.  The warp-specialised scan runs two
    consumer waves per producer by default; -ws1 forces one (ALAYA_FLAT_WS2=0)."""
    for var in _FLAT_ENV:
        monkeypatch.delenv(var, raising=False)
    if "-ws" in mode:
        monkeypatch.setenv("ALAYA_FLAT_TILES", "0")
    if mode.endswith("-ws1"):
        monkeypatch.setenv("ALAYA_FLAT_WS2", "0")
    if mode.startswith("f32"):
        monkeypatch.setenv("ALAYA_FLAT_CONTRACTION", "f32")
    if mode.startswith("split"):
        monkeypatch.setenv("ALAYA_FLAT_CONTRACTION", "bf16x3")
    if "prescan" in mode:
        monkeypatch.setenv("ALAYA_FLAT_PRESCAN", mode[-1])
    return mode


def contraction_of(mode, dim):
    """The contraction a flat search in this mode runs first (alaya_index_flat_last_contraction):
    0 f32, 1 bf16 hi/lo split, 2 single-pass f16."""
    if mode.startswith("f32"):
        return 0
    if mode.startswith("split") or (dim + 31) // 32 * 32 > 224:
        return 1
    return 2


def exact(orc, base, q, k):
    """The reference: orc_l2_f32 (the l2_sqr_avx2 order, bit-identical to the device's exact
    rescoring) on every row, then (distance, id) order.  Slots past the base hold
    (0xffffffff, FLT_MAX), as the device's."""
    lib = orc.lib()
    n = len(base)
    out_i = np.full((len(q), k), 0xFFFFFFFF, np.uint32)
    out_d = np.full((len(q), k), FLT_MAX, np.float32)
    rows = [np.ascontiguousarray(base[i]) for i in range(n)]
    ptrs = [orc._ptr(r) for r in rows]
    for a in range(len(q)):
        qa = np.ascontiguousarray(q[a])
        qp = orc._ptr(qa)
        d = np.array([lib.orc_l2_f32(qp, ptrs[i], base.shape[1]) for i in range(n)], np.float32)
        o = np.lexsort((np.arange(n), d))[:k]
        out_i[a, :len(o)], out_d[a, :len(o)] = o, d[o]
    return out_i, out_d


def exact_fast(orc, base, q, k, num_threads=16):
    """The same reference for larger inputs (n >= k): the ids from orc.exact_gt, which sorts by
    (distance, id) over every row, and orc_l2_f32 for the distances of those k rows."""
    lib = orc.lib()
    base = np.ascontiguousarray(base, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    assert len(base) >= k
    ids, _ = orc.exact_gt(base, q, k, num_threads=num_threads)
    d = np.zeros((len(q), k), np.float32)
    for a in range(len(q)):
        qp = orc._ptr(q[a])
        d[a] = [lib.orc_l2_f32(qp, orc._ptr(base[i]), base.shape[1]) for i in ids[a]]
    return ids.astype(np.uint32), d


def assert_exact(ids, dists, ref_i, ref_d, rows=None, what=""):
    """ids array_equal and distance bits array_equal as uint32 (over `rows` if given)."""
    ids, dists = np.asarray(ids), np.asarray(dists)
    if rows is not None:
        ids, dists, ref_i, ref_d = ids[rows], dists[rows], ref_i[rows], ref_d[rows]
    bad = np.nonzero((ids != ref_i).any(1) | (dists.view(np.uint32) != ref_d.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, (what, "wrong rows", bad[:8].tolist(), ids[bad[:1]], ref_i[bad[:1]])


def device_search(dev, q, k):
    """alaya_index_flat_search_device on the current torch stream: (ids, dists, flags) on the host."""
    import torch

    d0 = torch.device("cuda", 0)
    nq = len(q)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(d0)
    ids_d = torch.zeros((nq, k), dtype=torch.int32, device=d0)
    dd = torch.zeros((nq, k), dtype=torch.float32, device=d0)
    flags = torch.full((nq,), 7, dtype=torch.int32, device=d0)
    s = torch.cuda.current_stream(d0)
    dev.flat_search_device(qd.data_ptr(), nq, k, ids_d.data_ptr(), dd.data_ptr(), flags.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    f = flags.cpu().numpy()
    assert ((f == 0) | (f == 1)).all()  # every query's flag is written
    return ids_d.cpu().numpy().view(np.uint32), dd.cpu().numpy(), f


# ---- the near-tie sweep ------------------------------------------------------------------------
# (n, d, k): narrow rows at two strides, the big merge (k past the 32-entry shortlist) and the
# slabbed wide scan
SWEEP_SHAPES = [(4000, 64, 10), (4000, 128, 10), (3000, 64, 50), (2000, 960, 10)]
SWEEP_SIGMAS = [0.3, 0.1, 0.03, 0.01, 0.003, 0.001, 1e-5]
SWEEP_NQ = 48


def sweep_input(n, d, sigma, nq=SWEEP_NQ):
    """A cluster of width sigma around one point of the unit cube: the distances' spread shrinks
    with sigma^2 while each contraction's error bound stays at ~|q||b|, so the grid walks the gap
    between the k-th and the shortlist's last distance through the bound."""
    rng = np.random.default_rng(5)
    c = rng.random(d)
    base = np.ascontiguousarray((c + sigma * rng.standard_normal((n, d))).astype(np.float32))
    q = np.ascontiguousarray((c + sigma * rng.standard_normal((nq, d))).astype(np.float32))
    return base, q


def _f16_exp(maxabs):
    """f16_exp: t with |x| 2^t < 2^15 for every |x| <= maxabs (0 for zero or non-finite)."""
    maxabs = np.float32(maxabs)
    if not (maxabs > 0) or not (maxabs < np.float32(3.0e38)):
        return 0
    return 15 - int(np.frexp(maxabs)[1])


def shortlist_eps64(mode, base, q):
    """shortlist_eps restated in float64 for every query: the slack that the merge subtracts from
    (approximate cutoff + |q|^2) before it compares the k-th exact distance against it.  The
    constants are the kernel's; max_norm is capi.cpp's ensure_norms value; the query scale 2^t is
    per query in the warp-specialised scan and per wave of 32 queries in the single-role scan."""
    d = base.shape[1]
    stride = (d + 31) // 32 * 32
    contraction = contraction_of(mode, d)
    k_acc = float(stride)  # the slab widths 64/96/128 divide 960, the only wide row here
    assert stride <= 224 or stride == 960
    b64 = base.astype(np.float64)
    q64 = q.astype(np.float64)
    bmax = np.sqrt((b64 * b64).sum(1).max()) * 1.0001
    qn = (q64 * q64).sum(1)
    qnorm = np.sqrt(qn)
    gam = 2.0 * k_acc * 5.9604645e-8 * {1: 3.1, 2: 1.01, 0: 1.0}[contraction]
    eps = gam * (qn + bmax * bmax + 2.0 * qnorm * bmax)
    if contraction == 2:
        s = _f16_exp(bmax)
        qmax = np.abs(q).max(1)
        if "-ws" in mode:
            t = np.array([_f16_exp(m) for m in qmax])
        else:
            t = np.array([_f16_exp(qmax[a // 32 * 32:a // 32 * 32 + 32].max()) for a in range(len(q))])
        ab = 2.0 ** (-14 - s)
        aq = 2.0 ** (-14.0 - t)
        ec = (9.7680283e-4 + 2.4e-7) * qnorm * bmax + 1.0005 * np.sqrt(k_acc) * (ab * qnorm + aq * bmax) + k_acc * aq * ab
        eps = eps + 2.0 * 1.0001 * ec
    elif contraction == 1:
        eps = eps + 2.0 * 3.05 * 1.5258789e-5 * qnorm * bmax + 1e-30
    return eps


def shortlist_gap64(base, q, k):
    """Exact float64 gap between the k-th distance and the last one a merged shortlist can hold:
    the 32nd, or the 128th of the big merge's list (k > 24)."""
    last = 32 if k <= 24 else 128
    b64 = base.astype(np.float64)
    gap = np.zeros(len(q))
    for a in range(len(q)):
        diff = b64 - q[a].astype(np.float64)
        dd = np.partition((diff * diff).sum(1), (k - 1, last - 1))
        gap[a] = dd[last - 1] - dd[k - 1]
    return gap
