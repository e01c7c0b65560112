"""Vector file IO, ground truth and recall (mirrors alayalite/utils.py, python/src/alayalite/utils.py:26-115)."""

from __future__ import annotations

import hashlib

import numpy as np

__all__ = ["load_fvecs", "load_ivecs", "calc_recall", "calc_gt", "calc_gt_device", "calc_range_gt_device", "md5", "pack_allow", "range_csr"]


def _load_vecs(file_path, dtype):
    raw = np.fromfile(file_path, dtype=np.int32)
    if raw.size == 0:
        return np.zeros((0, 0), dtype)
    dim = int(raw[0])
    rows = raw.reshape(-1, dim + 1)
    return rows[:, 1:].copy().view(dtype)


def load_fvecs(file_path):
    """fvecs: per vector an int32 dimension followed by that many float32 values."""
    return _load_vecs(file_path, np.float32)


def load_ivecs(file_path):
    """ivecs: per vector an int32 dimension followed by that many int32 values."""
    return _load_vecs(file_path, np.int32)


def calc_recall(result, gt_data):
    """Mean |result_i ∩ gt_i| / k over the rows (utils.py:78-84)."""
    rows, cols = result.shape
    hits = sum(len(set(result[i].tolist()) & set(gt_data[i].tolist())) for i in range(rows))
    return 1.0 * hits / (rows * cols)


def calc_gt(data, query, topk):
    """Exact top-k by float64 L2 (utils.py:99-105)."""
    gt = np.zeros((query.shape[0], topk), dtype=np.int32)
    base = data.astype(np.float64)
    for i in range(query.shape[0]):
        d = np.linalg.norm(base - query[i].astype(np.float64), axis=1)
        gt[i] = np.argsort(d)[:topk]
    return gt


_GT_METRICS = {"l2": 0, "ip": 1, "cos": 2}


def calc_gt_device(data, query, topk, device=0, metric="l2", allow=None):
    """Exact top-k on the MI355X: the flat MFMA path (IndexType::FLAT has no implementation in the
    reference; this is its exact search, find_exact_gt in include/utils/evaluate.hpp:29-62: the f32
    l2_sqr metric, ties by id).  Any dimension, 1 <= topk <= 224.  Returns (ids int32, distances
    float32).  Differs from calc_gt (float64 norms) only where two rows tie within f32 rounding.
    metric "ip" ranks by the f32 ip_sqr distance -(q.b); "cos" does the same on copies of both
    arrays normalised row by row as ``fit`` normalises them.

    ``allow`` (a bool array over the rows, shape (n,)) restricts the answer to the allowed rows:
    the same ids and distance bits as ``calc_gt_device(data[rows], ...)`` mapped through
    ``rows = nonzero(allow)``, slots past the allowed rows (-1, FLT_MAX), without a second copy of
    the rows -- a scan of the allowed rows, meant for small allowed shares; above a few per cent
    the unmasked call on a sub-base is faster."""
    if metric not in _GT_METRICS:
        raise ValueError(f"metric must be one of {sorted(_GT_METRICS)}, got {metric!r}")
    from . import _native

    data = np.ascontiguousarray(data, dtype=np.float32)
    query = np.ascontiguousarray(query, dtype=np.float32)
    if metric == "cos":
        data = _native._ext.normalize_rows(data)
        query = _native._ext.normalize_rows(query)
    ix = _native._ext.DeviceIndex(device)
    ix.set_base(data, _GT_METRICS[metric])
    if allow is not None:
        allow = np.asarray(allow)
        if allow.ndim != 1:
            raise ValueError(f"allow must have shape (n,), got {allow.shape}")
        ids, dists = ix.flat_search_filtered(query, topk, pack_allow(allow, data.shape[0]))
        return ids.astype(np.int32), dists
    ids, dists, _ = ix.flat_search(query, topk)
    return ids.astype(np.int32), dists


def exact_range_args(nq, radius, max_results, allow=None, groups=None):
    """The checks ``Index.exact_range_search`` and ``calc_range_gt_device`` make before anything reaches the
    device: ``radius`` a number or an array of shape (nq,), not NaN; 1 <= ``max_results`` <= 4096; ``groups``
    only with ``allow``.  Returns the radii as a contiguous float32 array of shape (nq,)."""
    radii = np.asarray(radius, np.float32)
    if radii.shape not in ((), (nq,)):
        raise ValueError(f"radius must be a number or have shape (nq,) = ({nq},), got {radii.shape}")
    if np.isnan(radii).any():
        raise ValueError("radius must not be NaN")
    if not 1 <= int(max_results) <= 4096:
        raise ValueError(f"max_results must be in 1..4096, got {max_results}")
    if allow is None and groups is not None:
        raise ValueError("groups needs allow")
    return np.ascontiguousarray(np.broadcast_to(radii, (nq,)))


def calc_range_gt_device(data, query, radius, max_results=4096, device=0, metric="l2", allow=None):
    """Every row within ``radius`` of each query, exactly, on the MI355X: ``Index.exact_range_search`` on raw
    arrays, beside ``calc_gt_device``.  A row is a hit when its f32 distance (``calc_gt_device``'s: l2_sqr,
    -(q.b) for "ip", the same on normalised copies for "cos") is ``<= radius``, inclusive; ``radius`` is a
    number or an array of shape (nq,), not NaN.  ``allow`` (a bool array over the rows, shape (n,)) restricts
    the hits to the allowed rows.  Returns ``(lims, ids int32, dists float32, counts uint32)`` in
    ``Index.range_search``'s form: ``counts[i]`` is the exact number of hits, never capped, and query i's rows
    ``ids[lims[i]:lims[i + 1]]`` are ``min(counts[i], max_results)`` of them by (distance, id).  Where
    ``counts[i] > max_results`` (1..4096) the list is truncated to the hits with the smallest ids, NOT the
    nearest.  The cost is rows x queries on the f32 scan of ``calc_gt_device(allow=)``, not the MFMA scan."""
    if metric not in _GT_METRICS:
        raise ValueError(f"metric must be one of {sorted(_GT_METRICS)}, got {metric!r}")
    query = np.ascontiguousarray(query, dtype=np.float32)
    radii = exact_range_args(query.shape[0], radius, max_results)
    words = None
    if allow is not None:
        allow = np.asarray(allow)
        if allow.ndim != 1:
            raise ValueError(f"allow must have shape (n,), got {allow.shape}")
        words = pack_allow(allow, np.shape(data)[0])
    from . import _native

    data = np.ascontiguousarray(data, dtype=np.float32)
    if metric == "cos":
        data = _native._ext.normalize_rows(data)
        query = _native._ext.normalize_rows(query)
    ix = _native._ext.DeviceIndex(device)
    ix.set_base(data, _GT_METRICS[metric])
    step = max(1, (1 << 26) // max_results)  # at most 2^26 padded result slots per call
    lims, ids, dists, counts = [np.zeros(1, np.int64)], [], [], []
    for lo in range(0, query.shape[0], step):
        c, i, d = ix.flat_range_search(query[lo:lo + step], radii[lo:lo + step], max_results, words)
        part = range_csr(c, i, d, max_results)
        lims.append(part[0][1:] + lims[-1][-1])
        ids.append(part[1].astype(np.int32))
        dists.append(part[2])
        counts.append(c)
    if not counts:
        return lims[0], np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.uint32)
    return np.concatenate(lims), np.concatenate(ids), np.concatenate(dists), np.concatenate(counts)


def pack_allow(allow, n):
    """Bool masks over n rows as the words ``filtered_search`` reads: uint32 [G, ceil(n / 32)], bit
    i % 32 of word i // 32 of a mask = row i (little bit order), padding bits zero.  ``allow`` has
    shape (n,) -- one mask, G = 1 -- or (G, n); any dtype, nonzero = allowed."""
    a = np.asarray(allow)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[0] < 1:
        raise ValueError(f"allow must have shape (n,) or (G, n) with G >= 1, got {np.asarray(allow).shape}")
    if n < 0 or a.shape[1] != n:
        raise ValueError(f"allow must cover the index's {n} rows, got {a.shape[1]}")
    words = (n + 31) // 32
    bits = np.zeros((a.shape[0], words * 32), np.uint8)
    bits[:, :n] = a != 0
    packed = np.packbits(bits, axis=1, bitorder="little")
    return np.ascontiguousarray(packed).view("<u4").astype(np.uint32, copy=False).reshape(a.shape[0], words)


def range_csr(counts, ids, dists, max_results):
    """The padded result of a ``range_search`` -- counts (nq,), ids and dists (nq, max_results) -- as the
    CSR form ``Index.range_search`` returns: (lims, ids, dists) with lims int64 of length nq + 1 and
    query i's rows at ``[lims[i]:lims[i + 1]]``, ``min(counts[i], max_results)`` of them, in the
    padded form's order.  ``counts[i] > max_results`` marks a truncated list."""
    counts = np.asarray(counts)
    ids, dists = np.asarray(ids), np.asarray(dists)
    nq = counts.shape[0]
    if counts.ndim != 1 or ids.shape != (nq, max_results) or dists.shape != (nq, max_results):
        raise ValueError(f"counts must have shape (nq,) and ids, dists (nq, {max_results}); "
                         f"got {counts.shape}, {ids.shape}, {dists.shape}")
    kept = np.minimum(counts.astype(np.int64), max_results)
    lims = np.zeros(nq + 1, np.int64)
    np.cumsum(kept, out=lims[1:])
    take = np.arange(max_results)[None, :] < kept[:, None]
    return lims, ids[take], dists[take]


def md5(arr, chunk_size=1024 * 1024):
    h = hashlib.md5()
    data = arr.tobytes()
    for i in range(0, len(data), chunk_size):
        h.update(data[i:i + chunk_size])
    return h.hexdigest()
