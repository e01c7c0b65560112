"""Shared by the exact filtered k-NN tests (test_flat_filtered_host.py, test_flat_filtered.py): the
reference -- the oracle's distance (orc.dist: orc_l2_f32 / orc_ip_f32, the l2_sqr_avx2 / ip_sqr_avx2
order) over the rows that are valid and allowed, then (distance, id) order, empty slots
(0xffffffff, FLT_MAX) -- and the inputs both files use.  References are computed once per key and
handed out read-only."""

import functools

import numpy as np

FLT_MAX = np.finfo(np.float32).max
EMPTY = 0xFFFFFFFF
PASS_ROWS = 32  # id-list entries one wave takes per pass: the smallest chunk
CAP = 256 << 20
_cache = {}


def cached(key, make):
    if key not in _cache:
        val = make()
        for a in val if isinstance(val, tuple) else (val,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = val
    return _cache[key]


def distances(orc, metric, base, q, rows):
    """orc.dist(metric, q[a], base[i]) for every query a and every i of `rows`: (nq, len(rows)) f32.
    (The library entries orc.dist calls, on row addresses: the same bits without a copy per pair.)"""
    lib = orc.lib()
    f = lib.orc_l2_f32 if metric == orc.L2 else lib.orc_ip_f32
    base = np.ascontiguousarray(base, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    d = base.shape[1]
    ptrs = [base[i].ctypes.data for i in rows]
    out = np.zeros((len(q), len(rows)), np.float32)
    for a in range(len(q)):
        qp = q[a].ctypes.data
        out[a] = [f(qp, p, d) for p in ptrs]
    return out


def reference(orc, metric, base, q, k, allow, valid=None, groups=None):
    """Query a's answer: the valid rows its mask allows, by (distance, id), the first k; the rest
    empty.  allow: bool (n,) or (G, n) with groups (nq,); valid: bool (n,) or None."""
    allow = np.atleast_2d(np.asarray(allow) != 0)
    n = len(base)
    assert allow.shape[1] == n
    live = np.ones(n, bool) if valid is None else np.asarray(valid) != 0
    groups = np.zeros(len(q), np.int64) if groups is None else np.asarray(groups)
    out_i = np.full((len(q), k), EMPTY, np.uint32)
    out_d = np.full((len(q), k), FLT_MAX, np.float32)
    for g in range(len(allow)):
        qs = np.nonzero(groups == g)[0]
        rows = np.nonzero(allow[g] & live)[0]
        if len(qs) == 0 or len(rows) == 0:
            continue
        dist = distances(orc, metric, base, q[qs], rows)
        for a, qa in enumerate(qs):
            o = np.lexsort((rows, dist[a]))[:k]
            out_i[qa, :len(o)], out_d[qa, :len(o)] = rows[o], dist[a][o]
    return out_i, out_d


def assert_same(ids, dists, ref_i, ref_d, what=""):
    """array_equal on ids and on distance bits."""
    ids = np.asarray(ids)
    dists = np.asarray(dists)
    bad = np.nonzero((ids != ref_i).any(1) | (dists.view(np.uint32) != ref_d.view(np.uint32)).any(1))[0]
    assert ids.shape == ref_i.shape and len(bad) == 0, (what, "wrong queries", bad[:8].tolist(), ids[bad[:1]],
                                                       ref_i[bad[:1]], dists[bad[:1]], ref_d[bad[:1]])


def random_mask(n, share, seed):
    rng = np.random.default_rng(seed)
    return rng.random(n) < share


def valid_bytes(valid):
    """The validity bitmap set_base takes: bit i % 8 of byte i // 8 = row i."""
    return np.packbits(np.asarray(valid, np.uint8), bitorder="little")


# ---- inputs both files use -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gist_rows(n, nq, dim):
    from workloads.datasets import gist_like

    base, q = gist_like(n, nq, dim=dim, n_centres=5)
    base = np.ascontiguousarray(base, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    base.setflags(write=False)
    q.setflags(write=False)
    return base, q


TIE_K = 50
TIE_KINDS = ["tie_rows", "duplicated"]


@functools.lru_cache(maxsize=None)
def tie_input(kind):
    """(base, queries, allow).  tie_rows: rows of {0, 1, 2}, most distances tie.  duplicated: every
    row twice (ids i and i + 1000), and a mask that allows one copy, the other, both or neither."""
    import degree_common

    if kind == "tie_rows":
        base, q = degree_common.tie_rows(32, 3)
        allow = random_mask(len(base), 0.5, 11)
    else:
        b, q = gist_rows(1000, 12, 48)
        base = np.ascontiguousarray(np.concatenate([b, b]))
        allow = random_mask(len(base), 0.6, 12)
    allow.setflags(write=False)
    return base, q, allow


def short_input():
    """9 allowed rows under k = 10."""
    base, q = gist_rows(2000, 12, 128)
    allow = np.zeros(len(base), bool)
    allow[[3, 40, 41, 500, 777, 1024, 1500, 1998, 1999]] = True
    return base, q, allow


def padding_words(n, allow):
    """pack_allow's words with every bit at a position >= n set as well."""
    from alayalite_amd.utils import pack_allow

    words = pack_allow(allow, n).copy()
    if n % 32:
        words[:, -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    return words
