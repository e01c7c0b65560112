"""Shared by the exact range search tests (test_flat_range_host.py, test_flat_range.py,
test_index_exact_range.py): the numpy reference over the oracle's distances
(flat_filtered_common.distances: orc_l2_f32 / orc_ip_f32, the l2_sqr_avx2 / ip_sqr_avx2 order).  Per
query: the eligible rows (valid, allowed), those with d <= r as an f32 comparison, their count, the C
smallest ids when there are more than C, ordered by np.lexsort((ids, d)); the rest empty slots."""

import numpy as np

import flat_filtered_common as fc

FLT_MAX = fc.FLT_MAX
EMPTY = fc.EMPTY
PASS_ROWS = 32
CAP = 256 << 20
CHUNK_ENV = "ALAYA_FLAT_RANGE_CHUNK_ROWS"
STAGING_ENV = "ALAYA_FLAT_RANGE_STAGING_BYTES"


def from_distances(rows, dist, radii, cap):
    """rows: ascending eligible ids (m,); dist: (nq, m) f32 of those rows; radii: (nq,) f32.
    -> (counts uint32 (nq,), ids uint32 (nq, cap), dists f32 (nq, cap))."""
    rows = np.asarray(rows)
    dist = np.asarray(dist, np.float32)
    radii = np.asarray(radii, np.float32)
    nq = len(radii)
    counts = np.zeros(nq, np.uint32)
    out_i = np.full((nq, cap), EMPTY, np.uint32)
    out_d = np.full((nq, cap), FLT_MAX, np.float32)
    for a in range(nq):
        hit = np.nonzero(dist[a] <= radii[a])[0]  # f32 <= f32, inclusive; ascending id
        counts[a] = len(hit)
        hit = hit[:cap]  # the cap smallest ids
        o = hit[np.lexsort((rows[hit], dist[a][hit]))]
        out_i[a, :len(o)], out_d[a, :len(o)] = rows[o], dist[a][o]
    return counts, out_i, out_d


def reference(orc, metric, base, q, radii, cap, allow=None, valid=None, groups=None):
    """allow: None (no mask), bool (n,) or (G, n) with groups (nq,); valid: bool (n,) or None."""
    n = len(base)
    allow = np.ones((1, n), bool) if allow is None else np.atleast_2d(np.asarray(allow) != 0)
    live = np.ones(n, bool) if valid is None else np.asarray(valid) != 0
    groups = np.zeros(len(q), np.int64) if groups is None else np.asarray(groups)
    radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float32), (len(q),)))
    counts = np.zeros(len(q), np.uint32)
    out_i = np.full((len(q), cap), EMPTY, np.uint32)
    out_d = np.full((len(q), cap), FLT_MAX, np.float32)
    for g in range(len(allow)):
        qs = np.nonzero(groups == g)[0]
        rows = np.nonzero(allow[g] & live)[0]
        if len(qs) == 0 or len(rows) == 0:
            continue
        dist = fc.distances(orc, metric, base, q[qs], rows)
        counts[qs], out_i[qs], out_d[qs] = from_distances(rows, dist, radii[qs], cap)
    return counts, out_i, out_d


def assert_same(got, ref, what=""):
    """array_equal on counts, on ids and on distance bits, empty slots included."""
    counts, ids, dists = (np.asarray(a) for a in got)
    ref_c, ref_i, ref_d = ref
    assert counts.shape == ref_c.shape and ids.shape == ref_i.shape and dists.shape == ref_d.shape, what
    assert np.array_equal(counts, ref_c), (what, "counts", counts[:8], ref_c[:8])
    bad = np.nonzero((ids != ref_i).any(1) | (dists.view(np.uint32) != ref_d.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, (what, "wrong queries", bad[:8].tolist(), ids[bad[:1]], ref_i[bad[:1]], dists[bad[:1]],
                           ref_d[bad[:1]])


def csr_of(counts, ids, dists, cap):
    """The padded reference as (lims, ids, dists) of Index.exact_range_search's form."""
    kept = np.minimum(counts.astype(np.int64), cap)
    lims = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(kept, out=lims[1:])
    take = np.arange(cap)[None, :] < kept[:, None]
    return lims, ids[take], dists[take]
