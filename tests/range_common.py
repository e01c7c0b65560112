"""Shared by test_range_host.py and test_range_gpu.py: the range search restated on filter_common's replay.

A replay's ``pairs`` already is the stream the range search consumes: every (id, distance) the traversal
hands to its pool, entry offers included, whose row is valid and allowed, in arrival order.  So for a
radius r and a cap C: hits = the pairs with d <= r (f32, inclusive), counts = len(hits), and the stored
rows are hits[:C] -- the first C to arrive -- sorted by (float(d), id), then (EMPTY, FLT_MAX).  Replays
come from ``fc.replays`` with k = 10 so the cache is shared with the filter tests."""

import numpy as np

import degree_common as dc
import filter_common as fc

EMPTY, FLT_MAX = fc.EMPTY, fc.FLT_MAX
K = 10  # the replays' result pool: unused here, it keys the shared cache


def replays(orc, dim, metric, kind, ef, share=1.0, **kw):
    return fc.replays(orc, dim, metric, kind, K, ef, share, **kw)


def zero_query_replay(orc):
    """The all-zero query on the (64, IP) graph at ef 40: every distance is -(0 . b) = -0.0."""
    base, _, arrays = fc.graph(orc, 64, 1)
    view = dc.view_of(orc, base, arrays, 1)
    return replays(orc, 64, 1, "zero", 40, view=view, queries=[np.zeros(64, np.float32)], allow=np.ones(fc.N, bool))[0]


def hits(r, radius):
    radius = np.float32(radius)
    return [(v, d) for (v, d) in r["pairs"] if np.float32(d) <= radius]


def want_row(r, radius, cap):
    """(count, ids[cap], dists[cap]) of one replay."""
    h = hits(r, radius)
    kept = sorted(h[:cap], key=lambda p: (float(p[1]), p[0]))
    ids = np.full(cap, EMPTY, np.uint32)
    dists = np.full(cap, FLT_MAX, np.float32)
    for slot, (v, d) in enumerate(kept):
        ids[slot], dists[slot] = v, d
    return len(h), ids, dists


def radii_of(rs, radius):
    """One radius per replay: a scalar is broadcast."""
    radius = np.asarray(radius, np.float32)
    return np.broadcast_to(radius, (len(rs),))


def mth_distance(r, m):
    """The m-th smallest distance of a replay's pairs (m from 1)."""
    return sorted(np.float32(d) for _, d in r["pairs"])[m - 1]


def assert_matches(got, rs, radius, cap, what=""):
    """Device (counts, ids, dists, counters) against the restatement of every replay: counts, ids, distance
    bits, the empty tail (part of both rows) and the four counters."""
    counts, ids, dists, cnt = got
    assert len(counts) == len(rs) and ids.shape == (len(rs), cap) and dists.shape == (len(rs), cap), (what, ids.shape)
    for i, (r, rad) in enumerate(zip(rs, radii_of(rs, radius))):
        n, w_ids, w_d = want_row(r, rad, cap)
        assert int(counts[i]) == n, (what, i, int(counts[i]), n)
        assert np.array_equal(np.asarray(ids[i], np.uint32), w_ids), (what, i, ids[i], w_ids)
        assert np.array_equal(np.asarray(dists[i]).view(np.uint32), w_d.view(np.uint32)), (what, i, dists[i], w_d)
        kept = min(n, cap)
        assert (np.asarray(ids[i][kept:]) == EMPTY).all() and (np.asarray(dists[i][kept:]) == FLT_MAX).all(), (what, i)
        if cnt is not None:
            assert tuple(int(c) for c in cnt[i]) == tuple(r["counters"]), (what, i, cnt[i], r["counters"])
