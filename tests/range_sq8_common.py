"""Shared by test_range_sq8_host.py, test_range_sq8_gpu.py and range_shard_worker.py: the range search of an
SQ8 index restated on filter_sq8_common's replay.

A replay's ``pairs`` already is the stream the search consumes: every (id, code distance) the SQ8 traversal
hands to its pool, entry offers included, whose row is valid and allowed, in arrival order.  For a radius r,
a code radius c and a cap C:

  candidates = the pairs with float32(d_code) <= float32(c), in arrival order; cand = their number
  stored     = the first C candidates
  exact      = orc.dist(metric, rerank query, base[v]) of every stored pair
  hits       = the stored pairs with float32(exact) <= float32(r), by (float(exact), id); counts = their number

then (EMPTY, FLT_MAX).  The counters are the replay's.  Replays come from ``sc.replays`` / ``sc.replay`` with
k = 10 and m = 40, so the cache is shared with the filter tests."""

import numpy as np

import filter_sq8_common as sc

EMPTY, FLT_MAX = sc.EMPTY, sc.FLT_MAX
K, M = 10, 40  # the replays' result and candidate pools: unused here, they key the shared cache


def replays(orc, dim, metric, kind, order, ef, share=1.0):
    return sc.replays(orc, dim, metric, kind, order, K, ef, M, share)


def replay(orc, view, quant, order, q, ef, allow, metric=0, rq=None):
    return sc.replay(orc, view, quant, order, q, K, ef, M, allow, metric, rq=rq)


def code_radius(radius, slack):
    """float32(radius) + float32(slack), summed in float32: what Index.range_search hands to the device."""
    with np.errstate(over="ignore"):
        return np.float32(np.float32(radius) + np.float32(slack))


def candidates(pairs, c):
    c = np.float32(c)
    return [(v, d) for (v, d) in pairs if np.float32(d) <= c]


def exact_of(orc, base, metric, rq, pairs):
    return [np.float32(orc.dist(metric, rq, base[v])) for v, _ in pairs]


def want_row(orc, base, metric, rq, pairs, radius, c, cap):
    """(counts, cand, ids[cap], dists[cap]) of one query's pairs."""
    cands = candidates(pairs, c)
    stored = cands[:cap]
    exact = exact_of(orc, base, metric, rq, stored)
    radius = np.float32(radius)
    kept = sorted(((float(e), v, e) for (v, _), e in zip(stored, exact) if e <= radius), key=lambda t: (t[0], t[1]))
    ids = np.full(cap, EMPTY, np.uint32)
    dists = np.full(cap, FLT_MAX, np.float32)
    for slot, (_, v, e) in enumerate(kept):
        ids[slot], dists[slot] = v, e
    return len(kept), len(cands), ids, dists


def per_query(x, n):
    return np.broadcast_to(np.asarray(x, np.float32), (n,))


def mth_exact(orc, base, metric, rq, pairs, m):
    """The m-th smallest exact distance among a query's pairs (m from 1)."""
    return sorted(exact_of(orc, base, metric, rq, pairs))[m - 1]


def worst_overstatement(orc, base, metric, rq, pairs, radius):
    """The largest d_code - d_exact (float64) over the pairs whose exact distance is within the radius, 0 if
    none: a slack that, rounded up, makes each of them a candidate."""
    exact = exact_of(orc, base, metric, rq, pairs)
    gaps = [float(np.float32(d)) - float(e) for (_, d), e in zip(pairs, exact) if e <= np.float32(radius)]
    return max([0.0] + gaps)


def slack_above(radius, gap):
    """A float32 slack s >= 0 with float32(radius + s) >= radius + gap (as real numbers): the difference to the
    first float32 at or above radius + gap, nudged up until the float32 sum reaches it."""
    radius = np.float32(radius)
    target = float(radius) + max(gap, 0.0)
    c = np.float32(target)
    if float(c) < target:
        c = np.nextafter(c, np.float32(np.inf))
    s = np.float32(max(float(c) - float(radius), 0.0))
    while np.float32(radius + s) < c:
        s = np.nextafter(s, np.float32(np.inf))
    return s


def assert_matches(orc, got, rs, base, metric, rqs, radius, c, cap, what=""):
    """Device (counts, ids, dists, counters, cand) against the restatement of every replay: counts, cand, ids,
    exact distance bits, the empty tail and the four counters."""
    counts, ids, dists, cnt, cand = got
    n = len(rs)
    assert len(counts) == n and len(cand) == n and ids.shape == (n, cap) and dists.shape == (n, cap), (what, ids.shape)
    radius, c = per_query(radius, n), per_query(c, n)
    for i, r in enumerate(rs):
        w_n, w_cand, w_ids, w_d = want_row(orc, base, metric, rqs[i], r["pairs"], radius[i], c[i], cap)
        assert int(cand[i]) == w_cand, (what, i, int(cand[i]), w_cand)
        assert int(counts[i]) == w_n, (what, i, int(counts[i]), w_n)
        assert np.array_equal(np.asarray(ids[i], np.uint32), w_ids), (what, i, ids[i], w_ids)
        assert np.array_equal(np.asarray(dists[i]).view(np.uint32), w_d.view(np.uint32)), (what, i, dists[i], w_d)
        assert (np.asarray(ids[i][w_n:]) == EMPTY).all() and (np.asarray(dists[i][w_n:]) == FLT_MAX).all(), (what, i)
        if cnt is not None:
            assert tuple(int(x) for x in cnt[i]) == tuple(r["counters"]), (what, i, cnt[i], r["counters"])
