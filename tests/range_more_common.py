"""Shared by test_range_more_host.py and test_range_more_gpu.py: the radius-mode range search restated in
Python on the oracle's distance and LinearPool.

The rule (include/alaya_hip.h, alaya_index_range_search_radius), for a query with radius r, result cap C and
frontier cap F:

1. Phase 1 is filter_common.replay's loop: batch_search's traversal at ef, the same pops and the same four
   counters.  Every (id, d) it hands to its pool, entry offers included, whose row is valid and allowed is
   a pair; the pairs with d <= r (f32) are the hits, in arrival order.
2. Every (id, d) that phase 1 or phase 2 computes joins the frontier, in arrival order, when its row is
   valid and d <= r -- allowed or not.  ``frontier`` counts them, not capped; the first F are stored.  A
   removed row never joins; a repeated entry point joins twice.
3. Phase 2: when the pool has no unchecked entry left the stored frontier rows are expanded in arrival
   order, popped by phase 1 or not: the level-0 row is read, neighbours not yet visited are marked,
   measured in adjacency order and offered to the pairs and to the frontier.  Nothing goes into the pool.
   It ends when the cursor reaches the end of the stored frontier; ``more_dist`` counts its distances.
4. counts / the stored first C hits / their order are range_common.want_row's, on the pairs of both phases.

``dists_of`` caches orc.dist of a query against every row (the replays of one query at several radii and
caps read the same distances; a row's distance is a function of the two vectors alone)."""

import numpy as np

import degree_common as dc
import filter_common as fc
import range_common as rc

EMPTY, FLT_MAX = fc.EMPTY, fc.FLT_MAX
_rows = {}
_replays = {}


def dists_of(orc, key, base, queries, metric):
    """[nq, n] orc.dist of every (query, row), cached under `key`."""
    if key not in _rows:
        _rows[key] = np.array([[orc.dist(metric, q, b) for b in base] for q in queries], np.float32)
    return _rows[key]


def mth_exact(all_d, m, valid=None):
    """Per query, the exact m-th smallest distance over all (valid) rows (m from 1): replay-independent."""
    d = all_d if valid is None else all_d[:, valid]
    return np.sort(d, axis=1)[:, m - 1].astype(np.float32)


def replay(orc, view, q, ef, radius, max_frontier, allow, metric=0, eps=None, row_d=None):
    """One query.  row_d: this query's row of dists_of, or None to call orc.dist.  Returns a dict: pairs (the
    valid, allowed (id, dist) of both phases in arrival order: range_common's stream), pairs1 (phase 1's),
    front (the stored frontier ids), frontier, more_dist, counters (phase 1's four)."""
    base, l0 = view.base, view.l0
    n = base.shape[0]
    valid = view.valid
    radius = np.float32(radius)

    def is_valid(v):
        return valid is None or bool((valid[v >> 3] >> (v & 7)) & 1)

    def dist(v):  # QueryComputer: FLT_MAX for an invalid row
        if not is_valid(v):
            return FLT_MAX
        return np.float32(row_d[v]) if row_d is not None else orc.dist(metric, q, base[v])

    pool = orc.Pool(n, ef)
    pairs, front = [], []
    joined = 0

    def offer(v, d):
        nonlocal joined
        if not is_valid(v):
            return
        if allow[v]:
            pairs.append((v, d))
        if np.float32(d) <= radius:
            joined += 1
            if len(front) < max_frontier:
                front.append(v)

    def insert(v, d):
        pool.insert(v, d)
        offer(v, d)

    n_dist = n_expand = n_dist_up = n_hops_up = 0
    visited = set()
    if view.levels is not None:
        u = int(view.s.ep)
        cur = dist(u)
        n_dist_up += 1
        up_r = int(view.s.upper_R)
        for level in range(int(view.levels[u]), 0, -1):
            changed = True
            while changed:
                changed = False
                off = int(view.upper_off[u]) + (level - 1) * up_r
                n_hops_up += 1
                for v in view.upper_edges[off:off + up_r]:
                    if v == EMPTY:
                        break
                    d = dist(int(v))
                    n_dist_up += 1
                    if d < cur:
                        cur, nxt, changed = d, int(v), True
                if changed:
                    u = nxt
        insert(u, cur)
        visited.add(u)
    else:
        for e in eps:
            insert(int(e), dist(int(e)))
            n_dist_up += 1
            visited.add(int(e))
    while pool.has_next():
        node = pool.pop()
        n_expand += 1
        for v in l0[node]:
            if v == EMPTY:
                break
            v = int(v)
            if v in visited:
                continue
            visited.add(v)
            n_dist += 1
            insert(v, dist(v))
    n1 = len(pairs)
    # phase 2: the stored frontier, which grows while it is walked
    more = 0
    cursor = 0
    while cursor < len(front):
        node = front[cursor]
        cursor += 1
        for v in l0[node]:
            if v == EMPTY:
                break
            v = int(v)
            if v in visited:
                continue
            visited.add(v)
            more += 1
            offer(v, dist(v))
    return dict(pairs=pairs, pairs1=pairs[:n1], front=front, frontier=joined, more_dist=more,
                counters=(n_dist, n_expand, n_dist_up, n_hops_up), visited=len(visited))


def case(orc, dim, metric, kind="gist"):
    """(base, queries, arrays, view, all_d) of a filter_common graph."""
    base, queries, arrays = fc.graph(orc, dim, metric, kind)
    view = dc.view_of(orc, base, arrays, metric)
    return base, queries, arrays, view, dists_of(orc, (dim, metric, kind), base, queries, metric)


def replays(orc, dim, metric, kind, ef, radii, max_frontier=4096, share=1.0):
    """replay of every query of a filter_common input at its radius, cached per key."""
    radii = rc.radii_of(range(fc.NQ), radii)
    key = (dim, metric, kind, ef, radii.tobytes(), max_frontier, share)
    if key not in _replays:
        _, queries, _, view, all_d = case(orc, dim, metric, kind)
        allow = fc.mask(fc.N, share)
        _replays[key] = [replay(orc, view, q, ef, radii[i], max_frontier, allow, metric, row_d=all_d[i])
                         for i, q in enumerate(queries)]
    return _replays[key]


def assert_matches(got, rs, radius, cap, what=""):
    """Device (counts, ids, dists, counters, more) against the restatement: range_common's comparison on the
    longer hit stream, then (frontier, more_dist) of every query."""
    rc.assert_matches(got[:4], rs, radius, cap, what)
    more = got[4]
    assert more.shape == (len(rs), 2), (what, more.shape)
    for i, r in enumerate(rs):
        assert (int(more[i][0]), int(more[i][1])) == (r["frontier"], r["more_dist"]), \
            (what, i, more[i], r["frontier"], r["more_dist"])


def closed(l0, ids, in_radius):
    """The closure property: every level-0 neighbour of a row of `ids` that lies within the radius (the bool
    array in_radius over all rows) is in `ids` too.  A numpy walk of l0."""
    ids = np.asarray(ids, np.int64)
    have = np.zeros(len(in_radius), bool)
    have[ids] = True
    nb = l0[ids].ravel()
    nb = nb[nb != EMPTY].astype(np.int64)
    return bool((have[nb] | ~in_radius[nb]).all())
