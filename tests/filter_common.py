"""Shared by test_filter_host.py and test_filter_gpu.py: the filtered graph search restated in Python on
the oracle's distance and LinearPool, and the inputs both files use.

The restatement is degree_common.replay -- the reference's search of one query -- with the traversal
pool an ``orc.Pool`` of capacity ef and, beside it, a second ``orc.Pool`` of capacity k, the result pool:
``result.insert(v, d)`` for each ``(v, d)`` the traversal hands to ``pool.insert``, in that order, when
row v is valid and its allow bit is set.  Rows: gist_like(2000, 12, dim, 5 centres) and
degree_common.tie_rows(dim, 3); graphs: orc.build_hnsw(base, metric, 32, 100), once per key."""

import numpy as np

import degree_common as dc

EMPTY = dc.EMPTY
FLT_MAX = np.float32(np.finfo(np.float32).max)
N, NQ = dc.N, dc.NQ
_graphs = {}
_replays = {}


def mask(n, share):
    """The allow mask of a share of the rows: 1.0 = all ones, 0.0 = all zero."""
    if share >= 1.0:
        return np.ones(n, bool)
    if share <= 0.0:
        return np.zeros(n, bool)
    return np.random.default_rng(100 + round(1000 * share)).random(n) < share


def data(dim, kind="gist"):
    """(base, queries) of a kind: "gist" or "tie"."""
    if kind == "tie":
        return dc.tie_rows(dim, 3)
    return dc.rows(dim)


def graph(orc, dim, metric, kind="gist"):
    """(base, queries, arrays) with arrays = (l0, levels, upper_off, upper_edges, ep, upper_R)."""
    key = (dim, metric, kind)
    if key not in _graphs:
        base, queries = data(dim, kind)
        _graphs[key] = (base, queries, orc.build_hnsw(base, metric, 32, 100))
    return _graphs[key]


def replay(orc, view, q, k, ef, allow, metric=0, eps=None):
    """One query; eps: the entry points of a graph without overlay (view.levels is None), each inserted
    in turn, repeats included (Graph::initialize_search).  Returns a dict: ids, dists (k slots; empty
    ones (EMPTY, FLT_MAX)), counters (n_dist, n_expand, n_dist_upper, n_hops_upper), pool (the final traversal pool as (id, dist) pairs) and
    pairs (the allowed, valid (id, dist) in arrival order)."""
    base, l0 = view.base, view.l0
    n = base.shape[0]
    valid = view.valid

    def is_valid(v):
        return valid is None or bool((valid[v >> 3] >> (v & 7)) & 1)

    def dist(v):  # QueryComputer: FLT_MAX for an invalid row
        return orc.dist(metric, q, base[v]) if is_valid(v) else FLT_MAX

    pool = orc.Pool(n, ef)
    result = orc.Pool(n, k)
    pairs = []

    def insert(v, d):
        pool.insert(v, d)
        if is_valid(v) and allow[v]:
            result.insert(v, d)
            pairs.append((v, d))

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
    size = result.size()
    ids = np.full(k, EMPTY, np.uint32)
    dists = np.full(k, FLT_MAX, np.float32)
    for i in range(size):
        ids[i] = result.id(i)
        dists[i] = result.dist(i)
    return dict(ids=ids, dists=dists, counters=(n_dist, n_expand, n_dist_up, n_hops_up),
                pool=[(pool.id(i), np.float32(pool.dist(i))) for i in range(pool.size())], pairs=pairs)


def replays(orc, dim, metric, kind, k, ef, share, view=None, queries=None, allow=None, eps=None):
    """replay of every query of an input, cached per key (the GPU cases and the host conditions share
    them).  view / queries / allow replace the key's own (then nothing is cached)."""
    key = (dim, metric, kind, k, ef, share)
    if view is None and key in _replays:
        return _replays[key]
    if view is None:
        base, queries, arrays = graph(orc, dim, metric, kind)
        own_view = dc.view_of(orc, base, arrays, metric)
        out = [replay(orc, own_view, q, k, ef, mask(N, share), metric) for q in queries]
        _replays[key] = out
        return out
    return [replay(orc, view, q, k, ef, allow, metric, eps) for q in queries]


def stable_first_k(pairs, k):
    """The first k of the pairs under a stable sort by distance (ties in arrival order)."""
    order = sorted(range(len(pairs)), key=lambda i: (float(pairs[i][1]), i))[:k]
    ids = np.full(k, EMPTY, np.uint32)
    dists = np.full(k, FLT_MAX, np.float32)
    for slot, i in enumerate(order):
        ids[slot], dists[slot] = pairs[i]
    return ids, dists


def assert_matches(got, want, what=""):
    """Device (ids, dists, counters) rows against the restatement's, every query: ids, distance bits,
    the four counters."""
    ids, dists, cnt = got
    assert len(ids) == len(want)
    for i, r in enumerate(want):
        assert np.array_equal(np.asarray(ids[i], np.uint32), r["ids"]), (what, i, ids[i], r["ids"])
        assert np.array_equal(np.asarray(dists[i]).view(np.uint32), r["dists"].view(np.uint32)), (what, i, dists[i], r["dists"])
        if cnt is not None:
            assert tuple(int(c) for c in cnt[i]) == tuple(r["counters"]), (what, i, cnt[i], r["counters"])
