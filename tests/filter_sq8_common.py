"""Shared by test_filter_sq8_host.py, test_filter_sq8_gpu.py and filter_shard_worker.py: the filtered SQ8
search restated in Python on the oracle's quantizer, code distance, LinearPool and f32 distance.

The restatement mirrors filter_common.replay with the code distance -- the query is encoded to codes
(``orc.sq8_encode``) and every distance is ``orc.sq8_dist`` of two code rows, with no validity test in the
distance itself (SQ8Space's QueryComputer has none) -- and, beside the traversal pool of capacity ef, a
candidate pool of capacity m: ``candidates.insert(v, d_sq8)`` for each pair the traversal hands to
``pool.insert``, in that order, when row v is valid and its allow bit is set.  The candidates are then
rescored with ``orc.dist`` of the rerank query and their f32 rows, and the answer is the first k under
(exact distance, id), equal pairs in pool order; empty slots hold (EMPTY, FLT_MAX).

Inputs (2000 rows, 12 queries): "gist" = filter_common.graph's rows; "coarse" = degree_common.rows with rows
0..3 multiplied by 16 before the build and the fit, which widens every dimension's range so the codes are
coarse and the rerank matters; "tie" = degree_common.tie_rows(dim, 3)."""

import numpy as np

import degree_common as dc
import filter_common as fc

EMPTY = fc.EMPTY
FLT_MAX = fc.FLT_MAX
N, NQ = fc.N, fc.NQ
_inputs = {}
_replays = {}


def default_pool(k, ef):
    return min(224, max(k, ef))


def rows(dim, kind):
    if kind == "coarse":
        base, queries = dc.rows(dim)
        base = base.copy()
        base[:4] *= 16.0
        return base, queries
    return fc.data(dim, kind)


def inputs(orc, dim, metric, kind="gist"):
    """(base, queries, arrays, (mn, mx, codes)) of a kind; the graph is orc.build_hnsw(base, metric, 32, 100)."""
    key = (dim, metric, kind)
    if key not in _inputs:
        if kind == "coarse":
            base, queries = rows(dim, kind)
            arrays = orc.build_hnsw(base, metric, 32, 100)
        else:
            base, queries, arrays = fc.graph(orc, dim, metric, kind)
        mn, mx = orc.sq8_fit(base)
        _inputs[key] = (base, queries, arrays, (mn, mx, orc.sq8_encode(base, mn, mx)))
    return _inputs[key]


def view_of(orc, base, arrays, metric, quant, order, valid=None):
    """The SQ8 IndexView of the input (oracle search of the same space) -- also what replay walks."""
    mn, mx, codes = quant
    return dc.view_of(orc, base, arrays, metric, sq8=(codes, mn, mx, order), valid=valid)


def rerank(orc, base, metric, rq, cand, k):
    """The first k of the candidates (pool order) under (exact f32 distance, id), equal pairs in pool order."""
    exact = [np.float32(orc.dist(metric, rq, base[v])) for v, _ in cand]
    order = sorted(range(len(cand)), key=lambda i: (float(exact[i]), cand[i][0], i))[:k]
    ids = np.full(k, EMPTY, np.uint32)
    dists = np.full(k, FLT_MAX, np.float32)
    for slot, i in enumerate(order):
        ids[slot], dists[slot] = cand[i][0], exact[i]
    return ids, dists


def replay(orc, view, quant, order, q, k, ef, m, allow, metric=0, rq=None, eps=None):
    """One query.  view: the graph and the f32 rows (view.base), its validity bitmap in view.valid; quant =
    (mn, mx, codes); order: the code distance's reduction order (1 AVX2, 2 AVX-512); rq: the rerank query
    (None = q).  Returns a dict: ids, dists (k slots), counters, pool (the traversal pool as (id, code
    distance)), cand (the candidate pool, the same pairs) and pairs (allowed, valid pairs in arrival order)."""
    mn, mx, codes = quant
    base, l0 = view.base, view.l0
    n = base.shape[0]
    valid = view.valid
    qc = orc.sq8_encode(q, mn, mx)[0]

    def is_valid(v):
        return valid is None or bool((valid[v >> 3] >> (v & 7)) & 1)

    def dist(v):  # code to code; a removed row has an ordinary distance
        return orc.sq8_dist(metric, qc, codes[v], mn, mx, order)

    pool = orc.Pool(n, ef)
    candidates = orc.Pool(n, m)
    pairs = []

    def insert(v, d):
        pool.insert(v, d)
        if is_valid(v) and allow[v]:
            candidates.insert(v, d)
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
    cand = [(candidates.id(i), np.float32(candidates.dist(i))) for i in range(candidates.size())]
    ids, dists = rerank(orc, base, metric, q if rq is None else rq, cand, k)
    return dict(ids=ids, dists=dists, counters=(n_dist, n_expand, n_dist_up, n_hops_up),
                pool=[(pool.id(i), np.float32(pool.dist(i))) for i in range(pool.size())], cand=cand, pairs=pairs)


def replays(orc, dim, metric, kind, order, k, ef, m, share):
    """replay of every query of an input under mask(N, share), cached per key."""
    key = (dim, metric, kind, order, k, ef, m, share)
    if key not in _replays:
        base, queries, arrays, quant = inputs(orc, dim, metric, kind)
        view = dc.view_of(orc, base, arrays, metric)
        allow = fc.mask(N, share)
        _replays[key] = [replay(orc, view, quant, order, q, k, ef, m, allow, metric) for q in queries]
    return _replays[key]


assert_matches = fc.assert_matches
