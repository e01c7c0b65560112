"""Shared by test_filter_hop_host.py and test_filter_hop_gpu.py: the through search -- the filtered graph
search that expands through disallowed neighbours (include/alaya_hip.h, alaya_index_filtered_search_hop) --
restated in Python on the oracle's distance and LinearPool.  Inputs, graphs and ``mask(n, share)`` are
filter_common's.

passable(v): v's allow bit is set and v is valid.  Per pop the direct row's neighbours not yet visited are
marked visited; the passable ones are measured and inserted into the traversal pool (capacity ef) and the
result pool (capacity k), the others form the pop's through list.  Then each through row is walked for
passable rows not yet visited, which are marked, measured and inserted; a row that is not passable is
skipped there without a mark.  One level only."""

import numpy as np

import degree_common as dc
import filter_common as fc

EMPTY, FLT_MAX, N, NQ = fc.EMPTY, fc.FLT_MAX, fc.N, fc.NQ
mask, graph, data, stable_first_k = fc.mask, fc.graph, fc.data, fc.stable_first_k
_replays = {}
# the GPU file's main grid; test_filter_hop_host.py asserts what these inputs reach
KEFS = [(10, 16, 0.1), (10, 64, 0.02), (1, 8, 0.5), (32, 16, 0.2), (224, 64, 1.0)]
SHAPES = [(16, 0), (64, 0), (128, 1), (960, 0)]  # chunks 0, 4, 8 and 30


def _raw(l0, node):
    """A level-0 row to its first empty slot."""
    out = []
    for v in l0[node]:
        if v == EMPTY:
            break
        out.append(int(v))
    return out


def _row(l0, node, dedup):
    """The row as the search walks it; dedup: the first occurrence of an id only."""
    raw = _raw(l0, node)
    return list(dict.fromkeys(raw)) if dedup else raw


def replay(orc, view, q, k, ef, allow, metric=0, eps=None, dedup=None):
    """One query (filter_common.replay's arguments).  dedup: the graph is flagged for repeated edges (None =
    some row repeats an id, which is when set_graph flags it).  Returns a dict: ids, dists (k slots; empty
    ones (EMPTY, FLT_MAX)), counters (n_dist, n_expand, n_dist_upper, n_hops_upper, n_through), pool (the
    final traversal pool as (id, dist) pairs), pairs (the (id, dist) offered to the result pool, in arrival
    order), entries (the level-0 entries) and what the exercise conditions count over the pops: flush_pops
    (through rows yielded more than 64 candidates), empty_through (no through row), cross_dups (a row offered
    by two through rows of one pop) and dup_through (a through row that repeats an id which is passable and
    not yet visited when the row is walked, so only the repeated-edge filter keeps it from arriving twice)."""
    base, l0 = view.base, view.l0
    n = base.shape[0]
    valid = view.valid
    if dedup is None:
        dedup = graph_repeats(l0)

    def is_valid(v):
        return valid is None or bool((valid[v >> 3] >> (v & 7)) & 1)

    def passable(v):
        return bool(allow[v]) and is_valid(v)

    def dist(v):  # QueryComputer: FLT_MAX for an invalid row
        return orc.dist(metric, q, base[v]) if is_valid(v) else FLT_MAX

    pool = orc.Pool(n, ef)
    result = orc.Pool(n, k)
    pairs = []

    def offer(v, d):
        result.insert(v, d)
        pairs.append((v, d))

    n_dist = n_expand = n_dist_up = n_hops_up = n_through = 0
    visited = set()
    entries = []
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
        entry_pairs = [(u, cur)]
    else:
        entry_pairs = []
        for e in eps:
            entry_pairs.append((int(e), dist(int(e))))
            n_dist_up += 1
    for v, d in entry_pairs:  # into the pool whatever the bit; offered only when passable
        pool.insert(v, d)
        if passable(v):
            offer(v, d)
        visited.add(v)
        entries.append(v)

    flush_pops = empty_through = cross_dups = dup_through = 0
    while pool.has_next():
        node = pool.pop()
        n_expand += 1
        through = []
        for v in _row(l0, node, dedup):
            if v in visited:
                continue
            visited.add(v)
            if passable(v):
                d = dist(v)
                n_dist += 1
                pool.insert(v, d)
                offer(v, d)
            else:
                through.append(v)
        empty_through += not through
        got = {}  # passable rows this pop's through pass marked: the through row that did
        n_cand = 0
        for w in through:
            n_through += 1
            raw = _raw(l0, w)
            dup_through += any(raw.count(x) > 1 and passable(x) and x not in visited for x in set(raw))
            for x in _row(l0, w, dedup):
                if not passable(x):
                    continue
                if x in visited:
                    cross_dups += x in got and got[x] != w
                    continue
                visited.add(x)
                got[x] = w
                d = dist(x)
                n_dist += 1
                n_cand += 1
                pool.insert(x, d)
                offer(x, d)
        flush_pops += n_cand > 64
    size = result.size()
    ids = np.full(k, EMPTY, np.uint32)
    dists = np.full(k, FLT_MAX, np.float32)
    for i in range(size):
        ids[i] = result.id(i)
        dists[i] = result.dist(i)
    return dict(ids=ids, dists=dists, counters=(n_dist, n_expand, n_dist_up, n_hops_up, n_through),
                pool=[(pool.id(i), np.float32(pool.dist(i))) for i in range(pool.size())], pairs=pairs, entries=entries,
                flush_pops=flush_pops, empty_through=empty_through, cross_dups=cross_dups, dup_through=dup_through)


def graph_repeats(l0):
    """Some level-0 row repeats an id before its first empty slot (set_graph then flags the graph)."""
    for node in range(len(l0)):
        raw = _raw(l0, node)
        if len(set(raw)) != len(raw):
            return True
    return False


def replays(orc, dim, metric, kind, k, ef, share, view=None, queries=None, allow=None, eps=None):
    """replay of every query of an input, cached per key (the GPU cases and the host conditions share them).
    view / queries / allow replace the key's own (then nothing is cached)."""
    key = (dim, metric, kind, k, ef, share)
    if view is None and key in _replays:
        return _replays[key]
    if view is None:
        base, queries, arrays = graph(orc, dim, metric, kind)
        own_view = dc.view_of(orc, base, arrays, metric)
        dedup = graph_repeats(own_view.l0)
        out = [replay(orc, own_view, q, k, ef, mask(N, share), metric, dedup=dedup) for q in queries]
        _replays[key] = out
        return out
    dedup = graph_repeats(view.l0)
    return [replay(orc, view, q, k, ef, allow, metric, eps, dedup) for q in queries]


def assert_matches(got, want, what=""):
    """Device (ids, dists, counters, n_through) rows against the restatement's, every query: ids, distance
    bits, the four counters and n_through, all equal."""
    ids, dists, cnt, thr = got
    assert len(ids) == len(want) == len(cnt) == len(thr)
    for i, r in enumerate(want):
        assert np.array_equal(np.asarray(ids[i], np.uint32), r["ids"]), (what, i, ids[i], r["ids"])
        assert np.array_equal(np.asarray(dists[i]).view(np.uint32), r["dists"].view(np.uint32)), (what, i, dists[i], r["dists"])
        assert tuple(int(c) for c in cnt[i]) == tuple(r["counters"][:4]), (what, i, cnt[i], r["counters"])
        assert int(thr[i]) == r["counters"][4], (what, i, thr[i], r["counters"])


def recall(rows, truth):
    """Mean share of each query's true ids among its returned ids."""
    return float(np.mean([len(set(int(v) for v in r["ids"] if v != EMPTY) & set(t)) / len(t) for r, t in zip(rows, truth)]))


def exact_allowed(base, queries, allow, k):
    """The float64 L2 top-k over base[allow] of every query, as ids of base."""
    idx = np.nonzero(allow)[0]
    b = base[idx].astype(np.float64)
    out = []
    for q in queries:
        d = ((b - q.astype(np.float64)) ** 2).sum(1)
        out.append([int(v) for v in idx[np.argsort(d, kind="stable")[:k]]])
    return out
