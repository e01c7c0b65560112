"""Shared by test_search_degree.py: small gist-shaped inputs with level-0 rows of every width 1..64,
their graphs, oracle views and device indexes (built once per key), and the search's restatement that
counts how many expansions hand the kernel more than 32 (one screen pass) or 48 fresh candidates."""

import functools

import numpy as np

EMPTY = 0xFFFFFFFF
N, NQ = 2000, 12
_built = {}
_derived = {}


@functools.lru_cache(maxsize=None)
def rows(dim):
    """gist_like(2000, 12, dim, 5 centres): (base, queries), read-only."""
    from workloads.datasets import gist_like

    base, queries = gist_like(N, NQ, dim=dim, n_centres=5)
    base.setflags(write=False)
    queries.setflags(write=False)
    return base, queries


@functools.lru_cache(maxsize=None)
def tie_rows(dim, seed):
    """Rows of {0, 1, 2}: most distances tie, so the merge's (distance, arrival) order decides."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 3, (N, dim)).astype(np.float32)
    queries = rng.integers(0, 3, (NQ, dim)).astype(np.float32)
    queries[:4] = base[:4]  # exact hits: distance 0 ties among duplicates
    base.setflags(write=False)
    queries.setflags(write=False)
    return base, queries


def built(native, dim, metric, R, data=None):
    """Graph.build(base, metric, R, 100, 8, 100) of the shape's rows: (base, queries, arrays), arrays =
    (l0, levels, upper_off, upper_edges, ep, upper_R).  `data` = (name, base, queries) replaces rows(dim)."""
    key = (dim, metric, R, data[0] if data else None)
    if key not in _built:
        base, queries = (data[1], data[2]) if data else rows(dim)
        l0, levels, off, ue, ep, upper_r, _ = native.Graph.build(base, metric, R, 100, 8, 100).arrays()
        assert l0.shape == (N, R) and upper_r == R
        _built[key] = (base, queries, (l0, levels, off, ue, ep, upper_r))
    return _built[key]


def truncated(native, dim, metric, width):
    """The R = 64 build with every level-0 row cut to its first `width` entries (odd widths: rows
    that start at no multiple of 16 bytes); the overlay keeps upper_R = 64."""
    base, queries, (l0, levels, off, ue, ep, upper_r) = built(native, dim, metric, 64)
    return base, queries, (np.ascontiguousarray(l0[:, :width]), levels, off, ue, ep, upper_r)


def exact_neighbours(base, k):
    """Ids of the k nearest other rows of every row under L2 (float64, stable argsort, self excluded)."""
    b = base.astype(np.float64)
    sq = (b * b).sum(1)
    d = sq[:, None] + sq[None, :] - 2.0 * (b @ b.T)
    np.fill_diagonal(d, np.inf)
    return np.ascontiguousarray(np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.uint32))


def dense(native, dim, metric=0):
    """The R = 64 build's overlay over exact 64-NN level-0 rows: every row full, and early in a search
    nearly all 64 neighbours of a popped node are fresh."""
    key = ("dense", dim, metric)
    if key not in _derived:
        base, queries, (_, levels, off, ue, ep, upper_r) = built(native, dim, metric, 64)
        _derived[key] = (base, queries, (exact_neighbours(base, 64), levels, off, ue, ep, upper_r))
    return _derived[key]


def duplicated(native, dim, metric=0):
    """test_gpu.test_duplicate_edges_dedup's edit on the R = 64 build: every third row of 40..63 entries
    repeats its first neighbour after its last (set_graph then turns the kernel's dedup loop on)."""
    key = ("dup", dim, metric)
    if key not in _derived:
        base, queries, (l0, levels, off, ue, ep, upper_r) = built(native, dim, metric, 64)
        l0 = l0.copy()
        edited = 0
        for u in range(0, N, 3):
            cnt = int((l0[u] != EMPTY).sum())
            if 40 <= cnt < 64:
                l0[u, cnt] = l0[u, 0]
                edited += 1
        _derived[key] = (base, queries, (l0, levels, off, ue, ep, upper_r), edited)
    return _derived[key][:3]


def duplicated_rows_edited(native, dim, metric=0):
    duplicated(native, dim, metric)
    return _derived[("dup", dim, metric)][3]


def graph_of(native, arrays):
    l0, levels, off, ue, ep, upper_r = arrays
    return native.Graph.from_arrays(l0, levels, off, ue, upper_r, ep)


def view_of(orc, base, arrays, metric=0, **kw):
    l0, levels, off, ue, ep, upper_r = arrays
    return orc.IndexView(base, l0, levels, off, ue, upper_r, ep, metric=metric, **kw)


def device_of(native, base, arrays, metric=0):
    dev = native.DeviceIndex(0)
    dev.set_base(base, metric, None)
    dev.set_graph(graph_of(native, arrays))
    return dev


def check(view, dev, queries, k, ef):
    """tests/test_gpu.py::_check: ids, distance bits and the four counters against the oracle."""
    ids, dists, cnt = dev.search(queries, k, ef)
    for i, q in enumerate(queries):
        r_ids, r_d, r_c = view.search(q, k, ef, with_counters=True)
        assert np.array_equal(ids[i], r_ids), (i, ids[i], r_ids)
        assert np.array_equal(dists[i].view(np.uint32), r_d.view(np.uint32)), (i, dists[i], r_d)
        assert tuple(cnt[i]) == tuple(r_c), (i, cnt[i], r_c)
    return ids, dists, cnt


def int_bounds(native, base, queries):
    """The integer screen's bound (ALAYA_SEARCH_SCREEN=9) of every (query, row) pair, [nq, n], made on the
    host by the functions the kernel calls (alaya_screen_int_bound): a function of the two vectors alone,
    over exact integer sums, so the device's bound of a pair has these bits."""
    out = np.empty((len(queries), len(base)), np.float32)
    for i, q in enumerate(queries):
        out[i] = native.screen_int_bound(np.ascontiguousarray(np.broadcast_to(q, base.shape)), base)[2]
    return out


def replay(orc, view, q, ef, bounds=None):
    """test_search_screen._replay (the reference's L2 search of one query on the oracle's distance),
    counting what the degree tests need.  Returns a dict: ids (the pool), n_dist, n_expand, screened
    (candidates of expansions that began with a full pool), over32 / over48 (such expansions with more
    than 32 / 48 fresh candidates), any32 / any48 (expansions with more than 32 / 48 fresh candidates,
    whatever the pool held), most (the largest fresh count of any expansion), and -- given bounds, this
    query's row of int_bounds -- out9: the screened candidates whose bound is positive and reaches the
    pool's worst distance at the start of their expansion, which is the kernel's rule for dropping one."""
    base, l0 = view.base, view.l0
    u = int(view.s.ep)
    cur = orc.l2(q, base[u])
    up_r = int(view.s.upper_R)
    for level in range(int(view.levels[u]), 0, -1):
        changed = True
        while changed:
            changed = False
            off = int(view.upper_off[u]) + (level - 1) * up_r
            for v in view.upper_edges[off:off + up_r]:
                if v == EMPTY:
                    break
                d = orc.l2(q, base[v])
                if d < cur:
                    cur, nxt, changed = d, int(v), True
            if changed:
                u = nxt
    pool = [[cur, u, False]]  # sorted (dist, id, checked), capacity ef (LinearPool)
    visited = {u}
    pos = 0
    out = dict(n_dist=0, n_expand=0, screened=0, over32=0, over48=0, any32=0, any48=0, most=0, out9=0)
    while pos < len(pool):
        pool[pos][2] = True
        node = pool[pos][1]
        while pos < len(pool) and pool[pos][2]:
            pos += 1
        out["n_expand"] += 1
        full = len(pool) == ef
        tau = pool[-1][0]
        fresh = 0
        for v in l0[node]:
            if v == EMPTY:
                break
            v = int(v)
            if v in visited:
                continue
            visited.add(v)
            fresh += 1
            if full and bounds is not None and bounds[v] > 0 and bounds[v] >= tau:
                out["out9"] += 1
            d = orc.l2(q, base[v])
            if len(pool) == ef and d >= pool[-1][0]:
                continue
            at = len(pool)
            while at > 0 and pool[at - 1][0] > d:
                at -= 1
            pool.insert(at, [d, v, False])
            del pool[ef:]
            pos = min(pos, at)
        out["n_dist"] += fresh
        out["most"] = max(out["most"], fresh)
        out["any32"] += fresh > 32
        out["any48"] += fresh > 48
        if full:
            out["screened"] += fresh
            out["over32"] += fresh > 32
            out["over48"] += fresh > 48
    out["ids"] = [p[1] for p in pool]
    return out


def replay_totals(orc, view, queries, ef, bounds=None):
    """replay summed over the queries (ids dropped); bounds = int_bounds of the same rows and queries."""
    tot = dict(n_dist=0, n_expand=0, screened=0, over32=0, over48=0, any32=0, any48=0, most=0, out9=0)
    for i, q in enumerate(queries):
        r = replay(orc, view, q, ef, None if bounds is None else bounds[i])
        for key in tot:
            tot[key] = max(tot[key], r[key]) if key == "most" else tot[key] + r[key]
    return tot
