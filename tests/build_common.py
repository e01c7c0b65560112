"""Shared by the graph-construction suites (test_gpu_build.py, test_gpu_build_batched.py,
test_oracle_build_batched.py): the structural invariants of a built graph, the inputs that tell the
batched build's rules apart, and the CPU restatement's graph for each of them, computed once."""

import functools

import numpy as np

EMPTY = 0xFFFFFFFF
SEED = 100  # level-draw seed of every build here (the reference's default)


def check_structure(arrays, n, R):
    """Level-0 rows hold <= R distinct ids != self with -1 only as trailing padding; upper lists hold
    <= R/2 ids of nodes that exist on that level; the entry point is a node of the top level.
    `arrays` is Graph.arrays() or the restatement's tuple (same leading layout)."""
    l0, levels, off, ue, ep, upper_r = arrays[:6]
    assert l0.shape == (n, R) and upper_r == R
    for i in range(n):
        row = l0[i]
        cnt = int(np.argmax(row == EMPTY)) if (row == EMPTY).any() else R
        assert (row[cnt:] == EMPTY).all(), i
        live = row[:cnt]
        assert (live < n).all() and i not in live and len(set(live.tolist())) == cnt, i
    top = int(levels.max())
    assert levels[ep] == top
    for i in np.nonzero(levels)[0]:
        for lv in range(1, int(levels[i]) + 1):
            lst = ue[int(off[i]) + (lv - 1) * R: int(off[i]) + lv * R]
            live = lst[lst != EMPTY]
            assert len(live) <= R // 2 and (lst[len(live):] == EMPTY).all()
            assert i not in live and all(levels[v] >= lv for v in live), (i, lv)
    return l0, levels


def exact_topk(base, q, k, metric):
    b = base.astype(np.float64)
    out = []
    for v in q.astype(np.float64):
        d = ((b - v) ** 2).sum(1) if metric == 0 else -(b @ v)
        out.append(np.argsort(d, kind="stable")[:k])
    return np.array(out)


def recall(ids, gt):
    return np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(ids, gt)])


# ---- inputs --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uniform(n, d, seed):
    """Tie-free rows, U[0, 1)."""
    base = np.random.default_rng(seed).random((n, d), dtype=np.float32)
    base.setflags(write=False)
    return base


HUB_ROW = 7
# Level-draw seed of the hub builds.  With batch_div = 1 the batch doubles unless a point raises the
# max level and closes it early; under this seed, at M = 16 and at M = 32 alike, one batch is exactly
# rows 256..511 (cluster points only, met by a graph of the 256 spread rows only), and the upper-level
# entry of most of them is a spread row.  (Where the descent ends on a batch mate that joined an upper
# level a step earlier, the level-0 search starts from a still empty row and finds nothing else.)
HUB_SEED = 68


@functools.lru_cache(maxsize=None)
def hub():
    """768 x 16.  Rows 0..255 are uniform; rows 256..767 are a cluster around row 7 whose radius
    (<= 1e-3 per coordinate) is far below row 7's nearest-neighbour distance among rows 0..255, so
    a cluster point whose search reaches row 7 before any cluster point is in the graph selects it.  With batch_div = 1 the batch after 256 points holds 256 of
    them: one apply step brings row 7 hundreds of reverse edges (groups of 64, a prune between
    them), and the next batch and the refine passes meet a neighbourhood of near-equal candidates."""
    rng = np.random.default_rng(41)
    spread = rng.random((256, 16), dtype=np.float32)
    nn = np.sort(((spread - spread[HUB_ROW]) ** 2).sum(1))[1]
    assert nn > 0.05  # squared; the cluster's squared radius is <= 16e-6
    cluster = spread[HUB_ROW] + rng.uniform(-1e-3, 1e-3, (512, 16)).astype(np.float32)
    base = np.ascontiguousarray(np.concatenate([spread, cluster]), np.float32)
    base.setflags(write=False)
    return base


@functools.lru_cache(maxsize=None)
def tied_integers():
    """2000 x 64 rows of {0, 1, 2}: most distances tie, so the pool's arrival order and the prune's
    id order decide the graph."""
    base = np.random.default_rng(43).integers(0, 3, (2000, 64)).astype(np.float32)
    base.setflags(write=False)
    return base


@functools.lru_cache(maxsize=None)
def duplicate_block():
    """1000 random rows followed by 500 exact copies of the all-ones row (8-d): zero distances among
    the copies, and every copy is equally far from any other row."""
    rng = np.random.default_rng(47)
    base = np.concatenate([rng.random((1000, 8), dtype=np.float32), np.ones((500, 8), np.float32)])
    base = np.ascontiguousarray(base)
    base.setflags(write=False)
    return base


INPUTS = {"hub": hub, "tied_integers": tied_integers, "duplicate_block": duplicate_block}


def rows_of(spec):
    """spec = a name in INPUTS, or ("uniform", n, d, seed)."""
    return INPUTS[spec]() if isinstance(spec, str) else uniform(*spec[1:])


@functools.lru_cache(maxsize=None)
def _restated(spec, metric, R, efc, batch_div, max_batch, refine, seed):
    import oracle

    return oracle.build_hnsw_batched(rows_of(spec), metric, R, efc, seed, batch_div, max_batch, refine)


def restated(spec, metric=0, R=32, efc=100, batch_div=0, max_batch=0, refine=2, seed=SEED):
    """The restatement's (l0, levels, upper_off, upper_edges, ep, upper_R, stats) for one input and
    one parameter set; computed once per session and shared (treat the arrays as read-only)."""
    return _restated(spec, metric, R, efc, batch_div, max_batch, refine, seed)


# ---- device side ---------------------------------------------------------------------------------
PINNED_STATS = ("batches", "max_batch", "max_level", "prunes", "appends", "heuristic_dists")


def assert_graph_equals(g, stats, ref):
    """Exact equality of a device-built graph (Graph + stats dict) with the restatement's tuple."""
    l0, levels, off, ue, ep, upper_r = g.arrays()[:6]
    assert np.array_equal(levels, ref[1])
    assert np.array_equal(off, ref[2])
    assert (ep, upper_r) == (ref[4], ref[5]), (ep, upper_r, ref[4], ref[5])
    bad = np.nonzero((l0 != ref[0]).any(axis=1))[0]
    assert bad.size == 0, (bad.size, int(bad[0]), l0[bad[0]], ref[0][bad[0]])
    assert np.array_equal(l0, ref[0])
    bad = np.nonzero(ue != ref[3])[0] if ue.shape == ref[3].shape else np.array([-1])
    assert bad.size == 0, (bad.size, int(bad[0]))
    assert np.array_equal(ue, ref[3])
    got = {k: int(stats[k]) for k in PINNED_STATS}
    want = {k: ref[6][k] for k in PINNED_STATS}
    assert got == want


def assert_search_equals(view, dev, queries, k, ef):
    """dev.search against the CPU restatement of the search on `view`: ids, distance bits, counters."""
    ids, dists, cnt = dev.search(queries, k, ef)
    for i, q in enumerate(queries):
        r_ids, r_d, r_c = view.search(q, k, ef, with_counters=True)
        assert np.array_equal(ids[i], r_ids), (i, ids[i], r_ids)
        assert np.array_equal(dists[i].view(np.uint32), r_d.view(np.uint32)), (i, dists[i], r_d)
        assert tuple(cnt[i]) == tuple(r_c), (i, cnt[i], r_c)
