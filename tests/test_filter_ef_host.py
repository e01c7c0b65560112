"""The filtered searches' restatements at ef above 64 and the inputs of test_filter_ef_gpu.py, without a GPU.

The restatements are what the device must equal, so they are pinned first in the new range: with an all-ones
mask filter_common.replays is the oracle's own search (ids, distance bits, counters) at ef 129 and 387 and
d = 256, 512, 1024, and filter_hop_common.replays is filter_common.replays.  Then, for every tuple the GPU file
runs (tests/filter_ef_common.py), the conditions that keep it from being vacuous: the final traversal pool
holds exactly ef entries and n_dist >= 2 ef for every query -- the pool filled and went on rejecting and
shifting -- the through cases stepped through some row, and at ef 387 some insertion into a full pool lands
more than 128 entries below its end, which the kernels' shift loop covers in three 64-entry trips.

Two groups of GPU cases have conditions of their own, stated at their tests: ef at and above the row count (the
pool never fills: every reachable row is measured) and the queries that run several to a wave (the through
pool of a share-0.02 mask holds the few allowed rows only)."""

import bisect

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import filter_ef_common as ec
import filter_hop_common as hc
import filter_sq8_common as sc

PINNED = [(256, 0), (512, 1), (1024, 0)]
PINNED_EFS = [129, 387]


@pytest.mark.parametrize("ef", PINNED_EFS)
@pytest.mark.parametrize("dim,metric", PINNED)
def test_all_ones_mask_is_the_plain_search(orc, dim, metric, ef):
    base, queries, arrays = fc.graph(orc, dim, metric)
    view = dc.view_of(orc, base, arrays, metric)
    for i, r in enumerate(fc.replays(orc, dim, metric, "gist", 10, ef, 1.0)):
        ids, d, cnt = view.search(queries[i], 10, ef, with_counters=True)
        assert np.array_equal(r["ids"], ids), (i, r["ids"], ids)
        assert np.array_equal(r["dists"].view(np.uint32), d.view(np.uint32)), i
        assert tuple(r["counters"]) == tuple(cnt), (i, r["counters"], cnt)


@pytest.mark.parametrize("ef", PINNED_EFS)
@pytest.mark.parametrize("dim,metric", PINNED)
def test_all_ones_mask_through_is_the_filtered_search(orc, dim, metric, ef):
    want = fc.replays(orc, dim, metric, "gist", 10, ef, 1.0)
    for i, r in enumerate(hc.replays(orc, dim, metric, "gist", 10, ef, 1.0)):
        assert np.array_equal(r["ids"], want[i]["ids"]), (i, r["ids"], want[i]["ids"])
        assert np.array_equal(r["dists"].view(np.uint32), want[i]["dists"].view(np.uint32)), i
        assert tuple(r["counters"][:4]) == tuple(want[i]["counters"]) and r["counters"][4] == 0, (i, r["counters"])
        assert r["pool"] == want[i]["pool"], i


# ---- the conditions -----------------------------------------------------------------------------------
def _assert_fills(rows, ef, what, through=False):
    ratio = min(r["counters"][0] for r in rows) / ef
    print(what, "min n_dist / ef: %.2f" % ratio)
    for i, r in enumerate(rows):
        assert len(r["pool"]) == ef, (what, i, len(r["pool"]))
        assert r["counters"][0] >= 2 * ef, (what, i, r["counters"])
        if through:
            assert r["counters"][4] > 0, (what, i, r["counters"])


@pytest.mark.parametrize("case", ec.plain_cases(), ids=str)
def test_plain_cases_fill_the_pool(orc, case):
    dim, metric, kind, k, ef, share = case
    _assert_fills(fc.replays(orc, dim, metric, kind, k, ef, share), ef, case)


@pytest.mark.parametrize("case", ec.hop_cases(), ids=str)
def test_through_cases_fill_the_pool(orc, case):
    dim, metric, kind, k, ef, share = case
    # (with every row allowed -- the three-mask case's third mask -- no row is stepped through)
    _assert_fills(hc.replays(orc, dim, metric, kind, k, ef, share), ef, case, through=share < 1.0)


def test_through_second_half_mask_fills_the_pool(orc):
    """The three-mask case's second mask, on the queries that use it."""
    dim, metric, k, ef = ec.THREE
    base, queries, arrays = fc.graph(orc, dim, metric)
    view = dc.view_of(orc, base, arrays, metric)
    allow = ec.second_half_mask(fc.N)
    assert 900 <= int(allow.sum()) <= 1100 and not np.array_equal(allow, fc.mask(fc.N, 0.5))
    rows = hc.replays(orc, dim, metric, "half2", k, ef, 0.5, view=view, queries=queries[1::3], allow=allow)
    _assert_fills(rows, ef, "second half mask", through=True)


@pytest.mark.parametrize("case", ec.sq8_cases(), ids=str)
def test_sq8_cases_fill_the_pool(orc, case):
    dim, metric, order, k, ef, m, share = case
    _assert_fills(sc.replays(orc, dim, metric, "gist", order, k, ef, m, share), ef, case)


def test_several_queries_per_wave_leave_different_pools(orc):
    """Queries = base rows 0..47, ef 200, masks of shares 0.5 and 0.02 by turns.  The plain and the SQ8
    traversal pools fill whatever the mask.  The through pool holds allowed rows only: it fills at share 0.5
    and stays far below ef at share 0.02 (about 40 allowed rows), so consecutive queries of a wave leave
    pools of very different sizes behind -- what the case is for."""
    ef = ec.WAVE_EF
    _assert_fills(ec.wave_wants(orc, "plain"), ef, "wave plain")
    _assert_fills(ec.wave_wants(orc, "sq8"), ef, "wave sq8")
    rows = ec.wave_wants(orc, "through")
    _assert_fills(rows[0::2], ef, "wave through, share 0.5", through=True)
    sizes = [len(r["pool"]) for r in rows[1::2]]
    print("through pools at share 0.02:", sizes)
    assert max(sizes) <= 64 and all(r["counters"][4] > 0 for r in rows[1::2]), sizes
    # the result pools alternate as well: full at share 0.5, short of k for some query at share 0.02
    for kernel in ("plain", "through", "sq8"):
        rows = ec.wave_wants(orc, kernel)
        assert all((r["ids"] != fc.EMPTY).all() for r in rows[0::2]), kernel


@pytest.mark.parametrize("ef", ec.OVER_EFS)
def test_ef_at_the_row_count_measures_every_row(orc, ef):
    """The pool never fills, so nothing is ever rejected: the plain search measures the 1999 rows beside the
    entry and expands all 2000, and its answer is the exact filtered top k; the through search's pool holds
    the allowed rows it reached and nothing else."""
    dim, metric, k, share = ec.OVER
    allow = fc.mask(fc.N, share)
    for i, r in enumerate(fc.replays(orc, dim, metric, "gist", k, ef, share)):
        assert r["counters"][0] == fc.N - 1 and r["counters"][1] == fc.N, (i, r["counters"])
        assert len(r["pool"]) == fc.N < ef + 1
        assert sorted(v for v, _ in r["pairs"]) == [int(v) for v in np.nonzero(allow)[0]], i
    for i, r in enumerate(hc.replays(orc, dim, metric, "gist", k, ef, share)):
        assert len(r["pool"]) < ef and r["counters"][1] == len(r["pool"]) and r["counters"][4] > 0, (i, r["counters"])
        assert all(allow[v] for v, _ in r["pool"] if v not in r["entries"]), i
        assert sorted(v for v, _ in r["pairs"]) == [int(v) for v in np.nonzero(allow)[0]], i


# ---- the three-trip shift at ef 387 -----------------------------------------------------------------------
class _Recording:
    """orc.Pool that notes, per capacity, the longest span (size - position) of an insertion into a full pool."""

    spans = {}
    real = None

    def __init__(self, n, capacity):
        self._p = _Recording.real(n, capacity)
        self._cap = capacity

    def insert(self, i, d):
        size = self._p.size()
        if size == self._cap and d < self._p.dist(size - 1):
            keys = _Dists(self._p, size)
            at = bisect.bisect_right(keys, np.float32(d))
            _Recording.spans[self._cap] = max(_Recording.spans.get(self._cap, 0), size - at)
        return self._p.insert(i, d)

    def __getattr__(self, name):
        return getattr(self._p, name)


class _Dists:
    def __init__(self, pool, size):
        self._pool, self._size = pool, size

    def __len__(self):
        return self._size

    def __getitem__(self, i):
        return np.float32(self._pool.dist(i))


def _traversals_387():
    """One entry per distinct traversal pool of the ef 387 cases: the plain and the SQ8 traversal do not
    depend on the mask or on k."""
    out = {}
    for dim, metric, kind, k, ef, share in ec.plain_cases():
        if ef == 387:
            out[("plain", dim, metric)] = ("plain", dim, metric, 0, k, share)
    for dim, metric, kind, k, ef, share in ec.hop_cases():
        if ef == 387:
            out[("through", dim, metric, share)] = ("through", dim, metric, 0, k, share)
    for dim, metric, order, k, ef, m, share in ec.sq8_cases():
        if ef == 387:
            out[("sq8", dim, metric, order)] = ("sq8", dim, metric, order, k, share)
    return list(out.values())


@pytest.mark.parametrize("case", _traversals_387(), ids=str)
def test_ef_387_shifts_span_three_trips(orc, monkeypatch, case):
    """Some query inserts into the full 387-entry pool at a position more than 128 below its end.  (The
    kernel merges a batch at once and starts its shift at the batch's first position, which is at or below
    the position any member takes one by one; the full pool's size is the same either way.)"""
    kernel, dim, metric, order, k, share = case
    ef = 387
    assert k != ef
    _Recording.real = orc.Pool
    _Recording.spans = {}
    monkeypatch.setattr(orc, "Pool", _Recording)
    allow = fc.mask(fc.N, share)
    if kernel == "sq8":
        base, queries, arrays, quant = sc.inputs(orc, dim, metric)
    else:
        base, queries, arrays = fc.graph(orc, dim, metric)
    view = dc.view_of(orc, base, arrays, metric)
    for q in queries:
        if kernel == "plain":
            fc.replay(orc, view, q, k, ef, allow, metric)
        elif kernel == "through":
            hc.replay(orc, view, q, k, ef, allow, metric)
        else:
            sc.replay(orc, view, quant, order, q, 10, ef, 10, allow, metric)
        if _Recording.spans.get(ef, 0) > 128:
            break
    print(case, "longest shift span:", _Recording.spans.get(ef, 0))
    assert _Recording.spans.get(ef, 0) > 128, (case, _Recording.spans)
