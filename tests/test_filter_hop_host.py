"""The through search's restatement (tests/filter_hop_common.py) and the inputs of test_filter_hop_gpu.py,
without a GPU.

The restatement is what the device must equal, so it is pinned first: with an all-ones mask it is
filter_common.replay (so the oracle's own search) and steps through nothing; every id it returns is
passable, its traversal pool holds passable rows only beside the entry, and its answer is the first k of
the offered pairs under a stable sort by distance.  Then what the traversal is for -- recall at a share of
0.1 and ef 16 far above the plain filtered traversal's -- and the conditions that keep the GPU cases from
being vacuous: a pop whose through rows yield more than 64 candidates, a pop without through rows under a
partial mask, a row two through rows of one pop offer, and a through row that repeats an id."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import filter_hop_common as hc


@pytest.mark.parametrize("dim,metric,kind,k,ef", [(64, 0, "gist", 10, 40), (128, 1, "gist", 10, 40), (64, 0, "gist", 65, 10),
                                                  (960, 0, "gist", 224, 64), (16, 0, "tie", 10, 20)])
def test_all_ones_mask_is_the_filtered_search(orc, dim, metric, kind, k, ef):
    plain = fc.replays(orc, dim, metric, kind, k, ef, 1.0)
    for i, r in enumerate(hc.replays(orc, dim, metric, kind, k, ef, 1.0)):
        assert np.array_equal(r["ids"], plain[i]["ids"]), (i, r["ids"], plain[i]["ids"])
        assert np.array_equal(r["dists"].view(np.uint32), plain[i]["dists"].view(np.uint32)), i
        assert tuple(r["counters"][:4]) == tuple(plain[i]["counters"]), (i, r["counters"], plain[i]["counters"])
        assert r["counters"][4] == 0
        assert r["pool"] == plain[i]["pool"]


CASES = [(64, 0, "gist", 10, 16, 0.1), (128, 1, "gist", 10, 64, 0.02), (960, 0, "gist", 1, 8, 0.5),
         (16, 0, "gist", 32, 16, 0.2), (16, 0, "tie", 10, 20, 0.3), (128, 0, "tie", 10, 20, 0.3)]


@pytest.mark.parametrize("dim,metric,kind,k,ef,share", CASES)
def test_basic_invariants(orc, dim, metric, kind, k, ef, share):
    allow = fc.mask(fc.N, share)
    for i, r in enumerate(hc.replays(orc, dim, metric, kind, k, ef, share)):
        assert all(allow[v] for v in r["ids"] if v != fc.EMPTY), i
        assert all(allow[v] or v in r["entries"] for v, _ in r["pool"]), i
        assert all(allow[v] for v, _ in r["pairs"]), i
        ids, d = fc.stable_first_k(r["pairs"], k)
        assert np.array_equal(r["ids"], ids), (i, r["ids"], ids)
        assert np.array_equal(r["dists"].view(np.uint32), d.view(np.uint32)), i


def test_all_zero_mask_ends_after_the_entry(orc):
    for r in hc.replays(orc, 64, 0, "gist", 10, 40, 0.0):
        assert (r["ids"] == fc.EMPTY).all() and (r["dists"] == fc.FLT_MAX).all()
        assert r["counters"][0] == 0 and r["counters"][1] == 1 and r["counters"][4] > 0
        assert [v for v, _ in r["pool"]] == r["entries"] and not r["pairs"]


def test_recall_at_a_share_of_a_tenth(orc):
    """gist_like(2000, 12, 64, 5 centres), build_hnsw(.., 32, 100), k 10, ef 16, share 0.1, against the float64
    top-10 over base[allowed]: the through recall is at least 0.95 and at least 0.2 above the plain filtered
    traversal's (the issue's CPU prototype: 1.000 against 0.692)."""
    base, queries, _ = fc.graph(orc, 64, 0)
    allow = fc.mask(fc.N, 0.1)
    truth = hc.exact_allowed(base, queries, allow, 10)
    through = hc.recall(hc.replays(orc, 64, 0, "gist", 10, 16, 0.1), truth)
    plain = hc.recall(fc.replays(orc, 64, 0, "gist", 10, 16, 0.1), truth)
    print("recall@10 at share 0.1, ef 16: through", through, "plain", plain)
    assert through >= 0.95, through
    assert through >= plain + 0.2, (through, plain)


def test_removed_rows_are_stepped_through(orc):
    """With a bitmap and an all-ones mask the removed rows are the through rows; none enters the pool."""
    base, queries, arrays = fc.graph(orc, 64, 0)
    valid = np.full((fc.N + 7) // 8, 0xFF, np.uint8)
    removed = list(range(0, fc.N, 7))
    for v in removed:
        valid[v >> 3] &= ~np.uint8(1 << (v & 7))
    view = dc.view_of(orc, base, arrays, 0, valid=valid)
    ones = np.ones(fc.N, bool)
    rows = hc.replays(orc, 64, 0, "removed", 10, 16, 1.0, view=view, queries=queries, allow=ones)
    assert sum(r["counters"][4] for r in rows) > 0
    for r in rows:
        assert not np.isin(r["ids"], removed).any()
        assert all(v not in removed or v in r["entries"] for v, _ in r["pool"])


# ---- the GPU cases' inputs make the kernel's branches run ---------------------------------------------
def _total(rows, key):
    return sum(r[key] for r in rows)


def _grid_rows(orc):
    for dim, metric in hc.SHAPES:
        for k, ef, share in hc.KEFS:
            yield (dim, metric, k, ef, share), hc.replays(orc, dim, metric, "gist", k, ef, share)


def test_the_queue_flushes_mid_pop(orc):
    """Some pop's through rows yield more than 64 candidates, in the main grid at every width."""
    hit = {}
    for (dim, metric, k, ef, share), rows in _grid_rows(orc):
        hit[(dim, metric)] = hit.get((dim, metric), 0) + _total(rows, "flush_pops")
    print("pops with more than 64 through candidates:", hit)
    assert all(hit[s] >= 1 for s in hc.SHAPES), hit


def test_some_pop_has_no_through_row_under_a_partial_mask(orc):
    hit = {key: _total(rows, "empty_through") for key, rows in _grid_rows(orc) if key[4] < 1.0}
    print("pops without a through row:", hit)
    assert sum(hit.values()) >= 1, hit  # (rare at these shares: a few pops of the d = 128 IP cases)


def test_two_through_rows_of_a_pop_offer_the_same_row(orc):
    hit = {key: _total(rows, "cross_dups") for key, rows in _grid_rows(orc) if 0.0 < key[4] < 1.0}
    print("rows offered by a second through row of the same pop:", hit)
    assert all(v >= 1 for v in hit.values()), hit


def test_a_through_row_repeats_an_id_on_the_dup_graph(native, orc):
    """test_filter_hop_gpu.test_wide_rows_and_repeated_edges' inputs: on the dup graph some through row repeats
    an id that is passable and fresh; on both graphs most fresh neighbours are through rows and some pop's
    through rows overflow the queue."""
    for deg in ("dense", "dup"):
        base, queries, arrays = dc.dense(native, 128) if deg == "dense" else dc.duplicated(native, 128)
        view = dc.view_of(orc, base, arrays)
        assert hc.graph_repeats(view.l0) == (deg == "dup")
        for k, ef, share in ((10, 16, 0.1), (65, 10, 0.3)):
            allow = fc.mask(fc.N, share)
            rows = hc.replays(orc, 128, 0, deg, k, ef, share, view=view, queries=queries, allow=allow)
            n_dist, n_through = sum(r["counters"][0] for r in rows), sum(r["counters"][4] for r in rows)
            print(deg, k, ef, share, "through rows", n_through, "distances", n_dist, "flush pops", _total(rows, "flush_pops"),
                  "repeats met", _total(rows, "dup_through"))
            assert _total(rows, "flush_pops") >= 1 and _total(rows, "cross_dups") >= 1
            if share == 0.1:  # most fresh neighbours are through rows: more of them than rows measured
                assert n_through > n_dist, (deg, n_through, n_dist)
            if deg == "dup":
                assert _total(rows, "dup_through") >= 1
