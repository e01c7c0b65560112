"""The radius-mode range search's restatement (tests/range_more_common.py) and the inputs of
test_range_more_gpu.py, without a GPU.

What is pinned here is that the inputs reach the new paths: that the continuation finds rows the fixed
traversal missed (and at a small radius finds nothing to do), that a small frontier cap cuts it, that under
a mask the frontier runs through disallowed rows, that removed rows stay out, and that the restatement's
answer is closed under the level-0 adjacency."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import range_common as rc
import range_more_common as rm


def _counts(rs, radii, phase1=False):
    key = "pairs1" if phase1 else "pairs"
    return [len(rc.hits(dict(pairs=r[key]), rad)) for r, rad in zip(rs, radii)]


@pytest.mark.parametrize("dim,metric", [(64, 0), (128, 1), (960, 0)])
def test_continuation_adds_hits(orc, dim, metric):
    all_d = rm.case(orc, dim, metric)[4]
    for m in (65, 200, 400):
        radii = rm.mth_exact(all_d, m)
        rs = rm.replays(orc, dim, metric, "gist", 40, radii)
        both, first = _counts(rs, radii), _counts(rs, radii, True)
        print(dim, metric, m, "hits phase 1:", sum(first), "both:", sum(both), "more_dist:",
              min(r["more_dist"] for r in rs), "to", max(r["more_dist"] for r in rs))
        assert all(b >= a for a, b in zip(first, both)) and sum(both) > sum(first), (dim, metric, m, first, both)
        assert all(r["more_dist"] > 0 for r in rs), (dim, metric, m)
        assert all(r["frontier"] <= 4096 for r in rs)  # not cut: the GPU cases' F = 4096 holds every frontier
        assert all(r["pairs"][:len(r["pairs1"])] == r["pairs1"] for r in rs)


def test_small_radius_finds_nothing_to_do(orc):
    radii = rm.mth_exact(rm.case(orc, 64, 0)[4], 17)
    rs = rm.replays(orc, 64, 0, "gist", 40, radii)
    assert any(r["more_dist"] == 0 for r in rs), [r["more_dist"] for r in rs]
    for r in rs:
        if r["more_dist"] == 0:
            assert r["pairs"] == r["pairs1"] and r["frontier"] > 0


def test_small_ef_is_made_up_for(orc):
    radii = rm.mth_exact(rm.case(orc, 64, 0)[4], 200)
    rs = rm.replays(orc, 64, 0, "gist", 10, radii)
    both, first = sum(_counts(rs, radii)), sum(_counts(rs, radii, True))
    print("ef 10, m 200: hits", first, "->", both)
    assert both > 2 * first


def test_frontier_cap_cuts_the_continuation(orc):
    radii = rm.mth_exact(rm.case(orc, 64, 0)[4], 200)
    uncut = rm.replays(orc, 64, 0, "gist", 40, radii)
    cut = rm.replays(orc, 64, 0, "gist", 40, radii, 8)
    differs = 0
    for r, u, rad in zip(cut, uncut, radii):
        assert r["frontier"] > 8 and len(r["front"]) == 8 and r["front"] == u["front"][:8]
        h, hu, h1 = rc.hits(r, rad), rc.hits(u, rad), rc.hits(dict(pairs=r["pairs1"]), rad)
        assert r["pairs1"] == u["pairs1"] and len(h1) <= len(h) <= len(hu)
        differs += h != hu and h != h1
    assert differs > 0


def test_masked_frontier_runs_through_disallowed_rows(orc):
    radii = rm.mth_exact(rm.case(orc, 64, 0)[4], 200)
    rs = rm.replays(orc, 64, 0, "gist", 40, radii, share=0.1)
    allow = fc.mask(fc.N, 0.1)
    for r, rad in zip(rs, radii):
        assert r["frontier"] > len(rc.hits(r, rad)) > 0
        assert not all(allow[v] for v in r["front"]) and all(allow[v] for v, _ in r["pairs"])
    # the frontier itself is the unmasked one: the mask only selects the hits
    plain = rm.replays(orc, 64, 0, "gist", 40, radii)
    assert [r["front"] for r in rs] == [r["front"] for r in plain]
    assert [r["more_dist"] for r in rs] == [r["more_dist"] for r in plain]


def test_removed_rows_stay_out_of_the_frontier(orc):
    base, queries, arrays, view, all_d = rm.case(orc, 64, 0)
    radii = rm.mth_exact(all_d, 200)
    plain = rm.replays(orc, 64, 0, "gist", 40, radii)
    removed = sorted({v for r in plain for v in r["front"][:3]})
    valid = np.full((fc.N + 7) // 8, 0xFF, np.uint8)
    for v in removed:
        valid[v >> 3] &= ~np.uint8(1 << (v & 7))
    cut_view = dc.view_of(orc, base, arrays, 0, valid=valid)
    for i, q in enumerate(queries):
        r = rm.replay(orc, cut_view, q, 40, radii[i], 4096, np.ones(fc.N, bool), 0, row_d=all_d[i])
        assert not set(removed) & set(r["front"]) and not set(removed) & {v for v, _ in r["pairs"]}
        assert r["frontier"] > 0


@pytest.mark.parametrize("dim,metric", [(64, 0), (128, 1)])
def test_restatement_is_closed(orc, dim, metric):
    _, _, arrays, _, all_d = rm.case(orc, dim, metric)
    for m in (65, 400):
        radii = rm.mth_exact(all_d, m)
        for i, r in enumerate(rm.replays(orc, dim, metric, "gist", 40, radii)):
            ids = [v for v, _ in rc.hits(r, radii[i])]
            assert r["frontier"] <= 4096 and sorted(ids) == sorted(r["front"])
            assert rm.closed(arrays[0], ids, all_d[i] <= radii[i]), (dim, metric, m, i)
            first = [v for v, _ in rc.hits(dict(pairs=r["pairs1"]), radii[i])]
            assert set(first) <= set(ids)
    # and the walk itself notices an open set: drop a row that another returned row points to
    radius = rm.mth_exact(all_d, 400)[0]
    r = rm.replays(orc, dim, metric, "gist", 40, rm.mth_exact(all_d, 400))[0]
    ids = [v for v, _ in rc.hits(r, radius)]
    pointed = next(int(v) for u in ids for v in arrays[0][u] if v != fc.EMPTY and int(v) in set(ids) and int(v) != u)
    assert not rm.closed(arrays[0], [v for v in ids if v != pointed], all_d[0] <= radius)
