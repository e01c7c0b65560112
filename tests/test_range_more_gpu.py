"""The radius-mode range search on the device (range_more_search_kernel, range_sort_kernel) against its
restatement (tests/range_more_common.py): counts, ids, distance bits, the empty tail, the four counters and
(frontier, more_dist) equal for every query, none left out.  test_range_more_host.py pins that these inputs
reach the continuation's paths.

Each case is 2000 rows and at most 12 queries, except the ALAYA_FILTER_GRID case, whose queries are the 2000
base rows so that two waves run a thousand queries each, resetting the counts and the frontier in between.
Radii are exact m-th nearest distances over all rows, so they do not depend on what a traversal finds."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import range_common as rc
import range_more_common as rm

pytestmark = pytest.mark.gpu

FLT_MAX = fc.FLT_MAX
ONES = np.ones(fc.N, bool)
_devices = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("ALAYA_FILTER_GRID", "ALAYA_SEARCH_WAVES", "ALAYA_VIS_LIMIT", "ALAYA_VIS_LIMIT_PCT", "ALAYA_RANGE_SORT"):
        monkeypatch.delenv(name, raising=False)


def _words(allow, n=fc.N):
    from alayalite_amd.utils import pack_allow

    return pack_allow(allow, n)


def _device(native, orc, dim, metric, kind="gist"):
    key = (dim, metric, kind)
    if key not in _devices:
        base, _, arrays = fc.graph(orc, dim, metric, kind)
        _devices[key] = dc.device_of(native, base, arrays, metric)
    return _devices[key]


def _check(native, orc, dim, metric, ef, radii, cap=4096, front=4096, kind="gist", what=""):
    """One launch of a filter_common input against its cached replays; returns (device answer, replays)."""
    queries = fc.graph(orc, dim, metric, kind)[1]
    radii = np.ascontiguousarray(rc.radii_of(queries, radii))
    rs = rm.replays(orc, dim, metric, kind, ef, radii, front)
    got = _device(native, orc, dim, metric, kind).range_search_radius(queries, ef, radii, cap, front)
    rm.assert_matches(got, rs, radii, cap, (what, dim, metric, ef, cap, front))
    return got, rs


@pytest.mark.parametrize("dim,metric", [(64, 0), (64, 1), (100, 0), (128, 1), (960, 0)])
def test_main_grid(native, orc, dim, metric):
    _, queries, arrays, _, all_d = rm.case(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    grew = 0
    for m in (1, 17, 65, 200, 400):
        radii = rm.mth_exact(all_d, m)
        got, rs = _check(native, orc, dim, metric, 40, radii, what=("m", m))
        fixed = dev.range_search(queries, 40, radii, 4096)
        assert np.array_equal(got[3], fixed[3]) and (got[0] >= fixed[0]).all()  # phase 1's counters; no hit is lost
        assert (got[0] <= 4096).all() and (got[4][:, 0] <= 4096).all()  # nothing cut: the set is closed
        for i in range(len(queries)):
            ids = got[1][i][:int(got[0][i])]
            assert set(fixed[1][i][:int(fixed[0][i])].tolist()) <= set(ids.tolist()), (dim, metric, m, i)
            assert rm.closed(arrays[0], ids, all_d[i] <= radii[i]), (dim, metric, m, i)
        grew += int((got[0] > fixed[0]).sum())
    assert grew > 0
    # a radius below every distance: phase 2 is empty and the call is the fixed one
    below = np.nextafter(rm.mth_exact(all_d, 1), np.float32(-np.inf))
    got, _ = _check(native, orc, dim, metric, 40, below, 64, what="below")
    fixed = dev.range_search(queries, 40, below, 64)
    assert not got[0].any() and not got[4].any()
    for a, b in zip(got[:4], fixed):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # one radius, broadcast
    scalar = float(np.median(rm.mth_exact(all_d, 65)))
    _check(native, orc, dim, metric, 40, scalar, what="scalar")
    got = dev.range_search_radius(queries, 40, scalar, 4096, 4096)
    same = dev.range_search_radius(queries, 40, np.full(len(queries), scalar, np.float32), 4096, 4096)
    for a, b in zip(got, same):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("ef", [1, 10])
def test_small_ef(native, orc, ef):
    all_d = rm.case(orc, 64, 0)[4]
    for m in (17, 200):
        _check(native, orc, 64, 0, ef, rm.mth_exact(all_d, m), what=("ef", ef, m))


@pytest.mark.parametrize("cap", [1, 2, 64, 65, 4096])
def test_result_caps(native, orc, cap):
    radii = rm.mth_exact(rm.case(orc, 64, 0)[4], 200)
    got, _ = _check(native, orc, 64, 0, 40, radii, cap)
    assert (got[0] > cap).all() or cap == 4096  # the list is cut; the continuation is not
    assert np.array_equal(got[4], _check(native, orc, 64, 0, 40, radii)[0][4])


@pytest.mark.parametrize("front", [1, 8, 63, 64, 65])
def test_frontier_caps(native, orc, front):
    """The cut lands inside a 64-lane append and on its edge; rows past it are counted and returned, not expanded."""
    radii = rm.mth_exact(rm.case(orc, 64, 0)[4], 200)
    got, rs = _check(native, orc, 64, 0, 40, radii, 4096, front)
    assert (got[4][:, 0] > front).all() and all(len(r["front"]) == front for r in rs)
    uncut = _check(native, orc, 64, 0, 40, radii)[0]
    assert (got[0] <= uncut[0]).all() and (got[0] < uncut[0]).any()


@pytest.mark.parametrize("dim", [16, 128])
def test_tie_rows(native, orc, dim):
    all_d = rm.case(orc, dim, 0, "tie")[4]
    for m in (40, 150):
        radii = rm.mth_exact(all_d, m)
        assert min(int((all_d[i] == radii[i]).sum()) for i in range(len(radii))) >= 2
        got, _ = _check(native, orc, dim, 0, 20, radii, kind="tie", what=("tie", m))
        for i in range(len(radii)):  # inside a tie the ids ascend
            n = int(got[0][i])
            d, v = got[2][i][:n], got[1][i][:n].astype(np.int64)
            assert ((np.diff(d) > 0) | ((np.diff(d) == 0) & (np.diff(v) > 0))).all(), (dim, m, i)


def test_all_zero_ip_query(native, orc):
    """Every distance is -0.0, so radius 0.0 floods everything the graph reaches from the entry."""
    base, _, arrays = fc.graph(orc, 64, 1)
    view = dc.view_of(orc, base, arrays, 1)
    q = np.zeros((1, 64), np.float32)
    r = rm.replay(orc, view, q[0], 40, 0.0, 4096, ONES, 1)
    assert r["frontier"] == len(r["pairs"]) > 544 and r["more_dist"] > 0
    got = _device(native, orc, 64, 1).range_search_radius(q, 40, 0.0, 4096, 4096)
    assert int(got[0][0]) == r["frontier"]
    assert (got[2][0][:int(got[0][0])].view(np.uint32) == 0x80000000).all()
    rm.assert_matches(got, [r], 0.0, 4096, "zero")
    none = _device(native, orc, 64, 1).range_search_radius(q, 40, -1e-30, 4096, 4096)
    assert int(none[0][0]) == 0 and not none[4].any()


@pytest.mark.parametrize("dim,metric", [(64, 0), (128, 1), (960, 0)])
def test_masks_with_groups(native, orc, dim, metric):
    """Shares 0.1 and 0.02 in one batch: a disallowed in-radius row is no hit but is continued through."""
    _, queries, _, _, all_d = rm.case(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    shares = (0.1, 0.02)
    groups = (np.arange(len(queries)) % 2).astype(np.uint32)
    words = _words(np.stack([fc.mask(fc.N, s) for s in shares]))
    radii = rm.mth_exact(all_d, 200)
    rs = [rm.replays(orc, dim, metric, "gist", 40, radii, 4096, shares[g])[i] for i, g in enumerate(groups)]
    got = dev.range_search_radius(queries, 40, radii, 4096, 4096, words, groups)
    rm.assert_matches(got, rs, radii, 4096, ("masks", dim, metric))
    assert (got[4][:, 0] > got[0]).all()
    plain = dev.range_search_radius(queries, 40, radii, 4096, 4096)
    assert np.array_equal(got[4], plain[4]) and np.array_equal(got[3], plain[3])
    for cap, front in ((7, 4096), (4096, 8)):
        rs = [rm.replays(orc, dim, metric, "gist", 40, radii, front, shares[g])[i] for i, g in enumerate(groups)]
        rm.assert_matches(dev.range_search_radius(queries, 40, radii, cap, front, words, groups), rs, radii, cap,
                          ("masks", dim, metric, cap, front))


def _index(metric="l2", **kw):
    import alayalite_amd

    _index.count = getattr(_index, "count", 0) + 1
    return alayalite_amd.Client().create_index(f"range_more{_index.count}", metric=metric, capacity=fc.N + 64, **kw)


def _view_of_index(orc, idx, rows, metric, **kw):
    l0, levels, off, ue, ep, ur, _ = idx.native().graph_arrays()
    return orc.IndexView(rows, l0, levels, off, ue, ur, ep, metric=metric, **kw)


def _assert_csr(got, more, rs, radius, cap, id_type, what):
    """Index.range_search's (lims, ids, dists, counts) and last_range_more() against the restatement."""
    lims, ids, dists, counts = got
    assert lims.dtype == np.int64 and lims.shape == (len(rs) + 1,) and lims[0] == 0
    assert ids.dtype == id_type and dists.dtype == np.float32 and counts.dtype == np.uint32
    assert ids.shape == dists.shape == (int(lims[-1]),)
    assert more.dtype == np.uint32 and more.shape == (len(rs), 2)
    for i, (r, rad) in enumerate(zip(rs, rc.radii_of(rs, radius))):
        n, w_ids, w_d = rc.want_row(r, rad, cap)
        kept = min(n, cap)
        assert int(counts[i]) == n and int(lims[i + 1] - lims[i]) == kept, (what, i, counts[i], n, lims[i:i + 2])
        assert np.array_equal(ids[lims[i]:lims[i + 1]].astype(np.uint32), w_ids[:kept]), (what, i)
        assert np.array_equal(dists[lims[i]:lims[i + 1]].view(np.uint32), w_d[:kept].view(np.uint32)), (what, i)
        assert (int(more[i][0]), int(more[i][1])) == (r["frontier"], r["more_dist"]), (what, i, more[i])


def test_removed_rows_never_join(native, orc):
    base, queries = dc.rows(64)
    idx = _index()
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    view = _view_of_index(orc, idx, base, 0)
    all_d = rm.dists_of(orc, (64, 0, "gist"), base, queries, 0)
    radii = rm.mth_exact(all_d, 200)
    lims, first, _, _ = idx.range_search(queries.copy(), radii, 40, 4096, expand="radius")
    removed = sorted({int(v) for i in range(len(queries)) for v in first[lims[i]:lims[i] + 3]})
    assert len(removed) >= 12
    for v in removed:
        idx.remove(v)
    valid = np.full((fc.N + 7) // 8, 0xFF, np.uint8)
    for v in removed:
        valid[v >> 3] &= ~np.uint8(1 << (v & 7))
    view = _view_of_index(orc, idx, base, 0, valid=valid)
    for radius, cap, front in ((radii, 4096, 4096), (radii, 50, 4096), (float(FLT_MAX), 4096, 4096), (radii, 4096, 20)):
        rs = [rm.replay(orc, view, q, 40, rc.radii_of(queries, radius)[i], front, ONES, 0, row_d=all_d[i])
              for i, q in enumerate(queries)]
        assert not any(set(removed) & set(r["front"]) for r in rs)
        got = idx.range_search(queries.copy(), radius, 40, cap, expand="radius", max_frontier=front)
        assert not np.isin(got[1], removed).any()
        _assert_csr(got, idx.native().last_range_more(), rs, radius, cap, np.uint32, ("removed", cap, front))
        assert np.array_equal(idx.native().last_counters(), np.array([r["counters"] for r in rs], np.uint32))


def test_entry_points_without_overlay(native, orc):
    """A graph without overlay: a repeated entry point is offered, and joins the frontier, twice."""
    base, queries, arrays, _, all_d = rm.case(orc, 64, 0)
    l0 = arrays[0]
    eps = np.array([5, 77, 5, 901], np.uint32)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0, None)
    dev.set_graph(native.Graph.from_arrays(l0, None, None, None, 0, 0, eps))
    view = orc.IndexView(base, l0, None, None, None, 0, 0)
    for radius, cap, front in ((float(FLT_MAX), 4096, 4096), (float(FLT_MAX), 3, 3), (rm.mth_exact(all_d, 200), 4096, 4096)):
        radii = rc.radii_of(queries, radius)
        rs = [rm.replay(orc, view, q, 40, radii[i], front, ONES, 0, eps, all_d[i]) for i, q in enumerate(queries)]
        got = dev.range_search_radius(queries, 40, radius, cap, front)
        rm.assert_matches(got, rs, radius, cap, ("eps", cap, front))
    twice = dev.range_search_radius(queries, 40, float(FLT_MAX), 4096, 4096)
    assert all(list(row).count(5) == 2 for row in twice[1])
    assert np.array_equal(twice[0], twice[4][:, 0])  # no mask, nothing removed: every frontier row is a hit


@pytest.mark.parametrize("deg", ["dense", "dup"])
def test_wide_rows_and_repeated_edges(native, orc, deg):
    """R = 64: up to 64 rows join in one append, and the repeated ids of a row are dropped in phase 2 as well."""
    base, queries, arrays = dc.dense(native, 128) if deg == "dense" else dc.duplicated(native, 128)
    dev = dc.device_of(native, base, arrays)
    view = dc.view_of(orc, base, arrays)
    all_d = rm.dists_of(orc, (128, 0, "r64"), base, queries, 0)
    for m, cap, front in ((200, 4096, 4096), (400, 65, 4096), (400, 4096, 65), (400, 4096, 100)):
        radii = rm.mth_exact(all_d, m)
        rs = [rm.replay(orc, view, q, 40, radii[i], front, ONES, 0, row_d=all_d[i]) for i, q in enumerate(queries)]
        assert all(r["more_dist"] > 0 for r in rs)
        rm.assert_matches(dev.range_search_radius(queries, 40, radii, cap, front), rs, radii, cap, (deg, m, cap, front))


@pytest.mark.parametrize("dim", [64, 960])
def test_forced_spill(native, orc, dim):
    base, queries, arrays, _, all_d = rm.case(orc, dim, 0)
    dev = dc.device_of(native, base, arrays)
    dev.set_hash_log2(8)
    for m in (65, 400):
        radii = rm.mth_exact(all_d, m)
        rs = rm.replays(orc, dim, 0, "gist", 40, radii)
        assert min(r["visited"] for r in rs) > 256
        got = dev.range_search_radius(queries, 40, radii, 4096, 4096)
        assert dev.last_plan()["hash_log2"] == 8
        rm.assert_matches(got, rs, radii, 4096, ("spill", dim, m))


def _reachable(l0, start):
    """Rows reachable from `start` along level-0 edges: a numpy breadth-first walk."""
    seen = np.zeros(len(l0), bool)
    seen[start] = True
    edge = np.array([start])
    while len(edge):
        nb = l0[edge].ravel()
        nb = np.unique(nb[nb != fc.EMPTY].astype(np.int64))
        edge = nb[~seen[nb]]
        seen[edge] = True
    return seen


@pytest.mark.parametrize("dim,metric", [(64, 0), (960, 0)])
def test_radius_flt_max_floods_the_graph(native, orc, dim, metric):
    _, queries, arrays, _, _ = rm.case(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    got, rs = _check(native, orc, dim, metric, 40, float(FLT_MAX), what="flood")
    for i, r in enumerate(rs):
        n = int(_reachable(arrays[0], r["pairs"][0][0]).sum())
        assert int(got[0][i]) == n == int(got[4][i][0]), (dim, i, got[0][i], n)
        assert len(set(got[1][i][:n].tolist())) == n
    # the first-level visited table is smaller than what the flood fill visits: it has spilled
    assert (1 << dev.last_plan()["hash_log2"]) * 11 // 16 < min(r["visited"] for r in rs)


def test_two_workgroups_run_the_whole_batch(native, orc, monkeypatch):
    base, queries, arrays, view, all_d = rm.case(orc, 64, 0)
    dev = _device(native, orc, 64, 0)
    radius = np.float32(np.median(rm.mth_exact(all_d, 25)))
    rs = [rm.replay(orc, view, q, 16, radius, 16, ONES, 0) for q in base]
    assert any(r["frontier"] > 16 for r in rs) and any(0 < r["frontier"] <= 16 for r in rs)
    assert any(r["more_dist"] == 0 for r in rs) and any(r["more_dist"] > 0 for r in rs)
    monkeypatch.setenv("ALAYA_FILTER_GRID", "2")
    got = dev.range_search_radius(base, 16, float(radius), 24, 16)
    groups, waves = dev.last_launch()
    assert groups == 2 and groups * waves * 100 <= len(base), (groups, waves)
    assert (got[0] > 24).any() and (got[0] <= 24).any()
    rm.assert_matches(got, rs, float(radius), 24, "grid 2")


def test_index_cos_uint64_and_chunks(native, orc):
    """Index.range_search(expand="radius"): COS queries normalised as batch_search does, ids in the index's id
    type, and a chunked call equal to the whole one, last_range_more() included."""
    base, queries = dc.rows(64)
    rows = base.copy()
    idx = _index("cosine", id_type=np.uint64)
    idx.fit(rows, ef_construction=100, num_threads=1)  # normalises rows in place
    view = _view_of_index(orc, idx, rows, 2)
    nq = [orc.normalize(q) for q in queries]
    all_d = np.array([[orc.dist(2, q, b) for b in rows] for q in nq], np.float32)
    radii = rm.mth_exact(all_d, 200)
    assert (radii < 0).all()
    for cap, front in ((4096, 4096), (64, 4096), (4096, 33)):
        rs = [rm.replay(orc, view, q, 40, radii[i], front, ONES, 2, row_d=all_d[i]) for i, q in enumerate(nq)]
        got = idx.range_search(queries.copy(), radii, 40, cap, expand="radius", max_frontier=front)
        more = idx.native().last_range_more()
        _assert_csr(got, more, rs, radii, cap, np.uint64, ("cos", cap, front))
        chunked = idx.range_search(queries.copy(), radii, 40, cap, _chunk=5, expand="radius", max_frontier=front)
        for a, b in zip(got, chunked):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        assert np.array_equal(idx.native().last_range_more(), more)
    allow = fc.mask(fc.N, 0.1)
    rs_m = [rm.replay(orc, view, q, 40, radii[i], 4096, allow, 2, row_d=all_d[i]) for i, q in enumerate(nq)]
    got = idx.range_search(queries.copy(), radii, 40, 4096, allow=allow, expand="radius")
    _assert_csr(got, idx.native().last_range_more(), rs_m, radii, 4096, np.uint64, "cos mask")
    empty = idx.range_search(queries[:0].copy(), 1.0, 40, 8, expand="radius")
    assert empty[0].tolist() == [0] and empty[1].dtype == np.uint64 and empty[1].size == 0


def test_fixed_is_the_call_without_the_keyword(native, orc):
    base, queries = dc.rows(64)
    idx = _index()
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    radii = rm.mth_exact(rm.dists_of(orc, (64, 0, "gist"), base, queries, 0), 200)
    plain = idx.range_search(queries.copy(), radii, 40, 64)
    fixed = idx.range_search(queries.copy(), radii, 40, 64, expand="fixed", max_frontier=7)
    for a, b in zip(plain, fixed):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    more = idx.range_search(queries.copy(), radii, 40, 64, expand="radius")
    assert (more[3] >= plain[3]).all() and (more[3] > plain[3]).any()


def test_refusals(native, orc):
    base, queries, arrays = fc.graph(orc, 64, 0)
    dev = _device(native, orc, 64, 0)
    for front in (0, 16385):
        with pytest.raises(ValueError, match="1..16384"):
            dev.range_search_radius(queries, 40, 1.0, 64, front)
    dev.range_search_radius(queries, 40, 1.0, 64, 16384)
    with pytest.raises(ValueError, match="1..4096"):
        dev.range_search_radius(queries, 40, 1.0, 4097, 64)
    with pytest.raises(ValueError, match="ef"):
        dev.range_search_radius(queries, 0, 1.0, 64, 64)
    with pytest.raises(ValueError, match="NaN"):
        dev.range_search_radius(queries, 40, float("nan"), 64, 64)
    with pytest.raises(ValueError):
        dev.range_search_radius(queries, 40, 1.0, 64, 64, None, np.zeros(len(queries), np.uint32))  # indices without masks
    sq = dc.device_of(native, base, arrays)
    mn, mx = native.sq8_train(base)
    sq.set_sq8(native.sq8_encode(base, mn, mx, 1), mn, mx, native.host_sq8_order())
    with pytest.raises(ValueError, match="SQ8"):
        sq.range_search_radius(queries, 40, 1.0, 64, 64)
    idx = _index(quantization_type="sq8")
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    with pytest.raises(ValueError, match="SQ8"):
        idx.range_search(queries.copy(), 1.0, 40, 64, expand="radius")
    plain = _index()
    plain.fit(base.copy(), ef_construction=100, num_threads=1)
    for bad in (dict(max_frontier=0), dict(max_frontier=16385), dict(expand="through"), dict(expand="radius", max_results=0)):
        with pytest.raises(ValueError):
            plain.range_search(queries.copy(), 1.0, 40, **bad)


def test_device_entry(native, orc):
    """Results on torch device tensors, on a stream of the caller's, equal the host entry's."""
    import torch

    _, queries, _, _, all_d = rm.case(orc, 64, 0)
    dev = _device(native, orc, 64, 0)
    radii = rm.mth_exact(all_d, 200)
    cap, front, nq = 33, 150, len(queries)
    groups = np.zeros(nq, np.uint32)
    words = _words(fc.mask(fc.N, 0.1))
    host = dev.range_search_radius(queries, 40, radii, cap, front, words, groups)
    rm.assert_matches(host, rm.replays(orc, 64, 0, "gist", 40, radii, front, 0.1), radii, cap, "host")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_q = torch.from_numpy(queries.copy()).cuda()
        t_r = torch.from_numpy(radii).cuda()
        t_w = torch.from_numpy(words.view(np.int32)).cuda()
        t_g = torch.from_numpy(groups.view(np.int32)).cuda()
        t_counts = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
        t_ids = torch.full((nq, cap), -2, dtype=torch.int32, device="cuda")
        t_d = torch.zeros((nq, cap), dtype=torch.float32, device="cuda")
        t_c = torch.zeros((nq, 4), dtype=torch.int32, device="cuda")
        t_m = torch.full((nq, 2), -3, dtype=torch.int32, device="cuda")
        dev.range_search_radius_device(t_q.data_ptr(), nq, 40, t_r.data_ptr(), cap, t_w.data_ptr(), 1, t_g.data_ptr(),
                                       t_counts.data_ptr(), t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(),
                                       stream.cuda_stream, front, t_m.data_ptr())
        # no mask, no counters and no `more` through the device entry, on the same stream
        n_counts = torch.zeros((nq,), dtype=torch.int32, device="cuda")
        n_ids = torch.zeros((nq, cap), dtype=torch.int32, device="cuda")
        n_d = torch.zeros((nq, cap), dtype=torch.float32, device="cuda")
        dev.range_search_radius_device(t_q.data_ptr(), nq, 40, t_r.data_ptr(), cap, 0, 0, 0, n_counts.data_ptr(),
                                       n_ids.data_ptr(), n_d.data_ptr(), 0, stream.cuda_stream, front, 0)
    stream.synchronize()
    got = (t_counts.cpu().numpy().view(np.uint32), t_ids.cpu().numpy().view(np.uint32), t_d.cpu().numpy(),
           t_c.cpu().numpy().view(np.uint32), t_m.cpu().numpy().view(np.uint32))
    for a, b in zip(got, host):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    plain = dev.range_search_radius(queries, 40, radii, cap, front)
    assert np.array_equal(n_counts.cpu().numpy().view(np.uint32), plain[0])
    assert np.array_equal(n_ids.cpu().numpy().view(np.uint32), plain[1])
    assert np.array_equal(n_d.cpu().numpy().view(np.uint32), plain[2].view(np.uint32))
    with pytest.raises(ValueError, match="1..16384"):
        dev.range_search_radius_device(t_q.data_ptr(), nq, 40, t_r.data_ptr(), cap, 0, 0, 0, n_counts.data_ptr(),
                                       n_ids.data_ptr(), n_d.data_ptr(), 0, stream.cuda_stream, 0, 0)
