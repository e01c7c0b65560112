"""The range search on the device (range_search_kernel, range_sort_kernel) against its restatement
(tests/range_common.py): counts, ids, distance bits, the empty tail and the four counters equal for
every query, none left out.  test_range_host.py pins that these inputs reach the append list's paths.

Each case is 2000 rows and at most 12 queries, except the ALAYA_FILTER_GRID case, whose queries are the
2000 base rows so that two waves run a thousand queries each, resetting count and slot base in between."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import range_common as rc

pytestmark = pytest.mark.gpu

SHAPES = [(64, 0), (64, 1), (100, 0), (128, 0), (128, 1), (960, 0)]
FLT_MAX = fc.FLT_MAX
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


def _mth(rs, m):
    return np.array([rc.mth_distance(r, m) for r in rs], np.float32)


def _run_grid(dev, queries, rs, ef, what):
    """The radii and caps of the main grid on one (device, replays) pair."""
    for m in (1, 17, 64, 65):  # 64 fills the list exactly, 65 truncates it by one (ties may add more)
        if min(len(r["pairs"]) for r in rs) < m:
            continue
        radii = _mth(rs, m)
        rc.assert_matches(dev.range_search(queries, ef, radii, 64), rs, radii, 64, (what, "m", m))
    below = np.nextafter(_mth(rs, 1), np.float32(-np.inf))
    got = dev.range_search(queries, ef, below, 64)
    assert not got[0].any() and (got[1] == fc.EMPTY).all() and (got[2] == FLT_MAX).all()
    rc.assert_matches(got, rs, below, 64, (what, "below"))
    got = dev.range_search(queries, ef, float(FLT_MAX), 4096)
    assert [int(c) for c in got[0]] == [len(r["pairs"]) for r in rs]
    rc.assert_matches(got, rs, FLT_MAX, 4096, (what, "all"))
    for cap in (1, 2, 63, 64, 65, 100):
        rc.assert_matches(dev.range_search(queries, ef, float(FLT_MAX), cap), rs, FLT_MAX, cap, (what, "cap", cap))
    scalar = float(np.median(_mth(rs, min(17, min(len(r["pairs"]) for r in rs)))))  # one radius, broadcast
    rc.assert_matches(dev.range_search(queries, ef, scalar, 64), rs, scalar, 64, (what, "scalar"))


@pytest.mark.parametrize("dim,metric", SHAPES)
def test_main_grid(native, orc, dim, metric):
    _, queries, _ = fc.graph(orc, dim, metric)
    rs = rc.replays(orc, dim, metric, "gist", 40)
    assert min(len(r["pairs"]) for r in rs) >= 65
    _run_grid(_device(native, orc, dim, metric), queries, rs, 40, (dim, metric))


@pytest.mark.parametrize("ef", [1, 10])
def test_small_ef(native, orc, ef):
    _, queries, _ = fc.graph(orc, 64, 0)
    _run_grid(_device(native, orc, 64, 0), queries, rc.replays(orc, 64, 0, "gist", ef), ef, ("ef", ef))


@pytest.mark.parametrize("dim", [16, 128])
def test_tie_rows(native, orc, dim):
    """The radius is a distance many rows tie at: all of them are hits, and ties are ordered by id."""
    _, queries, _ = fc.graph(orc, dim, 0, "tie")
    dev = _device(native, orc, dim, 0, "tie")
    rs = rc.replays(orc, dim, 0, "tie", 20)
    for m in (5, 40, 150):
        radii = _mth(rs, m)
        tied = [sum(np.float32(d) == radii[i] for _, d in r["pairs"]) for i, r in enumerate(rs)]
        assert max(tied) >= 2, (dim, m, tied)
        got = dev.range_search(queries, 20, radii, 256)
        rc.assert_matches(got, rs, radii, 256, ("tie", dim, m))
        for i in range(len(rs)):  # stated directly: inside a tie the ids ascend
            n = int(got[0][i])
            d, v = got[2][i][:n], got[1][i][:n].astype(np.int64)
            assert ((np.diff(d) > 0) | ((np.diff(d) == 0) & (np.diff(v) > 0))).all(), (dim, m, i)
    rc.assert_matches(dev.range_search(queries, 20, float(FLT_MAX), 100), rs, FLT_MAX, 100, ("tie", dim, "cap"))


def test_all_zero_ip_query(native, orc):
    """Every distance is -0.0: radius 0.0 and radius -0.0 both return all 544 rows by id with the measured
    bits; the largest negative radius returns none."""
    r = rc.zero_query_replay(orc)
    dev = _device(native, orc, 64, 1)
    q = np.zeros((1, 64), np.float32)
    for radius in (0.0, -0.0):
        got = dev.range_search(q, 40, radius, 1024)
        assert int(got[0][0]) == 544
        assert (got[2][0][:544].view(np.uint32) == 0x80000000).all()
        assert (np.diff(got[1][0][:544].astype(np.int64)) > 0).all()
        rc.assert_matches(got, [r], radius, 1024, ("zero", radius))
    got = dev.range_search(q, 40, -1e-30, 1024)
    assert int(got[0][0]) == 0
    rc.assert_matches(got, [r], -1e-30, 1024, "zero none")


@pytest.mark.parametrize("share", [0.1, 0.02])
@pytest.mark.parametrize("dim,metric", [(64, 0), (128, 1), (960, 0)])
def test_masks(native, orc, dim, metric, share):
    _, queries, _ = fc.graph(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    rs = rc.replays(orc, dim, metric, "gist", 40, share)
    words = _words(fc.mask(fc.N, share))
    for radius, cap in ((float(FLT_MAX), 4096), (float(FLT_MAX), 7), (_mth(rc.replays(orc, dim, metric, "gist", 40), 100), 64)):
        rc.assert_matches(dev.range_search(queries, 40, radius, cap, words), rs, radius, cap, ("mask", dim, share, cap))


@pytest.mark.parametrize("dim", [64, 960])
def test_three_masks_in_one_batch(native, orc, dim):
    _, queries, _ = fc.graph(orc, dim, 0)
    dev = _device(native, orc, dim, 0)
    shares = (0.1, 1.0, 0.02)
    groups = np.arange(len(queries)) % 3
    words = _words(np.stack([fc.mask(fc.N, s) for s in shares]))
    rs = [rc.replays(orc, dim, 0, "gist", 40, shares[g])[i] for i, g in enumerate(groups)]
    for cap in (4096, 20):
        got = dev.range_search(queries, 40, float(FLT_MAX), cap, words, groups.astype(np.uint32))
        rc.assert_matches(got, rs, FLT_MAX, cap, ("three masks", dim, cap))


@pytest.mark.parametrize("dim,metric", [(64, 0), (128, 1)])
def test_all_zero_mask_and_no_mask(native, orc, dim, metric):
    _, queries, _ = fc.graph(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    got = dev.range_search(queries, 40, float(FLT_MAX), 64, _words(np.zeros(fc.N, bool)))
    assert not got[0].any() and (got[1] == fc.EMPTY).all() and (got[2] == FLT_MAX).all()
    assert np.array_equal(got[3], dev.search(queries, 10, 40)[2])
    rc.assert_matches(got, rc.replays(orc, dim, metric, "gist", 40, 0.0), FLT_MAX, 64, "zero mask")
    none = dev.range_search(queries, 40, float(FLT_MAX), 4096)
    ones = dev.range_search(queries, 40, float(FLT_MAX), 4096, _words(np.ones(fc.N, bool)))
    for a, b in zip(none, ones):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _index(metric="l2", **kw):
    import alayalite_amd

    _index.count = getattr(_index, "count", 0) + 1
    return alayalite_amd.Client().create_index(f"range{_index.count}", metric=metric, capacity=fc.N + 64, **kw)


def _view_of_index(orc, idx, rows, metric, **kw):
    l0, levels, off, ue, ep, ur, _ = idx.native().graph_arrays()
    return orc.IndexView(rows, l0, levels, off, ue, ur, ep, metric=metric, **kw)


def _assert_csr(got, rs, radius, cap, id_type, what):
    """Index.range_search's (lims, ids, dists, counts) against the restatement."""
    lims, ids, dists, counts = got
    assert lims.dtype == np.int64 and lims.shape == (len(rs) + 1,) and lims[0] == 0
    assert ids.dtype == id_type and dists.dtype == np.float32 and counts.dtype == np.uint32
    assert ids.shape == dists.shape == (int(lims[-1]),)
    for i, (r, rad) in enumerate(zip(rs, rc.radii_of(rs, radius))):
        n, w_ids, w_d = rc.want_row(r, rad, cap)
        kept = min(n, cap)
        assert int(counts[i]) == n and int(lims[i + 1] - lims[i]) == kept, (what, i, counts[i], n, lims[i:i + 2])
        assert np.array_equal(ids[lims[i]:lims[i + 1]].astype(np.uint32), w_ids[:kept]), (what, i)
        assert np.array_equal(dists[lims[i]:lims[i + 1]].view(np.uint32), w_d[:kept].view(np.uint32)), (what, i)


def test_removed_rows_never_come_back(native, orc):
    base, queries = dc.rows(64)
    idx = _index()
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    lims, first, _, _ = idx.range_search(queries.copy(), float(FLT_MAX), 40, 4096)
    removed = sorted({int(v) for i in range(len(queries)) for v in first[lims[i]:lims[i] + 3]})
    assert len(removed) >= 12
    for v in removed:
        idx.remove(v)
    valid = np.full((fc.N + 7) // 8, 0xFF, np.uint8)
    for v in removed:
        valid[v >> 3] &= ~np.uint8(1 << (v & 7))
    view = _view_of_index(orc, idx, base, 0, valid=valid)
    rs = rc.replays(orc, 64, 0, "removed", 40, view=view, queries=queries, allow=np.ones(fc.N, bool))
    for cap in (4096, 50):  # radius FLT_MAX is a removed row's own distance: still never a hit
        got = idx.range_search(queries.copy(), float(FLT_MAX), 40, cap)
        assert not np.isin(got[1], removed).any()
        _assert_csr(got, rs, FLT_MAX, cap, np.uint32, ("removed", cap))
        assert np.array_equal(idx.native().last_counters(), np.array([r["counters"] for r in rs], np.uint32))


def test_entry_points_without_overlay(native, orc):
    """A graph without overlay: every entry point is offered in turn, a repeated one twice, and it stays twice."""
    base, queries, arrays = fc.graph(orc, 64, 0)
    l0 = arrays[0]
    eps = np.array([5, 77, 5, 901], np.uint32)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0, None)
    dev.set_graph(native.Graph.from_arrays(l0, None, None, None, 0, 0, eps))
    view = orc.IndexView(base, l0, None, None, None, 0, 0)
    rs = rc.replays(orc, 64, 0, "eps", 40, view=view, queries=queries, allow=np.ones(fc.N, bool), eps=eps)
    for cap in (4096, 3, 2):
        got = dev.range_search(queries, 40, float(FLT_MAX), cap)
        rc.assert_matches(got, rs, FLT_MAX, cap, ("eps", cap))
    twice = dev.range_search(queries, 40, float(FLT_MAX), 4096)[1]
    assert all(list(row).count(5) == 2 for row in twice)  # the entry points are hits of every query


@pytest.mark.parametrize("deg", ["dense", "dup"])
def test_wide_rows_and_repeated_edges(native, orc, deg):
    """R = 64: up to 64 hits in one append; caps 65 and 100 are straddled by such appends."""
    base, queries, arrays = dc.dense(native, 128) if deg == "dense" else dc.duplicated(native, 128)
    dev = dc.device_of(native, base, arrays)
    view = dc.view_of(orc, base, arrays)
    rs = rc.replays(orc, 128, 0, deg, 40, view=view, queries=queries, allow=np.ones(fc.N, bool))
    for cap in (65, 100, 4096):
        rc.assert_matches(dev.range_search(queries, 40, float(FLT_MAX), cap), rs, FLT_MAX, cap, (deg, cap))
    radii = _mth(rs, 90)
    rc.assert_matches(dev.range_search(queries, 40, radii, 65), rs, radii, 65, (deg, "m 90"))


@pytest.mark.parametrize("dim", [64, 960])
def test_forced_spill(native, orc, dim):
    base, queries, arrays = fc.graph(orc, dim, 0)
    dev = dc.device_of(native, base, arrays)
    dev.set_hash_log2(8)
    rs = rc.replays(orc, dim, 0, "gist", 40)
    assert min(r["counters"][0] for r in rs) > 256
    got = dev.range_search(queries, 40, float(FLT_MAX), 4096)
    assert dev.last_plan()["hash_log2"] == 8
    rc.assert_matches(got, rs, FLT_MAX, 4096, ("spill", dim))
    radii = _mth(rs, 65)
    rc.assert_matches(dev.range_search(queries, 40, radii, 64), rs, radii, 64, ("spill", dim, "m 65"))


def test_two_workgroups_run_the_whole_batch(native, orc, monkeypatch):
    base, _, arrays = fc.graph(orc, 64, 0)
    dev = _device(native, orc, 64, 0)
    view = dc.view_of(orc, base, arrays)
    rs = rc.replays(orc, 64, 0, "base", 16, view=view, queries=base, allow=np.ones(fc.N, bool))
    radii = np.full(len(base), np.median(_mth(rs, 25)), np.float32)  # about half the lists are truncated at cap 24
    monkeypatch.setenv("ALAYA_FILTER_GRID", "2")
    got = dev.range_search(base, 16, radii, 24)
    groups, waves = dev.last_launch()
    assert groups == 2 and groups * waves * 100 <= len(base), (groups, waves)
    assert (got[0] > 24).any() and (got[0] <= 24).any()
    rc.assert_matches(got, rs, radii, 24, "grid 2")


def test_index_cos(native, orc):
    """Index.range_search normalises COS queries as batch_search does; the radius is a negative inner product."""
    base, queries = dc.rows(64)
    rows = base.copy()
    idx = _index("cosine")
    idx.fit(rows, ef_construction=100, num_threads=1)  # normalises rows in place
    view = _view_of_index(orc, idx, rows, 2)
    rs = rc.replays(orc, 64, 2, "cos", 40, view=view, queries=[orc.normalize(q) for q in queries], allow=np.ones(fc.N, bool))
    radii = _mth(rs, 30)
    assert (radii < 0).all()
    _assert_csr(idx.range_search(queries.copy(), radii, 40, 64), rs, radii, 64, np.uint32, "cos")
    scalar = float(np.median(radii))
    got = idx.range_search(queries.copy(), scalar, 40, 16)
    _assert_csr(got, rs, scalar, 16, np.uint32, "cos scalar")
    assert (got[3] > 16).any()  # some list is truncated
    chunked = idx.range_search(queries.copy(), scalar, 40, 16, _chunk=5)  # 5 + 5 + 2 queries
    for a, b in zip(got, chunked):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    allow = fc.mask(fc.N, 0.1)
    rs_m = rc.replays(orc, 64, 2, "cos", 40, view=view, queries=[orc.normalize(q) for q in queries], allow=allow)
    _assert_csr(idx.range_search(queries.copy(), scalar, 40, 64, allow=allow), rs_m, scalar, 64, np.uint32, "cos mask")
    assert np.array_equal(idx.native().last_counters(), np.array([r["counters"] for r in rs_m], np.uint32))


def test_index_uint64_ids_and_uint8_rows(native, orc):
    """Ids in the index's id type; uint8 rows take the generic element order on the runtime-width kernel."""
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 256, (fc.N, 24)).astype(np.uint8)
    queries = rng.integers(0, 256, (fc.NQ, 24)).astype(np.uint8)
    idx = _index(data_type=np.uint8, id_type=np.uint64)
    idx.fit(rows, ef_construction=100, num_threads=1)
    view = _view_of_index(orc, idx, rows.astype(np.float32), 0, generic=True)
    rs = rc.replays(orc, 24, 0, "u8", 40, view=view, queries=queries.astype(np.float32), allow=np.ones(fc.N, bool))
    radii = _mth(rs, 50)
    _assert_csr(idx.range_search(queries, radii, 40, 64), rs, radii, 64, np.uint64, "u8")
    two = np.stack([fc.mask(fc.N, 0.5), fc.mask(fc.N, 0.1)])
    groups = np.arange(fc.NQ) % 2
    rs2 = [rc.replays(orc, 24, 0, "u8", 40, view=view, queries=[queries[i].astype(np.float32)], allow=two[g])[0]
           for i, g in enumerate(groups)]
    _assert_csr(idx.range_search(queries, float(FLT_MAX), 40, 30, allow=two, groups=groups), rs2, FLT_MAX, 30, np.uint64, "u8 groups")
    empty = idx.range_search(queries[:0], 1.0, 40, 8)
    assert empty[0].tolist() == [0] and empty[1].dtype == np.uint64 and empty[1].size == empty[2].size == empty[3].size == 0
    # refusals
    for bad in (dict(radius=float("nan")), dict(radius=np.full(fc.NQ, np.nan, np.float32)), dict(radius=np.ones(fc.NQ + 1)),
                dict(radius=np.ones((fc.NQ, 1))), dict(max_results=0), dict(max_results=4097), dict(ef_search=0),
                dict(allow=np.ones(fc.N + 1, bool)), dict(allow=two), dict(groups=groups),
                dict(allow=two, groups=np.full(fc.NQ, 2))):
        kw = dict(radius=1.0, ef_search=40, max_results=64)
        kw.update(bad)
        with pytest.raises(ValueError):
            idx.range_search(queries, **kw)
    with pytest.raises(ValueError):
        idx.range_search(queries[:, :20], 1.0, 40, 64)


def test_refusals(native, orc):
    base, queries, arrays = fc.graph(orc, 64, 0)
    words = _words(fc.mask(fc.N, 0.1))
    dev = _device(native, orc, 64, 0)
    with pytest.raises(ValueError, match="1..4096"):
        dev.range_search(queries, 40, 1.0, 4097)
    with pytest.raises(ValueError, match="1..4096"):
        dev.range_search(queries, 40, 1.0, 0)
    with pytest.raises(ValueError, match="ef"):
        dev.range_search(queries, 0, 1.0, 64)
    with pytest.raises(ValueError, match="NaN"):
        dev.range_search(queries, 40, float("nan"), 64)
    with pytest.raises(ValueError, match="NaN"):
        dev.range_search(queries, 40, np.where(np.arange(len(queries)) == 7, np.nan, 1.0).astype(np.float32), 64)
    with pytest.raises(ValueError):
        dev.range_search(queries, 40, np.ones(len(queries) - 1, np.float32), 64)
    with pytest.raises(ValueError):
        dev.range_search(queries, 40, 1.0, 64, words[:, :-1])
    with pytest.raises(ValueError):
        dev.range_search(queries, 40, 1.0, 64, np.concatenate([words, words]))  # two masks, no indices
    with pytest.raises(ValueError):
        dev.range_search(queries, 40, 1.0, 64, words, np.ones(len(queries), np.uint32))  # index past n_masks
    with pytest.raises(ValueError):
        dev.range_search(queries, 40, 1.0, 64, None, np.zeros(len(queries), np.uint32))  # indices without masks
    sq = dc.device_of(native, base, arrays)
    mn, mx = native.sq8_train(base)
    sq.set_sq8(native.sq8_encode(base, mn, mx, 1), mn, mx, native.host_sq8_order())
    with pytest.raises(ValueError, match="SQ8"):
        sq.range_search(queries, 40, 1.0, 64)
    idx = _index(quantization_type="sq8")
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    with pytest.raises(ValueError, match="SQ8"):
        idx.range_search(queries.copy(), 1.0, 40, 64)


def test_device_entry(native, orc):
    """Results on torch device tensors equal the host entry's; nothing is read back before the stream is
    synchronised."""
    import torch

    _, queries, _ = fc.graph(orc, 64, 0)
    dev = _device(native, orc, 64, 0)
    rs = rc.replays(orc, 64, 0, "gist", 40, 0.1)
    radii = _mth(rc.replays(orc, 64, 0, "gist", 40), 200)
    cap, nq = 33, len(queries)
    groups = np.zeros(nq, np.uint32)
    host = dev.range_search(queries, 40, radii, cap, _words(fc.mask(fc.N, 0.1)), groups)
    rc.assert_matches(host, rs, radii, cap, "host")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_q = torch.from_numpy(queries.copy()).cuda()
        t_r = torch.from_numpy(radii).cuda()
        t_w = torch.from_numpy(_words(fc.mask(fc.N, 0.1)).view(np.int32)).cuda()
        t_g = torch.from_numpy(groups.view(np.int32)).cuda()
        t_counts = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
        t_ids = torch.full((nq, cap), -2, dtype=torch.int32, device="cuda")
        t_d = torch.zeros((nq, cap), dtype=torch.float32, device="cuda")
        t_c = torch.zeros((nq, 4), dtype=torch.int32, device="cuda")
        dev.range_search_device(t_q.data_ptr(), nq, 40, t_r.data_ptr(), cap, t_w.data_ptr(), 1, t_g.data_ptr(),
                                t_counts.data_ptr(), t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(), stream.cuda_stream)
        # no mask at all through the device entry, on the same stream
        n_counts = torch.zeros((nq,), dtype=torch.int32, device="cuda")
        n_ids = torch.zeros((nq, cap), dtype=torch.int32, device="cuda")
        n_d = torch.zeros((nq, cap), dtype=torch.float32, device="cuda")
        dev.range_search_device(t_q.data_ptr(), nq, 40, t_r.data_ptr(), cap, 0, 0, 0, n_counts.data_ptr(), n_ids.data_ptr(),
                                n_d.data_ptr(), 0, stream.cuda_stream)
    stream.synchronize()
    got = (t_counts.cpu().numpy().view(np.uint32), t_ids.cpu().numpy().view(np.uint32), t_d.cpu().numpy(),
           t_c.cpu().numpy().view(np.uint32))
    for a, b in zip(got, host):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    plain = dev.range_search(queries, 40, radii, cap)
    assert np.array_equal(n_counts.cpu().numpy().view(np.uint32), plain[0])
    assert np.array_equal(n_ids.cpu().numpy().view(np.uint32), plain[1])
    assert np.array_equal(n_d.cpu().numpy().view(np.uint32), plain[2].view(np.uint32))
