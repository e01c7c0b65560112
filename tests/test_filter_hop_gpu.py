"""The through search on the device (filtered_hop_search_kernel) against its restatement
(tests/filter_hop_common.py): ids, distance bits, the four counters and n_through equal for every query,
none left out.  test_filter_hop_host.py pins the restatement and that these inputs reach the kernel's
branches: a queue that flushes mid-pop, an empty through list, a row two through rows offer, a through row
that repeats an id.

Each case is 2000 rows and at most 12 queries, except the ALAYA_FILTER_GRID case, whose queries are the
2000 base rows so that two waves run a thousand queries each."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import filter_hop_common as hc

pytestmark = pytest.mark.gpu

KEFS, SHAPES = hc.KEFS, hc.SHAPES
_devices = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("ALAYA_FILTER_GRID", "ALAYA_SEARCH_WAVES", "ALAYA_VIS_LIMIT", "ALAYA_VIS_LIMIT_PCT"):
        monkeypatch.delenv(name, raising=False)


def _words(allow, n):
    from alayalite_amd.utils import pack_allow

    return pack_allow(allow, n)


def _device(native, orc, dim, metric, kind="gist"):
    key = (dim, metric, kind)
    if key not in _devices:
        base, _, arrays = fc.graph(orc, dim, metric, kind)
        _devices[key] = dc.device_of(native, base, arrays, metric)
    return _devices[key]


@pytest.mark.parametrize("k,ef,share", KEFS)
@pytest.mark.parametrize("dim,metric", SHAPES)
def test_main_grid(native, orc, dim, metric, k, ef, share):
    _, queries, _ = fc.graph(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    got = dev.filtered_search_hop(queries, k, ef, _words(fc.mask(fc.N, share), fc.N))
    hc.assert_matches(got, hc.replays(orc, dim, metric, "gist", k, ef, share), (dim, metric, k, ef, share))


@pytest.mark.parametrize("dim,metric", [(64, 0), (128, 1), (960, 0)])
def test_all_ones_mask_is_the_filtered_search(native, orc, dim, metric):
    """No row is stepped through: the device's own filtered_search, bit for bit, and n_through 0."""
    _, queries, _ = fc.graph(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    words = _words(np.ones(fc.N, bool), fc.N)
    for k, ef in ((10, 40), (65, 10)):
        ids, d, cnt, thr = dev.filtered_search_hop(queries, k, ef, words)
        ids0, d0, cnt0 = dev.filtered_search(queries, k, ef, words)
        assert np.array_equal(ids, ids0) and np.array_equal(d.view(np.uint32), d0.view(np.uint32))
        assert np.array_equal(cnt, cnt0)
        assert thr.shape == (len(queries),) and not thr.any()


@pytest.mark.parametrize("dim,metric", [(64, 0), (128, 1), (960, 0)])
def test_all_zero_mask(native, orc, dim, metric):
    """Every slot empty, no distance at level 0, and the one pop of the entry, whose whole row is stepped
    through."""
    _, queries, _ = fc.graph(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    ids, d, cnt, thr = dev.filtered_search_hop(queries, 10, 40, _words(np.zeros(fc.N, bool), fc.N))
    assert (ids == fc.EMPTY).all() and (d == fc.FLT_MAX).all()
    assert (cnt[:, 0] == 0).all() and (cnt[:, 1] == 1).all()
    assert (thr > 0).all()
    hc.assert_matches((ids, d, cnt, thr), hc.replays(orc, dim, metric, "gist", 10, 40, 0.0), "zero")


@pytest.mark.parametrize("dim", [64, 960])
def test_three_masks_in_one_batch(native, orc, dim):
    _, queries, _ = fc.graph(orc, dim, 0)
    dev = _device(native, orc, dim, 0)
    shares = (0.1, 0.5, 0.02)
    groups = np.arange(len(queries)) % 3
    words = _words(np.stack([fc.mask(fc.N, s) for s in shares]), fc.N)
    got = dev.filtered_search_hop(queries, 10, 16, words, groups.astype(np.uint32))
    want = [hc.replays(orc, dim, 0, "gist", 10, 16, shares[g])[i] for i, g in enumerate(groups)]
    hc.assert_matches(got, want, "three masks")


@pytest.mark.parametrize("dim", [16, 128])
def test_tie_rows(native, orc, dim):
    _, queries, _ = fc.graph(orc, dim, 0, "tie")
    dev = _device(native, orc, dim, 0, "tie")
    got = dev.filtered_search_hop(queries, 10, 20, _words(fc.mask(fc.N, 0.3), fc.N))
    hc.assert_matches(got, hc.replays(orc, dim, 0, "tie", 10, 20, 0.3), ("tie", dim))


def _index(metric="l2", **kw):
    import alayalite_amd

    _index.count = getattr(_index, "count", 0) + 1
    return alayalite_amd.Client().create_index(f"hop{_index.count}", metric=metric, capacity=fc.N + 64, **kw)


def _view_of_index(orc, idx, rows, metric, **kw):
    l0, levels, off, ue, ep, ur, _ = idx.native().graph_arrays()
    return orc.IndexView(rows, l0, levels, off, ue, ur, ep, metric=metric, **kw)


def _through(idx, queries, k, ef, allow, **kw):
    ids, d = idx.filtered_search(queries, k, ef, allow=allow, expand="through", **kw)
    return ids, d, idx.native().last_counters(), idx.native().last_through()


def test_cos(native, orc):
    """Index.filtered_search normalises COS queries as batch_search does."""
    base, queries = dc.rows(64)
    rows = base.copy()
    idx = _index("cosine")
    idx.fit(rows, ef_construction=100, num_threads=1)  # normalises rows in place
    allow = fc.mask(fc.N, 0.1)
    got = _through(idx, queries.copy(), 10, 16, allow)
    view = _view_of_index(orc, idx, rows, 2)
    want = hc.replays(orc, 64, 2, "cos", 10, 16, 0.1, view=view, queries=[orc.normalize(q) for q in queries], allow=allow)
    hc.assert_matches(got, want, "cos")


def test_uint64_ids(native, orc):
    """Ids come in the index's id type (empty slots: its maximum), two masks go through Index, and the
    default expansion is untouched by a through call before it."""
    base, queries = dc.rows(64)
    idx = _index(id_type=np.uint64)
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    allow = fc.mask(fc.N, 0.02)
    allow[allow.nonzero()[0][8:]] = False  # 8 rows allowed: every query comes up short of k = 10
    ids, d, cnt, thr = _through(idx, queries.copy(), 10, 16, allow)
    assert ids.dtype == np.uint64 and ids.shape == (fc.NQ, 10)
    view = _view_of_index(orc, idx, base, 0)
    want = hc.replays(orc, 64, 0, "u64", 10, 16, 0.02, view=view, queries=queries, allow=allow)
    empty = ids == np.iinfo(np.uint64).max
    assert empty[:, 8:].all()
    hc.assert_matches((np.where(empty, fc.EMPTY, ids).astype(np.uint32), d, cnt, thr), want, "u64")
    two = np.stack([allow, fc.mask(fc.N, 0.5)])
    groups = np.arange(fc.NQ) % 2
    ids2, d2 = idx.filtered_search(queries.copy(), 10, 16, allow=two, groups=groups, expand="through")
    assert np.array_equal(ids2[::2], ids[::2]) and np.array_equal(d2[::2].view(np.uint32), d[::2].view(np.uint32))
    plain = idx.filtered_search(queries.copy(), 10, 16, allow=allow)
    named = idx.filtered_search(queries.copy(), 10, 16, allow=allow, expand="plain")
    assert np.array_equal(plain[0], named[0]) and len(idx.native().last_through()) == 0
    fc.assert_matches((np.where(plain[0] == np.iinfo(np.uint64).max, fc.EMPTY, plain[0]).astype(np.uint32), plain[1],
                       idx.native().last_counters()),
                      fc.replays(orc, 64, 0, "u64", 10, 16, 0.02, view=view, queries=queries, allow=allow), "plain")


def test_removed_rows_are_stepped_through(native, orc):
    base, queries = dc.rows(64)
    idx = _index()
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    # the rows a through search would return: remove them, then allow them (and little else)
    allow = fc.mask(fc.N, 0.1)
    first = _through(idx, queries.copy(), 10, 16, allow)[0]
    removed = sorted({int(v) for v in first[:, :3].ravel() if v != fc.EMPTY})
    assert len(removed) >= 12
    for v in removed:
        idx.remove(v)
    valid = np.full((fc.N + 7) // 8, 0xFF, np.uint8)
    for v in removed:
        valid[v >> 3] &= ~np.uint8(1 << (v & 7))
    assert allow[removed].all()  # still allowed: only the validity bitmap keeps them out
    got = _through(idx, queries.copy(), 10, 16, allow)
    assert not np.isin(got[0], removed).any()
    view = _view_of_index(orc, idx, base, 0, valid=valid)
    want = hc.replays(orc, 64, 0, "removed", 10, 16, 0.1, view=view, queries=queries, allow=allow)
    hc.assert_matches(got, want, "removed")
    # with every row allowed the removed ones are the only through rows, and none sits in the pool at FLT_MAX
    ones = np.ones(fc.N, bool)
    got = _through(idx, queries.copy(), 10, 16, ones)
    want = hc.replays(orc, 64, 0, "removed", 10, 16, 1.0, view=view, queries=queries, allow=ones)
    hc.assert_matches(got, want, "removed, all ones")
    assert sum(r["counters"][4] for r in want) > 0
    assert all(d != fc.FLT_MAX for r in want for v, d in r["pool"] if v not in r["entries"])


def test_inserted_rows_with_a_longer_mask(native, orc):
    base, queries = dc.rows(64)
    idx = _index()
    idx.fit(base[:1990].copy(), ef_construction=100, num_threads=1)
    for row in base[1990:]:
        idx.insert(row.copy(), 48)
    assert idx.get_data_num() == fc.N
    with pytest.raises(ValueError):
        idx.filtered_search(queries.copy(), 10, 16, allow=np.ones(1990, bool), expand="through")
    allow = fc.mask(fc.N, 0.1)
    allow[1990:] = True
    got = _through(idx, queries.copy(), 10, 16, allow)
    view = _view_of_index(orc, idx, base, 0)
    want = hc.replays(orc, 64, 0, "inserted", 10, 16, 0.1, view=view, queries=queries, allow=allow)
    hc.assert_matches(got, want, "inserted")


@pytest.mark.parametrize("deg", ["dense", "dup"])
def test_wide_rows_and_repeated_edges(native, orc, deg):
    """R = 64 at shares that make most neighbours through rows: exact 64-NN rows, and rows that repeat an id."""
    base, queries, arrays = dc.dense(native, 128) if deg == "dense" else dc.duplicated(native, 128)
    dev = dc.device_of(native, base, arrays)
    view = dc.view_of(orc, base, arrays)
    for k, ef, share in ((10, 16, 0.1), (65, 10, 0.3)):
        allow = fc.mask(fc.N, share)
        got = dev.filtered_search_hop(queries, k, ef, _words(allow, fc.N))
        want = hc.replays(orc, 128, 0, deg, k, ef, share, view=view, queries=queries, allow=allow)
        hc.assert_matches(got, want, (deg, k, ef))


def test_entry_points_without_overlay(native, orc):
    """A graph without overlay: every entry point goes into the pool and, when passable, to the result pool, in
    turn, a repeated one twice."""
    base, queries, arrays = fc.graph(orc, 64, 0)
    l0 = arrays[0]
    eps = np.array([5, 77, 5, 901], np.uint32)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0, None)
    dev.set_graph(native.Graph.from_arrays(l0, None, None, None, 0, 0, eps))
    view = orc.IndexView(base, l0, None, None, None, 0, 0)
    allow = fc.mask(fc.N, 0.02)
    allow[[5, 901]] = True
    allow[77] = False
    for k, ef in ((10, 16), (3, 2)):
        got = dev.filtered_search_hop(queries, k, ef, _words(allow, fc.N))
        want = hc.replays(orc, 64, 0, "eps", k, ef, 0.02, view=view, queries=queries, allow=allow, eps=eps)
        hc.assert_matches(got, want, ("eps", k, ef))
        assert all([v for v, _ in r["pairs"]].count(5) == 2 for r in want)
        assert not np.isin(got[0], [77]).any()


@pytest.mark.parametrize("dim", [64, 960])
def test_forced_spill(native, orc, monkeypatch, dim):
    """A 256-slot visited table that spills at 64 entries (ALAYA_VIS_LIMIT): every query marks more ids than
    that, direct neighbours and through candidates together, and goes on in the bitset."""
    base, queries, arrays = fc.graph(orc, dim, 0)
    dev = dc.device_of(native, base, arrays)
    dev.set_hash_log2(8)
    monkeypatch.setenv("ALAYA_VIS_LIMIT", "64")
    want = hc.replays(orc, dim, 0, "gist", 10, 16, 0.1)
    assert min(r["counters"][0] + r["counters"][4] for r in want) > 192  # ids marked: past the table's limit
    got = dev.filtered_search_hop(queries, 10, 16, _words(fc.mask(fc.N, 0.1), fc.N))
    assert dev.last_plan()["hash_log2"] == 8
    hc.assert_matches(got, want, ("spill", dim))


def test_two_workgroups_run_the_whole_batch(native, orc, monkeypatch):
    """ALAYA_FILTER_GRID=2 with the 2000 base rows as queries: each wave runs about a thousand queries in
    sequence, resetting its pools and its visited set in between."""
    base, _, arrays = fc.graph(orc, 64, 0)
    dev = _device(native, orc, 64, 0)
    allow = fc.mask(fc.N, 0.1)
    monkeypatch.setenv("ALAYA_FILTER_GRID", "2")
    got = dev.filtered_search_hop(base, 10, 8, _words(allow, fc.N))
    groups, waves = dev.last_launch()
    assert groups == 2 and groups * waves * 100 <= len(base), (groups, waves)
    view = dc.view_of(orc, base, arrays)
    want = hc.replays(orc, 64, 0, "base", 10, 8, 0.1, view=view, queries=base, allow=allow)
    hc.assert_matches(got, want, "grid 2")


def test_refusals(native, orc):
    base, queries, arrays = fc.graph(orc, 64, 0)
    words = _words(fc.mask(fc.N, 0.1), fc.N)
    dev = _device(native, orc, 64, 0)
    with pytest.raises(ValueError, match="1..224"):
        dev.filtered_search_hop(queries, 225, 40, words)
    with pytest.raises(ValueError):
        dev.filtered_search_hop(queries, 0, 40, words)
    with pytest.raises(ValueError, match="ef"):
        dev.filtered_search_hop(queries, 10, 0, words)
    with pytest.raises(ValueError):
        dev.filtered_search_hop(queries, 10, 40, words[:, :-1])
    sq = dc.device_of(native, base, arrays)
    mn, mx = native.sq8_train(base)
    sq.set_sq8(native.sq8_encode(base, mn, mx, 1), mn, mx, native.host_sq8_order())
    with pytest.raises(ValueError, match="SQ8"):
        sq.filtered_search_hop(queries, 10, 40, words)
    # through Index: an unknown expansion, rerank_pool with the through one, an SQ8 index
    allow = fc.mask(fc.N, 0.1)
    idx = _index()
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    with pytest.raises(ValueError, match="expand"):
        idx.filtered_search(queries.copy(), 10, 40, allow=allow, expand="nonsense")
    with pytest.raises(ValueError, match="f32 indexes only"):
        idx.filtered_search(queries.copy(), 10, 40, allow=allow, rerank_pool=20, expand="through")
    sqi = _index(quantization_type="sq8")
    sqi.fit(base.copy(), ef_construction=100, num_threads=1)
    with pytest.raises(ValueError, match="f32 indexes only"):
        sqi.filtered_search(queries.copy(), 10, 40, allow=allow, expand="through")
    with pytest.raises(ValueError, match="f32 indexes only"):
        sqi.native().filtered_search(queries.copy(), 10, 40, _words(allow, fc.N), None, 0, True)
