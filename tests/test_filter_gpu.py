"""The filtered graph search on the device (filtered_search_kernel) against its restatement
(tests/filter_common.py): ids, distance bits and the four counters equal for every query, none left
out.  test_filter_host.py pins the restatement and that these inputs reach the result pool's paths.

Each case is 2000 rows and at most 12 queries, except the ALAYA_FILTER_GRID case, whose queries are the
2000 base rows so that two waves run a thousand queries each on one result pool."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc

pytestmark = pytest.mark.gpu

KEFS = [(10, 40, 0.1), (10, 40, 0.02), (65, 10, 0.5), (5, 1, 1.0), (224, 10, 1.0), (1, 40, 0.1)]
SHAPES = [(64, 0), (64, 1), (100, 0), (128, 0), (128, 1), (960, 0)]
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
    got = dev.filtered_search(queries, k, ef, _words(fc.mask(fc.N, share), fc.N))
    fc.assert_matches(got, fc.replays(orc, dim, metric, "gist", k, ef, share), (dim, metric, k, ef, share))


@pytest.mark.parametrize("dim,metric", [(64, 0), (128, 1), (960, 0)])
def test_all_zero_mask(native, orc, dim, metric):
    """Every slot empty; the counters are the unfiltered search's."""
    _, queries, _ = fc.graph(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    ids, d, cnt = dev.filtered_search(queries, 10, 40, _words(np.zeros(fc.N, bool), fc.N))
    assert (ids == fc.EMPTY).all() and (d == fc.FLT_MAX).all()
    fc.assert_matches((ids, d, cnt), fc.replays(orc, dim, metric, "gist", 10, 40, 0.0), "zero")
    assert np.array_equal(cnt, dev.search(queries, 10, 40)[2])


@pytest.mark.parametrize("dim", [64, 960])
def test_three_masks_in_one_batch(native, orc, dim):
    _, queries, _ = fc.graph(orc, dim, 0)
    dev = _device(native, orc, dim, 0)
    shares = (0.1, 0.5, 0.02)
    groups = np.arange(len(queries)) % 3
    words = _words(np.stack([fc.mask(fc.N, s) for s in shares]), fc.N)
    got = dev.filtered_search(queries, 10, 40, words, groups.astype(np.uint32))
    want = [fc.replays(orc, dim, 0, "gist", 10, 40, shares[g])[i] for i, g in enumerate(groups)]
    fc.assert_matches(got, want, "three masks")


@pytest.mark.parametrize("dim", [16, 128])
def test_tie_rows(native, orc, dim):
    _, queries, _ = fc.graph(orc, dim, 0, "tie")
    dev = _device(native, orc, dim, 0, "tie")
    got = dev.filtered_search(queries, 10, 20, _words(fc.mask(fc.N, 0.3), fc.N))
    fc.assert_matches(got, fc.replays(orc, dim, 0, "tie", 10, 20, 0.3), ("tie", dim))


def _index(metric="l2", **kw):
    import alayalite_amd

    _index.count = getattr(_index, "count", 0) + 1
    return alayalite_amd.Client().create_index(f"filter{_index.count}", metric=metric, capacity=fc.N + 64, **kw)


def _view_of_index(orc, idx, rows, metric, **kw):
    l0, levels, off, ue, ep, ur, _ = idx.native().graph_arrays()
    return orc.IndexView(rows, l0, levels, off, ue, ur, ep, metric=metric, **kw)


def test_cos(native, orc):
    """Index.filtered_search normalises COS queries as batch_search does."""
    base, queries = dc.rows(64)
    rows = base.copy()
    idx = _index("cosine")
    idx.fit(rows, ef_construction=100, num_threads=1)  # normalises rows in place
    allow = fc.mask(fc.N, 0.1)
    ids, d = idx.filtered_search(queries.copy(), 10, 40, allow=allow)
    view = _view_of_index(orc, idx, rows, 2)
    want = fc.replays(orc, 64, 2, "cos", 10, 40, 0.1, view=view, queries=[orc.normalize(q) for q in queries], allow=allow)
    fc.assert_matches((ids, d, idx.native().last_counters()), want, "cos")


def test_uint64_ids_and_uint8_rows(native, orc):
    """Ids come in the index's id type (empty slots: its maximum); uint8 rows take the generic element
    order on the runtime-width kernel (d = 24 values below 256: every partial sum is an exact integer,
    so the oracle's f32 distance has the same bits in any order)."""
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 256, (fc.N, 24)).astype(np.uint8)
    queries = rng.integers(0, 256, (fc.NQ, 24)).astype(np.uint8)
    idx = _index(data_type=np.uint8, id_type=np.uint64)
    idx.fit(rows, ef_construction=100, num_threads=1)
    assert idx.get_data_num() == fc.N
    allow = fc.mask(fc.N, 0.02)
    allow[allow.nonzero()[0][8:]] = False  # 8 rows allowed: every query comes up short of k = 10
    ids, d = idx.filtered_search(queries, 10, 40, allow=allow)
    assert ids.dtype == np.uint64 and ids.shape == (fc.NQ, 10)
    view = _view_of_index(orc, idx, rows.astype(np.float32), 0, generic=True)
    want = fc.replays(orc, 24, 0, "u8", 10, 40, 0.02, view=view, queries=queries.astype(np.float32), allow=allow)
    empty = ids == np.iinfo(np.uint64).max
    assert empty[:, 8:].all()
    ids32 = np.where(empty, fc.EMPTY, ids).astype(np.uint32)
    fc.assert_matches((ids32, d, idx.native().last_counters()), want, "u8")
    # two masks through Index, and its argument checks
    two = np.stack([allow, fc.mask(fc.N, 0.5)])
    groups = np.arange(fc.NQ) % 2
    ids2, d2 = idx.filtered_search(queries, 10, 40, allow=two, groups=groups)
    assert np.array_equal(ids2[::2], ids[::2]) and np.array_equal(d2[::2].view(np.uint32), d[::2].view(np.uint32))
    with pytest.raises(ValueError):
        idx.filtered_search(queries, 10, 40, allow=np.ones(fc.N + 1, bool))
    with pytest.raises(ValueError):
        idx.filtered_search(queries, 10, 40, allow=two)
    with pytest.raises(ValueError):
        idx.filtered_search(queries, 10, 40, allow=two, groups=np.full(fc.NQ, 2))
    with pytest.raises(ValueError):
        idx.filtered_search(queries[:, :20], 10, 40, allow=allow)
    with pytest.raises(ValueError):
        idx.filtered_search(queries, 225, 40, allow=allow)


def test_removed_rows_never_come_back(native, orc):
    base, queries = dc.rows(64)
    idx = _index()
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    # the rows a filtered search would return: remove them, then allow them (and little else)
    allow = fc.mask(fc.N, 0.1)
    first, _ = idx.filtered_search(queries.copy(), 10, 40, allow=allow)
    removed = sorted({int(v) for v in first[:, :3].ravel() if v != fc.EMPTY})
    assert len(removed) >= 12
    for v in removed:
        idx.remove(v)
    valid = np.full((fc.N + 7) // 8, 0xFF, np.uint8)
    for v in removed:
        valid[v >> 3] &= ~np.uint8(1 << (v & 7))
    assert allow[removed].all()  # still allowed: only the validity bitmap keeps them out
    ids, d = idx.filtered_search(queries.copy(), 10, 40, allow=allow)
    assert not np.isin(ids, removed).any()
    view = _view_of_index(orc, idx, base, 0, valid=valid)
    want = fc.replays(orc, 64, 0, "removed", 10, 40, 0.1, view=view, queries=queries, allow=allow)
    fc.assert_matches((ids, d, idx.native().last_counters()), want, "removed")


def test_inserted_rows_with_a_longer_mask(native, orc):
    base, queries = dc.rows(64)
    idx = _index()
    idx.fit(base[:1990].copy(), ef_construction=100, num_threads=1)
    for row in base[1990:]:
        idx.insert(row.copy(), 48)
    assert idx.get_data_num() == fc.N
    with pytest.raises(ValueError):
        idx.filtered_search(queries.copy(), 10, 40, allow=np.ones(1990, bool))
    allow = fc.mask(fc.N, 0.1)
    allow[1990:] = True
    ids, d = idx.filtered_search(queries.copy(), 10, 40, allow=allow)
    view = _view_of_index(orc, idx, base, 0)
    want = fc.replays(orc, 64, 0, "inserted", 10, 40, 0.1, view=view, queries=queries, allow=allow)
    fc.assert_matches((ids, d, idx.native().last_counters()), want, "inserted")


@pytest.mark.parametrize("deg", ["dense", "dup"])
def test_wide_rows_and_repeated_edges(native, orc, deg):
    """R = 64: exact 64-NN rows (up to 64 fresh candidates offered at once) and rows that repeat an id."""
    base, queries, arrays = dc.dense(native, 128) if deg == "dense" else dc.duplicated(native, 128)
    dev = dc.device_of(native, base, arrays)
    view = dc.view_of(orc, base, arrays)
    for k, ef, share in ((10, 40, 0.1), (65, 10, 0.5)):
        allow = fc.mask(fc.N, share)
        got = dev.filtered_search(queries, k, ef, _words(allow, fc.N))
        want = fc.replays(orc, 128, 0, deg, k, ef, share, view=view, queries=queries, allow=allow)
        fc.assert_matches(got, want, (deg, k, ef))


def test_entry_points_without_overlay(native, orc):
    """A graph without overlay: every entry point is offered to the result pool in turn, a repeated one
    twice (Graph::initialize_search inserts it twice)."""
    base, queries, arrays = fc.graph(orc, 64, 0)
    l0 = arrays[0]
    eps = np.array([5, 77, 5, 901], np.uint32)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0, None)
    dev.set_graph(native.Graph.from_arrays(l0, None, None, None, 0, 0, eps))
    view = orc.IndexView(base, l0, None, None, None, 0, 0)
    allow = fc.mask(fc.N, 0.02)
    allow[[5, 901]] = True
    for k, ef in ((10, 40), (3, 2)):
        got = dev.filtered_search(queries, k, ef, _words(allow, fc.N))
        want = fc.replays(orc, 64, 0, "eps", k, ef, 0.02, view=view, queries=queries, allow=allow, eps=eps)
        fc.assert_matches(got, want, ("eps", k, ef))
        assert any(list(r["ids"]).count(5) == 2 for r in want)


@pytest.mark.parametrize("dim", [64, 960])
def test_forced_spill(native, orc, dim):
    """A 256-slot visited table: every query visits more ids than it holds and spills to the bitset."""
    base, queries, arrays = fc.graph(orc, dim, 0)
    dev = dc.device_of(native, base, arrays)
    dev.set_hash_log2(8)
    want = fc.replays(orc, dim, 0, "gist", 10, 40, 0.1)
    assert min(r["counters"][0] for r in want) > 256  # (the table spills at half full or sooner)
    got = dev.filtered_search(queries, 10, 40, _words(fc.mask(fc.N, 0.1), fc.N))
    assert dev.last_plan()["hash_log2"] == 8
    fc.assert_matches(got, want, ("spill", dim))


def test_two_workgroups_run_the_whole_batch(native, orc, monkeypatch):
    """ALAYA_FILTER_GRID=2 with the 2000 base rows as queries: each wave runs about a thousand queries in
    sequence, resetting its result pool in between."""
    base, _, arrays = fc.graph(orc, 64, 0)
    dev = _device(native, orc, 64, 0)
    allow = fc.mask(fc.N, 0.1)
    monkeypatch.setenv("ALAYA_FILTER_GRID", "2")
    got = dev.filtered_search(base, 10, 16, _words(allow, fc.N))
    groups, waves = dev.last_launch()
    assert groups == 2 and groups * waves * 100 <= len(base), (groups, waves)
    view = dc.view_of(orc, base, arrays)
    want = fc.replays(orc, 64, 0, "base", 10, 16, 0.1, view=view, queries=base, allow=allow)
    fc.assert_matches(got, want, "grid 2")


def test_refusals(native, orc):
    base, queries, arrays = fc.graph(orc, 64, 0)
    words = _words(fc.mask(fc.N, 0.1), fc.N)
    dev = _device(native, orc, 64, 0)
    with pytest.raises(ValueError, match="1..224"):
        dev.filtered_search(queries, 225, 40, words)
    with pytest.raises(ValueError):
        dev.filtered_search(queries, 0, 40, words)
    with pytest.raises(ValueError, match="ef"):
        dev.filtered_search(queries, 10, 0, words)
    with pytest.raises(ValueError):
        dev.filtered_search(queries, 10, 40, words[:, :-1])
    with pytest.raises(ValueError):
        dev.filtered_search(queries, 10, 40, np.concatenate([words, words]))  # two masks, no indices
    with pytest.raises(ValueError):
        dev.filtered_search(queries, 10, 40, words, np.ones(len(queries), np.uint32))  # index past n_masks
    sq = dc.device_of(native, base, arrays)
    mn, mx = native.sq8_train(base)
    sq.set_sq8(native.sq8_encode(base, mn, mx, 1), mn, mx, native.host_sq8_order())
    with pytest.raises(ValueError, match="SQ8"):
        sq.filtered_search(queries, 10, 40, words)
