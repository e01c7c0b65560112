"""The filtered SQ8 search on the device (filtered_sq8_search_kernel, then rerank_kernel) against its
restatement (tests/filter_sq8_common.py): ids, distance bits and the four counters equal for every query, none
left out.  test_filter_sq8_host.py pins the restatement and that these inputs reach the paths.

Each case is 2000 rows and at most 12 queries, except the ALAYA_FILTER_GRID case, whose queries are the 2000
base rows so that every wave of two 4-wave workgroups runs hundreds of queries on one candidate pool."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import filter_sq8_common as sc

pytestmark = pytest.mark.gpu

# (k, ef, m, share); m = 0: the default, checked against min(224, max(k, ef))
KEFS = [(10, 40, 40, 0.1), (10, 40, 10, 0.1), (10, 40, 224, 0.5), (5, 1, 5, 1.0), (10, 40, 40, 0.02), (1, 40, 1, 0.1),
        (65, 10, 224, 0.5), (10, 40, 0, 0.1)]
SHAPES = [(64, 0), (100, 0), (7, 0), (128, 1), (768, 1), (960, 0)]  # chunks 0 (runtime d), 4, 24 and 30
_devices = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("ALAYA_FILTER_GRID", "ALAYA_SEARCH_WAVES", "ALAYA_VIS_LIMIT", "ALAYA_VIS_LIMIT_PCT", "ALAYA_SPILL_TABLE",
                 "ALAYA_SPILL_FLAGS", "ALAYA_DIRTY_CAP"):
        monkeypatch.delenv(name, raising=False)


def _words(allow, n=fc.N):
    from alayalite_amd.utils import pack_allow

    return pack_allow(allow, n)


def _new_device(native, orc, dim, metric, kind, order, valid=None):
    base, _, arrays, (mn, mx, codes) = sc.inputs(orc, dim, metric, kind)
    dev = native.DeviceIndex(0)
    dev.set_base(base, metric, valid)
    dev.set_graph(dc.graph_of(native, arrays))
    dev.set_sq8(codes, mn, mx, order)
    return dev


def _device(native, orc, dim, metric, kind, order):
    key = (dim, metric, kind, order)
    if key not in _devices:
        _devices[key] = _new_device(native, orc, dim, metric, kind, order)
    return _devices[key]


@pytest.mark.parametrize("k,ef,m,share", KEFS)
@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("dim,metric", SHAPES)
def test_main_grid(native, orc, dim, metric, order, k, ef, m, share):
    queries = sc.inputs(orc, dim, metric)[1]
    dev = _device(native, orc, dim, metric, "gist", order)
    got = dev.filtered_search_sq8(queries, k, ef, _words(fc.mask(fc.N, share)), None, m)
    want = sc.replays(orc, dim, metric, "gist", order, k, ef, m if m else sc.default_pool(k, ef), share)
    sc.assert_matches(got, want, (dim, metric, order, k, ef, m, share))


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("k,ef,m,share", [(10, 40, 40, 0.1), (10, 40, 10, 0.1), (10, 40, 224, 0.5)])
def test_coarse_codes(native, orc, order, k, ef, m, share):
    queries = sc.inputs(orc, 64, 0, "coarse")[1]
    dev = _device(native, orc, 64, 0, "coarse", order)
    got = dev.filtered_search_sq8(queries, k, ef, _words(fc.mask(fc.N, share)), None, m)
    sc.assert_matches(got, sc.replays(orc, 64, 0, "coarse", order, k, ef, m, share), ("coarse", order, k, ef, m, share))


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("dim", [16, 128])
def test_tie_rows(native, orc, dim, order):
    queries = sc.inputs(orc, dim, 0, "tie")[1]
    dev = _device(native, orc, dim, 0, "tie", order)
    got = dev.filtered_search_sq8(queries, 10, 20, _words(fc.mask(fc.N, 0.3)), None, 40)
    sc.assert_matches(got, sc.replays(orc, dim, 0, "tie", order, 10, 20, 40, 0.3), ("tie", dim, order))


@pytest.mark.parametrize("dim,metric,order", [(64, 0, 2), (128, 1, 1), (768, 1, 2)])
def test_all_zero_mask(native, orc, dim, metric, order):
    """Every slot empty; the counters are the unfiltered SQ8 search's."""
    queries = sc.inputs(orc, dim, metric)[1]
    dev = _device(native, orc, dim, metric, "gist", order)
    ids, d, cnt = dev.filtered_search_sq8(queries, 10, 40, _words(np.zeros(fc.N, bool)))
    assert (ids == sc.EMPTY).all() and (d == sc.FLT_MAX).all()
    sc.assert_matches((ids, d, cnt), sc.replays(orc, dim, metric, "gist", order, 10, 40, 40, 0.0), "zero")
    assert np.array_equal(cnt, dev.search_sq8(queries, 10, 40, 0)[2])


@pytest.mark.parametrize("dim,metric,order", [(64, 0, 2), (768, 1, 2), (100, 0, 1)])
def test_three_masks_in_one_batch(native, orc, dim, metric, order):
    queries = sc.inputs(orc, dim, metric)[1]
    dev = _device(native, orc, dim, metric, "gist", order)
    shares = (0.1, 0.5, 0.02)
    groups = np.arange(len(queries)) % 3
    words = _words(np.stack([fc.mask(fc.N, s) for s in shares]))
    got = dev.filtered_search_sq8(queries, 10, 40, words, groups.astype(np.uint32), 40)
    want = [sc.replays(orc, dim, metric, "gist", order, 10, 40, 40, shares[g])[i] for i, g in enumerate(groups)]
    sc.assert_matches(got, want, "three masks")


@pytest.mark.parametrize("order", [2, 1])
def test_removed_rows_never_come_back(native, orc, order):
    """A validity bitmap (set_base(rows, metric, valid)) removes the rows the first filtered search returned
    while the mask still allows them: they are traversed as before (the counters do not move) and never
    offered to the candidate pool."""
    base, queries, arrays, quant = sc.inputs(orc, 64, 0)
    allow = fc.mask(fc.N, 0.1)
    words = _words(allow)
    first = _device(native, orc, 64, 0, "gist", order).filtered_search_sq8(queries, 10, 40, words, None, 40)
    removed = sorted({int(v) for v in first[0][:, :3].ravel() if v != sc.EMPTY})
    assert len(removed) >= 12 and allow[removed].all()
    valid = np.full((fc.N + 7) // 8, 0xFF, np.uint8)
    for v in removed:
        valid[v >> 3] &= ~np.uint8(1 << (v & 7))
    dev = _new_device(native, orc, 64, 0, "gist", order, valid)
    ids, d, cnt = dev.filtered_search_sq8(queries, 10, 40, words, None, 40)
    assert not np.isin(ids, removed).any()
    assert np.array_equal(cnt, first[2])
    view = dc.view_of(orc, base, arrays, 0, valid=valid)
    want = [sc.replay(orc, view, quant, order, q, 10, 40, 40, allow, 0) for q in queries]
    sc.assert_matches((ids, d, cnt), want, ("removed", order))


@pytest.mark.parametrize("dim,metric,order,table", [(64, 0, 1, None), (64, 0, 2, None), (768, 1, 2, None), (768, 1, 2, "6"),
                                                    (960, 0, 2, "9")])
def test_forced_spill(native, orc, monkeypatch, dim, metric, order, table):
    """A 256-slot first level: every query visits more ids than it holds and spills -- order 1 to the bitset,
    order 2 to the spill table (test_sq8_spill.py's forcing: tables of 64 / 512 entries fill their buckets, so
    many ids take the bitset third level).  Twice on the same slots: a slot left dirty would show."""
    if table is not None:
        monkeypatch.setenv("ALAYA_SPILL_TABLE", table)
    queries = sc.inputs(orc, dim, metric)[1]
    dev = _new_device(native, orc, dim, metric, "gist", order)
    dev.set_hash_log2(8)
    want = sc.replays(orc, dim, metric, "gist", order, 10, 40, 40, 0.1)
    assert min(r["counters"][0] for r in want) > 256  # (the table spills at half full or sooner)
    for rep in range(2):
        got = dev.filtered_search_sq8(queries, 10, 40, _words(fc.mask(fc.N, 0.1)), None, 40)
        assert dev.last_plan()["hash_log2"] == 8
        sc.assert_matches(got, want, ("spill", dim, order, table, rep))


@pytest.mark.parametrize("order", [2, 1])
def test_two_workgroups_run_the_whole_batch(native, orc, monkeypatch, order):
    """ALAYA_FILTER_GRID=2 with the 2000 base rows as queries, ef 16: each of the eight waves runs hundreds of
    queries in sequence, resetting its candidate pool in between."""
    base, _, arrays, quant = sc.inputs(orc, 64, 0)
    dev = _device(native, orc, 64, 0, "gist", order)
    allow = fc.mask(fc.N, 0.1)
    monkeypatch.setenv("ALAYA_FILTER_GRID", "2")
    got = dev.filtered_search_sq8(base, 10, 16, _words(allow), None, 16)
    groups, waves = dev.last_launch()
    assert groups == 2 and waves == 4, (groups, waves)
    view = dc.view_of(orc, base, arrays, 0)
    want = [sc.replay(orc, view, quant, order, q, 10, 16, 16, allow, 0) for q in base]
    sc.assert_matches(got, want, ("grid 2", order))


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("nq", [1, 2, 3])
def test_small_batches(native, orc, order, nq):
    """1, 2 or 3 queries: the workgroup is narrower than four waves, or some waves draw no query -- they
    still pass the workgroup's barrier."""
    queries = sc.inputs(orc, 100, 0)[1]
    dev = _device(native, orc, 100, 0, "gist", order)
    got = dev.filtered_search_sq8(queries[:nq], 10, 40, _words(fc.mask(fc.N, 0.1)), None, 40)
    sc.assert_matches(got, sc.replays(orc, 100, 0, "gist", order, 10, 40, 40, 0.1)[:nq], ("small", nq, order))


def test_refusals(native, orc):
    base, queries, arrays, _ = sc.inputs(orc, 64, 0)
    words = _words(fc.mask(fc.N, 0.1))
    dev = _device(native, orc, 64, 0, "gist", 2)
    with pytest.raises(ValueError, match="pool"):
        dev.filtered_search_sq8(queries, 10, 40, words, None, 9)  # pool < k
    with pytest.raises(ValueError, match="1..224"):
        dev.filtered_search_sq8(queries, 10, 40, words, None, 225)
    with pytest.raises(ValueError, match="1..224"):
        dev.filtered_search_sq8(queries, 225, 40, words)
    with pytest.raises(ValueError):
        dev.filtered_search_sq8(queries, 0, 40, words)
    with pytest.raises(ValueError, match="ef"):
        dev.filtered_search_sq8(queries, 10, 0, words)
    with pytest.raises(ValueError):
        dev.filtered_search_sq8(queries, 10, 40, words[:, :-1])
    with pytest.raises(ValueError):
        dev.filtered_search_sq8(queries, 10, 40, np.concatenate([words, words]))  # two masks, no indices
    plain = dc.device_of(native, base, arrays)
    with pytest.raises(ValueError, match="no SQ8 codes"):
        plain.filtered_search_sq8(queries, 10, 40, words)
    with pytest.raises(ValueError, match="SQ8"):
        dev.filtered_search(queries, 10, 40, words)  # the f32 entry point still refuses an SQ8 index


@pytest.mark.parametrize("metric,id_type", [("l2", np.uint32), ("ip", np.uint64), ("cosine", np.uint32)])
def test_index_api(native, orc, metric, id_type, tmp_path):
    """Index.filtered_search on an SQ8 index: the traversal encodes the query as given, the rerank takes the
    normalised one for COS -- batch_search's two forms (test_sq8.py::test_sq8_index_api builds the same view)."""
    import alayalite_amd

    rng = np.random.default_rng(7)
    base = rng.standard_normal((fc.N, 64)).astype(np.float32)
    queries = rng.standard_normal((fc.NQ, 64)).astype(np.float32)
    client = alayalite_amd.Client(str(tmp_path))
    index = client.create_index("fsq", capacity=fc.N, quantization_type="sq8", metric=metric, id_type=id_type)
    index.fit(base.copy())
    m = {"l2": 0, "ip": 1, "cosine": 2}[metric]
    fb = np.stack([orc.normalize(r) for r in base]) if m == 2 else base
    fq = np.stack([orc.normalize(r) for r in queries]) if m == 2 else queries
    mn, mx = orc.sq8_fit(fb)
    quant = (mn, mx, orc.sq8_encode(fb, mn, mx))
    order = native.host_sq8_order()
    allow = fc.mask(fc.N, 0.02)
    allow[allow.nonzero()[0][30:]] = False  # 30 rows allowed: some queries come up short of k

    def check(idx, pool, m_eff):
        l0, levels, off, ue, ep, ur, _ = idx.native().graph_arrays()  # (the index's own graph, as it stands)
        view = orc.IndexView(fb, l0, levels, off, ue, ur, ep, metric=m)
        ids, d = idx.filtered_search(queries.copy(), 10, 40, allow=allow, rerank_pool=pool)
        assert ids.dtype == id_type and ids.shape == (fc.NQ, 10)
        empty = ids == np.iinfo(id_type).max
        ids32 = np.where(empty, sc.EMPTY, ids).astype(np.uint32)
        want = [sc.replay(orc, view, quant, order, queries[i], 10, 40, m_eff, allow, m, rq=fq[i]) for i in range(fc.NQ)]
        sc.assert_matches((ids32, d, idx.native().last_counters()), want, (metric, pool))
        return ids, d

    ids, d = check(index, None, 40)
    assert (ids == np.iinfo(id_type).max).any() and (ids != np.iinfo(id_type).max).any()
    check(index, 10, 10)
    client.save_index("fsq")
    again = alayalite_amd.Client(str(tmp_path)).get_index("fsq")
    check(again, None, 40)  # the loaded index equals the restatement on the graph it loaded


def test_rerank_pool_needs_an_sq8_index(native):
    import alayalite_amd

    base, queries = dc.rows(64)
    idx = alayalite_amd.Client().create_index("fsq_plain", capacity=fc.N)
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    with pytest.raises(ValueError):
        idx.filtered_search(queries.copy(), 10, 40, allow=fc.mask(fc.N, 0.1), rerank_pool=40)
