"""The range search of an SQ8 index on the device (range_sq8_search_kernel, range_rerank_kernel, then
range_sort_kernel) against its restatement (tests/range_sq8_common.py): counts, candidate counts, ids, exact
distance bits, the empty tail and the four counters equal for every query, none left out.
test_range_sq8_host.py pins the restatement and that these inputs reach both disagreements of code and exact
distance.

Each case is 2000 rows and at most 12 queries, except the ALAYA_FILTER_GRID case, whose queries are the 2000
base rows so that every wave of two 4-wave workgroups runs hundreds of queries, resetting its count and region
base in between."""

from collections import Counter

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import filter_sq8_common as sc
import range_sq8_common as rq

pytestmark = pytest.mark.gpu

SHAPES = [(64, 0), (100, 0), (7, 0), (128, 1), (768, 1), (960, 0)]  # chunks 0 (runtime d), 4, 24 and 30
FLT_MAX = sc.FLT_MAX
INF = np.float32(np.inf)
_devices = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("ALAYA_FILTER_GRID", "ALAYA_SEARCH_WAVES", "ALAYA_VIS_LIMIT", "ALAYA_VIS_LIMIT_PCT", "ALAYA_SPILL_TABLE",
                 "ALAYA_SPILL_FLAGS", "ALAYA_DIRTY_CAP", "ALAYA_RANGE_SORT"):
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


def _mth(orc, base, metric, queries, rs, m):
    """Per query, the m-th smallest exact distance among its pairs (the last one when there are fewer; 0 when
    there are none)."""
    out = []
    for q, r in zip(queries, rs):
        n = len(r["pairs"])
        out.append(rq.mth_exact(orc, base, metric, q, r["pairs"], min(m, n)) if n else np.float32(0.0))
    return np.array(out, np.float32)


def _replay_slack(orc, base, metric, queries, rs, radii):
    """Per query, a slack that covers the replay's largest d_code - d_exact over its exact-in rows."""
    return np.array([rq.slack_above(rad, rq.worst_overstatement(orc, base, metric, q, r["pairs"], rad))
                     for q, r, rad in zip(queries, rs, radii)], np.float32)


def _run(orc, dev, base, metric, queries, rs, radii, slack, cap, what, words=None, groups=None, ef=40):
    n = len(rs)
    radii = np.ascontiguousarray(rq.per_query(radii, n))
    c = np.array([rq.code_radius(r, s) for r, s in zip(radii, rq.per_query(slack, n))], np.float32)
    got = dev.range_search_sq8(queries, ef, radii, c, cap, words, groups)
    rq.assert_matches(orc, got, rs, base, metric, queries, radii, c, cap, what)
    return got


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("dim,metric", SHAPES)
def test_main_grid(native, orc, dim, metric, order):
    base, queries, _, _ = sc.inputs(orc, dim, metric)
    rs = rq.replays(orc, dim, metric, "gist", order, 40)
    dev = _device(native, orc, dim, metric, "gist", order)
    what = (dim, metric, order)
    run = lambda radii, slack, cap, tag: _run(orc, dev, base, metric, queries, rs, radii, slack, cap, what + (tag,))  # noqa: E731
    lost = gained = 0
    for m in (1, 17, 64):
        radii = _mth(orc, base, metric, queries, rs, m)
        zero = run(radii, 0.0, 64, ("slack 0", m))
        covered = run(radii, _replay_slack(orc, base, metric, queries, rs, radii), 64, ("replay slack", m))
        run(radii, INF, 64, ("slack inf", m))
        # the replay-derived slack returns every exact-in pair up to the cap: here every query has exactly m
        # (ties aside, at least m) of them and m <= 64
        for i, (q, r) in enumerate(zip(queries, rs)):
            exact_in = sum(e <= radii[i] for e in rq.exact_of(orc, base, metric, q, r["pairs"]))
            assert exact_in >= m
            if covered[4][i] <= 64:
                assert covered[0][i] == exact_in, (what, m, i, covered[0][i], exact_in)
        lost += int((covered[0].astype(np.int64) - zero[0]).clip(min=0).sum())
        gained += int((zero[4].astype(np.int64) - zero[0]).sum())
    assert lost + gained > 0, what  # slack 0 misses rows the slack admits, or the rerank cut removes candidates
    over = run(_mth(orc, base, metric, queries, rs, 65), INF, 64, "m 65")  # the cap is past by one
    assert (over[4] > 64).all() and (over[0] <= 64).all()
    # just below every exact distance: nothing is a hit, candidates remain under a slack
    below = np.nextafter(_mth(orc, base, metric, queries, rs, 1), np.float32(-np.inf))
    none = run(below, 0.0, 64, "below, slack 0")
    some = run(below, INF, 64, "below, slack inf")
    assert (none[0] == 0).all() and (some[0] == 0).all() and (some[4] > 64).all()
    full = run(FLT_MAX, 0.0, 4096, "FLT_MAX, cap 4096")
    assert np.array_equal(full[0], full[4]) and [int(x) for x in full[4]] == [len(r["pairs"]) for r in rs]
    for cap in (1, 2, 63, 64, 65, 100):
        got = run(FLT_MAX, 0.0, cap, ("FLT_MAX", cap))
        assert (got[0] == cap).all()
    radius = float(np.median(_mth(orc, base, metric, queries, rs, 17)))
    run(radius, 0.0, 64, "scalar radius")
    got = dev.range_search_sq8(queries, 40, radius, radius, 64)  # numbers, as given
    rq.assert_matches(orc, got, rs, base, metric, queries, radius, radius, 64, what + ("scalars",))
    radii = _mth(orc, base, metric, queries, rs, 17)
    slack = np.where(np.arange(len(rs)) % 3 == 0, np.float32(0.0),
                     np.where(np.arange(len(rs)) % 3 == 1, _replay_slack(orc, base, metric, queries, rs, radii), INF))
    run(radii, slack.astype(np.float32), 64, "per-query slack")


@pytest.mark.parametrize("order", [2, 1])
def test_coarse_codes(native, orc, order):
    """Coarse codes: the code radius lets rows in that the rerank cut removes."""
    base, queries, _, _ = sc.inputs(orc, 64, 0, "coarse")
    rs = rq.replays(orc, 64, 0, "coarse", order, 40)
    dev = _device(native, orc, 64, 0, "coarse", order)
    removed = 0
    for m in (17, 64):
        radii = _mth(orc, base, 0, queries, rs, m)
        got = _run(orc, dev, base, 0, queries, rs, radii, 0.0, 4096, ("coarse", order, m))
        removed += int((got[4].astype(np.int64) - got[0]).sum())
        _run(orc, dev, base, 0, queries, rs, radii, INF, 64, ("coarse inf", order, m))
    assert removed == 75 + 259  # test_range_sq8_host.py's figures


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("dim", [16, 128])
def test_tie_rows(native, orc, dim, order):
    """The radius at the exact distance most of a query's pairs tie at: ids ascend inside a tie."""
    base, queries, _, _ = sc.inputs(orc, dim, 0, "tie")
    rs = rq.replays(orc, dim, 0, "tie", order, 20)
    dev = _device(native, orc, dim, 0, "tie", order)
    radii, ties = [], []
    for q, r in zip(queries, rs):
        d, n = Counter(float(e) for e in rq.exact_of(orc, base, 0, q, r["pairs"])).most_common(1)[0]
        radii.append(d)
        ties.append(n)
    assert min(ties) >= 3, ties
    radii = np.array(radii, np.float32)
    for slack, cap in ((0.0, 1024), (INF, 1024), (INF, 64)):
        counts, ids, d, _, _ = _run(orc, dev, base, 0, queries, rs, radii, slack, cap, ("tie", dim, order, slack, cap), ef=20)
        for i in range(len(rs)):
            row_i, row_d = ids[i][:counts[i]].astype(np.int64), d[i][:counts[i]]
            assert (np.diff(row_d) >= 0).all() and (np.diff(row_i)[np.diff(row_d) == 0] > 0).all(), (dim, order, i)
    assert (counts > 1).any()


@pytest.mark.parametrize("dim,metric,order", [(64, 0, 2), (768, 1, 2), (100, 0, 1)])
def test_masks(native, orc, dim, metric, order):
    base, queries, _, _ = sc.inputs(orc, dim, metric)
    dev = _device(native, orc, dim, metric, "gist", order)
    shares = (0.1, 0.02, 1.0)
    per_share = {s: rq.replays(orc, dim, metric, "gist", order, 40, s) for s in shares + (0.0,)}
    for s in (0.1, 0.02):
        rs = per_share[s]
        for m, slack in ((5, 0.0), (17, INF)):
            _run(orc, dev, base, metric, queries, rs, _mth(orc, base, metric, queries, rs, m), slack, 64,
                 ("share", s, m), _words(fc.mask(fc.N, s)))
        _run(orc, dev, base, metric, queries, rs, FLT_MAX, 0.0, 4096, ("share", s, "all"), _words(fc.mask(fc.N, s)))
    # three masks in one batch
    groups = np.arange(len(queries)) % 3
    rs = [per_share[shares[g]][i] for i, g in enumerate(groups)]
    words = _words(np.stack([fc.mask(fc.N, s) for s in shares]))
    for slack in (0.0, INF):
        _run(orc, dev, base, metric, queries, rs, _mth(orc, base, metric, queries, rs, 9), slack, 64, "three masks", words,
             groups.astype(np.uint32))
    # an all-zero mask: no candidate whatever the radii; the counters are the unfiltered SQ8 search's
    got = _run(orc, dev, base, metric, queries, per_share[0.0], FLT_MAX, INF, 64, "zero mask", _words(np.zeros(fc.N, bool)))
    assert (got[0] == 0).all() and (got[4] == 0).all() and (got[1] == sc.EMPTY).all() and (got[2] == FLT_MAX).all()
    assert np.array_equal(got[3], dev.search_sq8(queries, 10, 40, 0)[2])
    # no mask equals the all-ones mask
    rs = per_share[1.0]
    radii = _mth(orc, base, metric, queries, rs, 17)
    a = _run(orc, dev, base, metric, queries, rs, radii, INF, 64, "no mask")
    b = _run(orc, dev, base, metric, queries, rs, radii, INF, 64, "ones mask", _words(np.ones(fc.N, bool)))
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("order", [2, 1])
def test_removed_rows_are_never_candidates(native, orc, order):
    """A validity bitmap removes rows the first call returned: they are traversed as before (the counters do
    not move) and are never candidates, whatever the radii."""
    base, queries, arrays, quant = sc.inputs(orc, 64, 0)
    rs = rq.replays(orc, 64, 0, "gist", order, 40)
    radii = _mth(orc, base, 0, queries, rs, 17)
    first = _run(orc, _device(native, orc, 64, 0, "gist", order), base, 0, queries, rs, radii, INF, 64, "before")
    removed = sorted({int(v) for v in first[1][:, :3].ravel() if v != sc.EMPTY})
    assert len(removed) >= 12
    valid = np.full((fc.N + 7) // 8, 0xFF, np.uint8)
    for v in removed:
        valid[v >> 3] &= ~np.uint8(1 << (v & 7))
    dev = _new_device(native, orc, 64, 0, "gist", order, valid)
    view = dc.view_of(orc, base, arrays, 0, valid=valid)
    want = [rq.replay(orc, view, quant, order, q, 40, np.ones(fc.N, bool), 0) for q in queries]
    for rad, slack, cap in ((radii, INF, 64), (radii, 0.0, 64), (FLT_MAX, INF, 4096)):
        got = _run(orc, dev, base, 0, queries, want, rad, slack, cap, ("removed", order, cap))
        assert not np.isin(got[1], removed).any()
        assert np.array_equal(got[3], first[3])
    assert [int(x) for x in got[4]] == [len(r["pairs"]) for r in want]
    assert sum(len(r["pairs"]) for r in want) < sum(len(r["pairs"]) for r in rs)


@pytest.mark.parametrize("dim,metric,order,table", [(64, 0, 1, None), (64, 0, 2, None), (768, 1, 2, None), (768, 1, 2, "6"),
                                                    (960, 0, 2, "9")])
def test_forced_spill(native, orc, monkeypatch, dim, metric, order, table):
    """A 256-slot first level: every query visits more ids than it holds and spills -- order 1 to the bitset,
    order 2 to the spill table (tables of 64 / 512 entries fill their buckets, so many ids take the bitset third
    level).  Twice on the same slots: a slot left dirty would show."""
    if table is not None:
        monkeypatch.setenv("ALAYA_SPILL_TABLE", table)
    base, queries, _, _ = sc.inputs(orc, dim, metric)
    dev = _new_device(native, orc, dim, metric, "gist", order)
    dev.set_hash_log2(8)
    rs = rq.replays(orc, dim, metric, "gist", order, 40)
    assert min(r["counters"][0] for r in rs) > 256  # (the table spills at half full or sooner)
    radii = _mth(orc, base, metric, queries, rs, 64)
    for rep in range(2):
        _run(orc, dev, base, metric, queries, rs, radii, INF, 64, ("spill", dim, order, table, rep))
        assert dev.last_plan()["hash_log2"] == 8
        _run(orc, dev, base, metric, queries, rs, FLT_MAX, 0.0, 4096, ("spill all", dim, order, table, rep))


@pytest.mark.parametrize("order", [2, 1])
def test_two_workgroups_run_the_whole_batch(native, orc, monkeypatch, order):
    """ALAYA_FILTER_GRID=2 with the 2000 base rows as queries, ef 16: each of the eight waves runs hundreds of
    queries in sequence; the count and the region base reset between a wave's queries."""
    base, _, arrays, quant = sc.inputs(orc, 64, 0)
    dev = _device(native, orc, 64, 0, "gist", order)
    view = dc.view_of(orc, base, arrays, 0)
    allow = np.ones(fc.N, bool)
    want = [rq.replay(orc, view, quant, order, q, 16, allow, 0) for q in base]
    # (query i's radius is its (1 + i % 24)-th smallest code distance, so the lists differ in length from one
    # query of a wave to the next, and only the stored candidates are measured exactly here)
    radii = np.array([sorted(np.float32(d) for _, d in r["pairs"])[i % 24] for i, r in enumerate(want)], np.float32)
    monkeypatch.setenv("ALAYA_FILTER_GRID", "2")
    got = _run(orc, dev, base, 0, base, want, radii, 0.0, 32, ("grid 2", order), ef=16)
    groups, waves = dev.last_launch()
    assert groups == 2 and waves == 4, (groups, waves)
    assert len(set(int(x) for x in got[4])) > 3 and len(set(int(x) for x in got[0])) > 3


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("nq", [1, 2, 3])
def test_small_batches(native, orc, order, nq):
    """1, 2 or 3 queries: the workgroup is narrower than four waves, or some waves draw no query -- they still
    pass the workgroup's barrier."""
    base, queries, _, _ = sc.inputs(orc, 100, 0)
    dev = _device(native, orc, 100, 0, "gist", order)
    rs = rq.replays(orc, 100, 0, "gist", order, 40)[:nq]
    radii = _mth(orc, base, 0, queries[:nq], rs, 17)
    _run(orc, dev, base, 0, queries[:nq], rs, radii, INF, 64, ("small", nq, order))


@pytest.mark.parametrize("dim,metric,order", [(64, 0, 2), (128, 1, 1), (768, 1, 2)])
def test_agrees_with_its_neighbours(native, orc, dim, metric, order):
    """The counters are search_sq8's at the same ef; at radius FLT_MAX the candidate id set is the pairs of the
    filtered SQ8 replay (the allowed, valid rows the traversal measured)."""
    base, queries, _, _ = sc.inputs(orc, dim, metric)
    dev = _device(native, orc, dim, metric, "gist", order)
    for share in (1.0, 0.1):
        rs = sc.replays(orc, dim, metric, "gist", order, 10, 40, 40, share)
        words = None if share == 1.0 else _words(fc.mask(fc.N, share))
        counts, ids, d, cnt, cand = dev.range_search_sq8(queries, 40, FLT_MAX, FLT_MAX, 4096, words)
        assert np.array_equal(cnt, dev.search_sq8(queries, 10, 40, 0)[2])
        for i, r in enumerate(rs):
            assert counts[i] == cand[i] == len(r["pairs"])
            assert sorted(ids[i][:counts[i]].tolist()) == sorted(v for v, _ in r["pairs"]), (dim, metric, order, i)


def test_rerank_queries_are_the_exact_side(native, orc):
    """The traversal encodes `queries`; the exact distance and the radius cut take `rerank_queries`."""
    base, queries, _, _ = sc.inputs(orc, 64, 1)
    dev = _device(native, orc, 64, 1, "gist", 2)
    rs = rq.replays(orc, 64, 1, "gist", 2, 40)
    rqs = np.ascontiguousarray(queries * np.float32(0.5))
    radii = _mth(orc, base, 1, rqs, rs, 17)
    c = np.full(len(rs), INF, np.float32)
    got = dev.range_search_sq8(queries, 40, radii, c, 64, None, None, rqs)
    rq.assert_matches(orc, got, rs, base, 1, rqs, radii, c, 64, "rerank queries")


def test_sort_switch_runs_the_stages_alone(native, orc, monkeypatch):
    base, queries, _, _ = sc.inputs(orc, 64, 0)
    dev = _device(native, orc, 64, 0, "gist", 2)
    rs = rq.replays(orc, 64, 0, "gist", 2, 40)
    monkeypatch.setenv("ALAYA_RANGE_SORT", "0")
    counts, _, _, cnt, cand = dev.range_search_sq8(queries, 40, FLT_MAX, FLT_MAX, 64)
    assert (counts == 0).all() and [int(x) for x in cand] == [len(r["pairs"]) for r in rs]
    assert [tuple(int(x) for x in row) for row in cnt] == [tuple(r["counters"]) for r in rs]
    # 2: the search and the rerank without the sort -- the counts are the hits' as well
    monkeypatch.setenv("ALAYA_RANGE_SORT", "2")
    radii = _mth(orc, base, 0, queries, rs, 17)
    counts, _, _, cnt, cand = dev.range_search_sq8(queries, 40, radii, np.full(len(rs), INF, np.float32), 64)
    want = [rq.want_row(orc, base, 0, q, r["pairs"], rad, INF, 64) for q, r, rad in zip(queries, rs, radii)]
    assert [int(x) for x in counts] == [w[0] for w in want] and [int(x) for x in cand] == [w[1] for w in want]
    assert [tuple(int(x) for x in row) for row in cnt] == [tuple(r["counters"]) for r in rs]


def test_refusals(native, orc):
    import alayalite_amd

    base, queries, arrays, _ = sc.inputs(orc, 64, 0)
    words = _words(fc.mask(fc.N, 0.1))
    dev = _device(native, orc, 64, 0, "gist", 2)
    nan = np.float32(np.nan)
    with pytest.raises(ValueError, match="max_results"):
        dev.range_search_sq8(queries, 40, 1.0, 1.0, 0)
    with pytest.raises(ValueError, match="max_results"):
        dev.range_search_sq8(queries, 40, 1.0, 1.0, 4097)
    with pytest.raises(ValueError, match="ef"):
        dev.range_search_sq8(queries, 0, 1.0, 1.0, 64)
    with pytest.raises(ValueError, match="NaN"):
        dev.range_search_sq8(queries, 40, nan, 1.0, 64)
    with pytest.raises(ValueError, match="NaN"):
        dev.range_search_sq8(queries, 40, 1.0, np.where(np.arange(len(queries)) == 5, nan, 1.0).astype(np.float32), 64)
    with pytest.raises(ValueError):
        dev.range_search_sq8(queries, 40, np.ones(len(queries) - 1, np.float32), 1.0, 64)
    with pytest.raises(ValueError):
        dev.range_search_sq8(queries, 40, 1.0, 1.0, 64, words[:, :-1])  # a short mask
    with pytest.raises(ValueError):
        dev.range_search_sq8(queries, 40, 1.0, 1.0, 64, np.concatenate([words, words]))  # two masks, no indices
    with pytest.raises(ValueError):
        dev.range_search_sq8(queries, 40, 1.0, 1.0, 64, None, np.zeros(len(queries), np.uint32))  # indices without masks
    plain = dc.device_of(native, base, arrays)
    with pytest.raises(ValueError, match="no SQ8 codes"):
        plain.range_search_sq8(queries, 40, 1.0, 1.0, 64)
    with pytest.raises(ValueError, match="SQ8"):
        dev.range_search(queries, 40, 1.0, 64)  # the f32 entry still refuses an SQ8 index
    # the Index layer
    client = alayalite_amd.Client()
    f32 = client.create_index("rsq_plain", capacity=fc.N)
    f32.fit(base.copy(), ef_construction=100, num_threads=1)
    with pytest.raises(ValueError, match="slack"):
        f32.range_search(queries.copy(), 1.0, 40, 64, slack=0.0)
    sq = client.create_index("rsq_sq8", capacity=fc.N, quantization_type="sq8")
    sq.fit(base.copy(), ef_construction=100, num_threads=1)
    with pytest.raises(ValueError, match="SQ8"):
        sq.range_search(queries.copy(), 1.0, 40, 64, expand="radius", slack=0.0)
    with pytest.raises(ValueError, match="SQ8.*slack="):
        sq.range_search(queries.copy(), 1.0, 40, 64)
    with pytest.raises(ValueError, match="slack"):
        sq.range_search(queries.copy(), 1.0, 40, 64, slack=-1.0)
    with pytest.raises(ValueError, match="slack"):
        sq.range_search(queries.copy(), 1.0, 40, 64, slack=np.nan)
    with pytest.raises(ValueError, match="slack"):
        sq.range_search(queries.copy(), 1.0, 40, 64, slack=np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="NaN"):
        sq.range_search(queries.copy(), np.nan, 40, 64, slack=0.0)
    with pytest.raises(ValueError, match="NaN"):
        sq.range_search(queries.copy(), -np.inf, 40, 64, slack=np.inf)
    for cap in (0, 4097):
        with pytest.raises(ValueError, match="max_results"):
            sq.range_search(queries.copy(), 1.0, 40, cap, slack=0.0)
    with pytest.raises(ValueError, match="ef"):
        sq.range_search(queries.copy(), 1.0, 0, 64, slack=0.0)


@pytest.mark.parametrize("metric,id_type", [("l2", np.uint32), ("ip", np.uint64), ("cosine", np.uint32)])
def test_index_api(native, orc, metric, id_type, tmp_path):
    """Index.range_search(slack=) on an SQ8 index against the restatement on the index's own graph and
    quantizer: the traversal encodes the query as given, the rerank takes the normalised one for COS."""
    import alayalite_amd

    rng = np.random.default_rng(7)
    base = rng.standard_normal((fc.N, 64)).astype(np.float32)
    queries = rng.standard_normal((fc.NQ, 64)).astype(np.float32)
    client = alayalite_amd.Client(str(tmp_path))
    index = client.create_index("rsq", capacity=fc.N, quantization_type="sq8", metric=metric, id_type=id_type)
    index.fit(base.copy())
    m = {"l2": 0, "ip": 1, "cosine": 2}[metric]
    fb = np.stack([orc.normalize(r) for r in base]) if m == 2 else base
    fq = np.stack([orc.normalize(r) for r in queries]) if m == 2 else queries
    mn, mx = orc.sq8_fit(fb)
    quant = (mn, mx, orc.sq8_encode(fb, mn, mx))
    order = native.host_sq8_order()
    allow = fc.mask(fc.N, 0.5)
    empty = np.iinfo(id_type).max

    def check(idx, allow_, radius_m, slack, cap, chunk=None):
        l0, levels, off, ue, ep, ur, _ = idx.native().graph_arrays()  # (the index's own graph, as it stands)
        view = orc.IndexView(fb, l0, levels, off, ue, ur, ep, metric=m)
        mask = np.ones(fc.N, bool) if allow_ is None else allow_
        rs = [rq.replay(orc, view, quant, order, queries[i], 40, mask, m, rq=fq[i]) for i in range(fc.NQ)]
        radii = _mth(orc, fb, m, fq, rs, radius_m)
        slacks = rq.per_query(slack, fc.NQ)
        c = np.array([rq.code_radius(r, s) for r, s in zip(radii, slacks)], np.float32)
        lims, ids, d, counts = idx.range_search(queries.copy(), radii, 40, cap, allow=allow_, slack=slack, _chunk=chunk)
        cand = idx.native().last_range_candidates()
        assert ids.dtype == id_type and d.dtype == np.float32 and counts.dtype == np.uint32 and lims.dtype == np.int64
        assert cand.dtype == np.uint32 and cand.shape == (fc.NQ,)
        assert lims[0] == 0 and lims[-1] == len(ids) == len(d) and np.array_equal(np.diff(lims), counts)
        assert not (ids == empty).any()
        pad_i = np.full((fc.NQ, cap), sc.EMPTY, np.uint32)
        pad_d = np.full((fc.NQ, cap), FLT_MAX, np.float32)
        for i in range(fc.NQ):
            pad_i[i, :counts[i]] = ids[lims[i]:lims[i + 1]]
            pad_d[i, :counts[i]] = d[lims[i]:lims[i + 1]]
        got = (counts, pad_i, pad_d, idx.native().last_counters() if chunk is None else None, cand)
        rq.assert_matches(orc, got, rs, fb, m, fq, radii, c, cap, (metric, radius_m, cap, chunk))
        return lims, ids, d, counts, cand

    one = check(index, None, 17, 0.0, 64)
    assert (one[3] > 0).any()
    check(index, allow, 17, INF, 64)
    trunc = check(index, None, 64, INF, 32)
    assert (trunc[4] > 32).all()  # truncation shows in the candidates
    per_query = np.where(np.arange(fc.NQ) % 2 == 0, np.float32(0.0), INF).astype(np.float32)
    whole = check(index, allow, 17, per_query, 64)
    parts = check(index, allow, 17, per_query, 64, chunk=5)
    for a, b in zip(whole, parts):
        assert np.array_equal(a, b)
    client.save_index("rsq")
    again = alayalite_amd.Client(str(tmp_path)).get_index("rsq")
    check(again, allow, 17, INF, 64)  # the loaded index equals the restatement on the graph it loaded
