"""The three filtered graph searches on the device (filtered_search_kernel, filtered_hop_search_kernel,
filtered_sq8_search_kernel) against their restatements at ef above 64 and at d = 256, 512, 768 and 1024: ids,
distance bits, the four counters (and n_through) equal for every query, none left out.

ef selects code and plan, not just size: the traversal merge runs from registers at d = 128 / 256 while
ef <= 128 (its second register half is dead below ef 65) and through LDS otherwise, where the shift loop and
the pop's scan take more than one 64-entry trip only past 64 entries; the visited table's cap and the place of
the result pool move with ef; and the launch is refused when the pools outgrow the LDS.  The case lists are
tests/filter_ef_common.py's; test_filter_ef_host.py asserts that each of them fills its traversal pool and
goes on rejecting, and that the ef 387 cases shift across three trips.

Each case is one launch of at most 12 queries over 2000 rows (48 queries where several run per wave; the
LDS-edge search launches about twenty times)."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import filter_ef_common as ec
import filter_hop_common as hc
import filter_sq8_common as sc

pytestmark = pytest.mark.gpu

LDS_PER_CU = 160 * 1024
_devices = {}
_sq8_devices = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("ALAYA_FILTER_GRID", "ALAYA_SEARCH_WAVES", "ALAYA_VIS_LIMIT", "ALAYA_VIS_LIMIT_PCT", "ALAYA_SPILL_TABLE",
                 "ALAYA_SPILL_FLAGS", "ALAYA_DIRTY_CAP"):
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


def _new_sq8_device(native, orc, dim, metric, order):
    base, _, arrays, (mn, mx, codes) = sc.inputs(orc, dim, metric)
    dev = dc.device_of(native, base, arrays, metric)
    dev.set_sq8(codes, mn, mx, order)
    return dev


def _sq8_device(native, orc, dim, metric, order):
    key = (dim, metric, order)
    if key not in _sq8_devices:
        _sq8_devices[key] = _new_sq8_device(native, orc, dim, metric, order)
    return _sq8_devices[key]


def _plain(native, orc, case):
    dim, metric, kind, k, ef, share = case
    queries = fc.graph(orc, dim, metric, kind)[1]
    dev = _device(native, orc, dim, metric, kind)
    got = dev.filtered_search(queries, k, ef, _words(fc.mask(fc.N, share)))
    fc.assert_matches(got, fc.replays(orc, dim, metric, kind, k, ef, share), case)
    return dev, got


def _through(native, orc, case):
    dim, metric, kind, k, ef, share = case
    queries = fc.graph(orc, dim, metric, kind)[1]
    dev = _device(native, orc, dim, metric, kind)
    got = dev.filtered_search_hop(queries, k, ef, _words(fc.mask(fc.N, share)))
    hc.assert_matches(got, hc.replays(orc, dim, metric, kind, k, ef, share), case)
    return dev, got


# ---- 1, 3: the widths at large ef ------------------------------------------------------------------------
@pytest.mark.parametrize("k,ef,share", ec.PLAIN_KEFS)
@pytest.mark.parametrize("dim,metric", ec.WIDE_SHAPES)
def test_plain_widths(native, orc, dim, metric, k, ef, share):
    _plain(native, orc, (dim, metric, "gist", k, ef, share))


@pytest.mark.parametrize("k,ef,share", ec.HOP_KEFS)
@pytest.mark.parametrize("dim,metric", ec.WIDE_SHAPES)
def test_through_widths(native, orc, dim, metric, k, ef, share):
    _through(native, orc, (dim, metric, "gist", k, ef, share))


def test_through_at_its_measured_configuration(native, orc):
    """d = 960, ef 387, half the rows allowed."""
    _through(native, orc, ec.HOP_ROUND17)


# ---- 2: the register merge's edges -----------------------------------------------------------------------
@pytest.mark.parametrize("ef", ec.MERGE_EFS)
@pytest.mark.parametrize("dim,metric", ec.MERGE_SHAPES)
def test_plain_register_merge_boundary(native, orc, dim, metric, ef):
    _plain(native, orc, (dim, metric, "gist", 10, ef, ec.MERGE_PLAIN_SHARE))


@pytest.mark.parametrize("ef", ec.MERGE_EFS)
@pytest.mark.parametrize("dim,metric", ec.MERGE_SHAPES)
def test_through_register_merge_boundary(native, orc, dim, metric, ef):
    _through(native, orc, (dim, metric, "gist", 10, ef, ec.MERGE_HOP_SHARE))


@pytest.mark.parametrize("search", [_plain, _through], ids=["plain", "through"])
def test_tie_rows_in_both_register_halves(native, orc, search):
    """ef 100 over rows of {0, 1, 2}: equal distances sit in both halves of the two-register merge, which orders
    them by lane; that must be the arrival order."""
    search(native, orc, ec.TIE)


# ---- 4: SQ8 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,ef,m,share", ec.SQ8_KEFS)
@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("dim,metric", ec.SQ8_SHAPES)
def test_sq8_widths(native, orc, dim, metric, order, k, ef, m, share):
    queries = sc.inputs(orc, dim, metric)[1]
    dev = _sq8_device(native, orc, dim, metric, order)
    got = dev.filtered_search_sq8(queries, k, ef, _words(fc.mask(fc.N, share)), None, m)
    sc.assert_matches(got, sc.replays(orc, dim, metric, "gist", order, k, ef, m, share), (dim, metric, order, k, ef, m, share))


@pytest.mark.parametrize("order,table", [(2, None), (2, "6"), (1, None)])
def test_sq8_forced_spill(native, orc, monkeypatch, order, table):
    """test_filter_sq8_gpu.py's forcing at ef 200: a 256-slot first level, so every query spills -- order 2 to
    the spill table, whose size follows ef (table None) or is 64 entries, which fill their buckets and send
    many ids on to the bitset (table "6"); order 1 to the bitset.  Twice on the same slots."""
    dim, metric, _, k, ef, m, share = ec.SQ8_FORCED
    if table is not None:
        monkeypatch.setenv("ALAYA_SPILL_TABLE", table)
    queries = sc.inputs(orc, dim, metric)[1]
    dev = _new_sq8_device(native, orc, dim, metric, order)
    dev.set_hash_log2(8)
    want = sc.replays(orc, dim, metric, "gist", order, k, ef, m, share)
    assert min(r["counters"][0] for r in want) > 256  # (the table spills at half full or sooner)
    for rep in range(2):
        got = dev.filtered_search_sq8(queries, k, ef, _words(fc.mask(fc.N, share)), None, m)
        assert dev.last_plan()["hash_log2"] == 8
        sc.assert_matches(got, want, ("spill", order, table, rep))


# ---- 5: the plan moves with ef -----------------------------------------------------------------------------
@pytest.mark.parametrize("search", [_plain, _through], ids=["plain", "through"])
def test_plan_moves_with_ef(native, orc, search):
    dim, metric, k, small, large, share = ec.PLAN
    plans = []
    for ef in (small, large):
        dev, _ = search(native, orc, (dim, metric, "gist", k, ef, share))
        plans.append(dev.last_plan())
        print("ef", ef, "plan", plans[-1])
    assert (plans[0]["hash_log2"], plans[0]["lds_bytes"]) != (plans[1]["hash_log2"], plans[1]["lds_bytes"]), plans


# ---- 6: ef at and above the row count -------------------------------------------------------------------
@pytest.mark.parametrize("ef", ec.OVER_EFS)
@pytest.mark.parametrize("search", [_plain, _through], ids=["plain", "through"])
def test_ef_at_the_row_count_is_the_exact_scan(native, orc, search, ef):
    """The pool never fills: every reachable row is measured, and the answer is the exact filtered scan's --
    the same ids and, the two kernels summing in the same order over rows without ties, the same distance bits."""
    dim, metric, k, share = ec.OVER
    queries = fc.graph(orc, dim, metric)[1]
    words = _words(fc.mask(fc.N, share))
    dev, got = search(native, orc, (dim, metric, "gist", k, ef, share))
    flat_ids, flat_d = dev.flat_search_filtered(queries, k, words)
    for i in range(len(queries)):
        assert len(set(got[0][i].tolist())) == k
        assert set(got[0][i].tolist()) == set(flat_ids[i].tolist()), (i, got[0][i], flat_ids[i])
        assert np.array_equal(np.sort(got[1][i]).view(np.uint32), np.sort(flat_d[i]).view(np.uint32)), (i, got[1][i], flat_d[i])


# ---- 7: the LDS-budget edge ----------------------------------------------------------------------------------
def _largest_accepted(call):
    """call(ef) -> the search's output.  Doubles ef from 256 to the first refusal, which must be the planner's
    ValueError, then bisects: (the largest accepted ef, its output, launches)."""

    def attempt(ef):
        try:
            return call(ef)
        except ValueError as e:
            assert "LDS budget" in str(e), e
            return None

    lo, launches = 256, 1
    out = attempt(lo)
    assert out is not None
    hi = 2 * lo
    while True:
        assert hi <= 1 << 20, "no refusal"
        launches += 1
        got = attempt(hi)
        if got is None:
            break
        lo, out, hi = hi, got, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        launches += 1
        got = attempt(mid)
        if got is None:
            hi = mid
        else:
            lo, out = mid, got
    return lo, out, launches


@pytest.mark.parametrize("kernel", ["plain", "through", "sq8 order 2", "sq8 order 1"])
def test_lds_budget_edge(native, orc, kernel):
    """The largest ef the planner accepts at d = 1024, k = 224 runs and equals the restatement inside the
    160 KiB of a CU; one more is refused with a ValueError, not by the launch."""
    dim, metric, k, share = ec.EDGE
    queries = fc.graph(orc, dim, metric)[1]
    words = _words(fc.mask(fc.N, share))
    if kernel == "plain":
        dev = _device(native, orc, dim, metric)
        call = lambda e: dev.filtered_search(queries, k, e, words)  # noqa: E731
    elif kernel == "through":
        dev = _device(native, orc, dim, metric)
        call = lambda e: dev.filtered_search_hop(queries, k, e, words)  # noqa: E731
    else:
        order = int(kernel[-1])
        dev = _sq8_device(native, orc, dim, metric, order)
        call = lambda e: dev.filtered_search_sq8(queries, k, e, words, None, k)  # noqa: E731
    ef, _, launches = _largest_accepted(call)
    got = call(ef)  # again, so that the plan read below is this launch's
    plan = dev.last_plan()
    print(kernel, "largest accepted ef:", ef, "launches:", launches + 1, "plan:", plan)
    if kernel == "plain":
        fc.assert_matches(got, fc.replays(orc, dim, metric, "gist", k, ef, share), (kernel, ef))
    elif kernel == "through":
        hc.assert_matches(got, hc.replays(orc, dim, metric, "gist", k, ef, share), (kernel, ef))
    else:
        sc.assert_matches(got, sc.replays(orc, dim, metric, "gist", order, k, ef, k, share), (kernel, ef))
    assert plan["lds_bytes"] <= LDS_PER_CU, plan
    # the edge is the LDS's: four more pool entries per wave (each pool array is a 16-byte multiple) would not fit
    assert plan["lds_bytes"] + 32 * plan["waves_per_group"] > LDS_PER_CU, plan


# ---- 8: several queries per wave ---------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["plain", "through", "sq8"])
def test_several_queries_per_wave(native, orc, monkeypatch, kernel):
    """ALAYA_FILTER_GRID=1, queries = base rows 0..47, ef 200, masks of shares 0.5 and 0.02 by turns: a wave's
    consecutive queries leave very different result pools (and, through, traversal pools) behind."""
    monkeypatch.setenv("ALAYA_FILTER_GRID", "1")
    words = _words(np.stack([fc.mask(fc.N, s) for s in ec.WAVE_SHARES]))
    groups = (np.arange(ec.WAVE_NQ) % 2).astype(np.uint32)
    ef = ec.WAVE_EF
    if kernel == "sq8":
        dim, metric, order = ec.WAVE_SQ8
        queries = sc.inputs(orc, dim, metric)[0][:ec.WAVE_NQ]
        dev = _sq8_device(native, orc, dim, metric, order)
        got = dev.filtered_search_sq8(queries, 10, ef, words, groups, ef)
        assert dev.last_launch()[0] == 1
        sc.assert_matches(got, ec.wave_wants(orc, kernel), kernel)
        return
    dim, metric = ec.WAVE_F32
    queries = fc.graph(orc, dim, metric)[0][:ec.WAVE_NQ]
    dev = _device(native, orc, dim, metric)
    if kernel == "plain":
        got = dev.filtered_search(queries, 10, ef, words, groups)
        assert dev.last_launch()[0] == 1
        fc.assert_matches(got, ec.wave_wants(orc, kernel), kernel)
    else:
        got = dev.filtered_search_hop(queries, 10, ef, words, groups)
        assert dev.last_launch()[0] == 1
        hc.assert_matches(got, ec.wave_wants(orc, kernel), kernel)


# ---- 9: three masks in one batch at ef 387 ----------------------------------------------------------------
def test_plain_three_masks_in_one_batch(native, orc):
    dim, metric, k, ef = ec.THREE
    queries = fc.graph(orc, dim, metric)[1]
    dev = _device(native, orc, dim, metric)
    shares = ec.THREE_PLAIN_SHARES
    groups = np.arange(len(queries)) % 3
    words = _words(np.stack([fc.mask(fc.N, s) for s in shares]))
    got = dev.filtered_search(queries, k, ef, words, groups.astype(np.uint32))
    want = [fc.replays(orc, dim, metric, "gist", k, ef, shares[g])[i] for i, g in enumerate(groups)]
    fc.assert_matches(got, want, "three masks")


def test_through_three_masks_in_one_batch(native, orc):
    """Half the rows, another half, all rows: every pool fills."""
    dim, metric, k, ef = ec.THREE
    base, queries, arrays = fc.graph(orc, dim, metric)
    dev = _device(native, orc, dim, metric)
    second = ec.second_half_mask(fc.N)
    groups = np.arange(len(queries)) % 3
    words = _words(np.stack([fc.mask(fc.N, 0.5), second, np.ones(fc.N, bool)]))
    got = dev.filtered_search_hop(queries, k, ef, words, groups.astype(np.uint32))
    view = dc.view_of(orc, base, arrays, metric)
    mid = hc.replays(orc, dim, metric, "half2", k, ef, 0.5, view=view, queries=queries[1::3], allow=second)
    want = []
    for i, g in enumerate(groups):
        want.append(mid[i // 3] if g == 1 else hc.replays(orc, dim, metric, "gist", k, ef, (0.5, None, 1.0)[g])[i])
    hc.assert_matches(got, want, "three masks")
