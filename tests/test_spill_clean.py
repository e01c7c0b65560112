"""Every graph search kernel family leaves the visited set's second level clean, checked by reading it back
(DeviceIndex.spill_residue: the per-slot bitsets and spill tables of the index's scratch).

A word a query leaves set does not fault: it marks rows visited for whichever later query lands on that slot,
in a later launch, from another entry point.  So every case here forces 64-slot first-level tables
(set_hash_log2(6): every query spills at its first expansions), holds the launch to a few persistent searchers
so that each slot runs at least 8 queries one after the other, compares every answer with its restatement
(ids, distance bits, counts, counters), and then reads the areas back: 0 nonzero words, 0 nonzero entries, over
a number of bytes that covers every slot of the launch.  tests/spill_common.py has the inputs;
test_spill_clean_host.py checks that they spill and overflow a 3-word dirty list.

The filtered and range families are held to two workgroups by ALAYA_FILTER_GRID=2.  The two unfiltered
families have no such knob: they run one workgroup per CU (ALAYA_MAX_WAVES_PER_CU=1, helpers off) on a batch
of 8 queries per slot, the 250 distinct queries repeated."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc
import filter_hop_common as hc
import filter_sq8_common as sc
import range_common as rc
import range_more_common as rm
import range_sq8_common as rq
import spill_common as sp

pytestmark = pytest.mark.gpu

K = sp.K
WORDS_PER_SLOT = (sp.N + 31) // 32
ENV = ("ALAYA_FILTER_GRID", "ALAYA_SEARCH_WAVES", "ALAYA_VIS_LIMIT", "ALAYA_VIS_LIMIT_PCT", "ALAYA_SPILL_TABLE",
       "ALAYA_SPILL_FLAGS", "ALAYA_DIRTY_CAP", "ALAYA_RANGE_SORT", "ALAYA_MAX_WAVES_PER_CU", "ALAYA_HELPERS",
       "ALAYA_HELP_FLAGS", "ALAYA_TWO_WAVES", "ALAYA_SEARCH_SCREEN", "ALAYA_SEARCH_SCOUT")


@pytest.fixture(autouse=True)
def _few_slots(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("ALAYA_FILTER_GRID", "2")
    monkeypatch.setenv("ALAYA_MAX_WAVES_PER_CU", "1")
    monkeypatch.setenv("ALAYA_HELPERS", "0")
    monkeypatch.setenv("ALAYA_SPILL_TABLE", str(sp.SPILL_TABLE_LOG2))


def _device(native, c):
    """A fresh index of the case's graph (SQ8 families: with the AVX-512-order codes), 64-slot compact tables."""
    dev = dc.device_of(native, c["base"], c["arrays"])
    if c["quant"] is not None:
        mn, mx, codes = c["quant"]
        dev.set_sq8(codes, mn, mx, sp.ORDER)
    dev.set_hash_log2(sp.HASH_LOG2)
    dev.set_visited_mode(1)
    return dev


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _order(c):
    """The batch as indices into the case's queries: all of them once where ALAYA_FILTER_GRID holds the grid, else
    repeated to 8 queries for every slot of a launch of one workgroup per CU.

    The slot counts assumed here are the plan's under this file's environment (csrc/capi.cpp, plan_search):
    ALAYA_MAX_WAVES_PER_CU=1 holds the grid to one workgroup per CU, and with helpers off search_waves() gives an
    f32 workgroup 1 searcher and an SQ8 workgroup 4.  If either changes, _clean's "vacuous" failure for these two
    families means this function's batch is too small, not that a kernel is wrong."""
    if c["family"] == "plain":
        return _repeated(1)
    if c["family"] == "sq8":
        return _repeated(4)
    return np.arange(sp.NQ)


def _repeated(waves):
    """Indices of the NQ distinct queries repeated to 8 per slot of one `waves`-searcher workgroup per CU."""
    return np.arange(max(sp.NQ, 8 * waves * _cus())) % sp.NQ


def _launch(dev, c, order):
    f, ef = c["family"], c["ef"]
    q = np.ascontiguousarray(c["queries"][order])
    cap = sp.RANGE_CAP.get(f)
    if f == "plain":
        return dev.search(q, K, ef)
    if f == "sq8":
        return dev.search_sq8(q, K, ef, 0)
    if f == "filtered":
        return dev.filtered_search(q, K, ef, sp.words(c["allow"]))
    if f == "hop":
        return dev.filtered_search_hop(q, K, ef, sp.words(c["allow"]))
    if f == "filtered_sq8":
        return dev.filtered_search_sq8(q, K, ef, sp.words(c["allow"]), None, c["pool"])
    if f == "range":
        return dev.range_search(q, ef, np.ascontiguousarray(c["radii"][order]), cap, sp.words(c["allow"]))
    if f == "range_more":
        return dev.range_search_radius(q, ef, np.ascontiguousarray(c["radii"][order]), cap, sp.MAX_FRONTIER)
    if f == "range_sq8":
        return dev.range_search_sq8(q, ef, np.ascontiguousarray(c["radii"][order]),
                                    np.ascontiguousarray(c["code_radii"][order]), cap)
    raise KeyError(f)


def _compare(orc, c, got, order, what):
    f = c["family"]
    want = sp.in_order(c, order)
    if f in ("plain", "sq8"):
        ids, dists, cnt = got
        assert np.array_equal(ids, np.stack([w[0] for w in want])), what
        assert np.array_equal(dists.view(np.uint32), np.stack([w[1] for w in want]).view(np.uint32)), what
        assert np.array_equal(np.asarray(cnt, np.int64), np.array([tuple(w[2]) for w in want], np.int64)), what
    elif f == "filtered":
        fc.assert_matches(got, want, what)
    elif f == "hop":
        hc.assert_matches(got, want, what)
    elif f == "filtered_sq8":
        sc.assert_matches(got, want, what)
    elif f == "range":
        rc.assert_matches(got, want, c["radii"][order], sp.RANGE_CAP[f], what)
    elif f == "range_more":
        rm.assert_matches(got, want, c["radii"][order], sp.RANGE_CAP[f], what)
    else:
        rq.assert_matches(orc, got, want, c["base"], 0, c["queries"][order], c["radii"][order], c["code_radii"][order],
                          sp.RANGE_CAP[f], what)


def _clean(dev, nq, what, sq8=False, words_per_slot=WORDS_PER_SLOT, min_per_slot=8, table_log2=sp.SPILL_TABLE_LOG2):
    """After a launch of nq queries: it ran at 64 first-level slots with at least min_per_slot queries per
    searcher slot, and the read-back covers every slot's bitset (and spill table) and finds nothing set."""
    assert dev.last_plan()["hash_log2"] == sp.HASH_LOG2, (what, dev.last_plan())
    groups, waves = dev.last_launch()
    slots = groups * waves
    assert slots >= 1 and nq >= min_per_slot * slots, f"vacuous: {nq} queries on {groups} x {waves} slots {what}"
    w, e, wb, eb = dev.spill_residue()
    assert wb >= slots * words_per_slot * 4 > 0, (what, wb, slots)
    if sq8:
        assert eb >= slots * (2 << table_log2) > 0, (what, eb, slots, table_log2)
    assert (w, e) == (0, 0), f"{what}: {w} bitset words and {e} spill-table entries left set ({wb} + {eb} bytes read)"
    return slots


# ---- a. the accessor ---------------------------------------------------------------------------------------
def test_read_back_sees_a_marked_word_and_the_next_launch_zeroes_it(native, orc):
    c = sp.case(orc, "filtered")
    sp.check_inputs(c)
    dev = _device(native, c)
    assert dev.spill_residue() == (0, 0, 0, 0)  # no launch yet: nothing allocated, nothing read
    with pytest.raises(ValueError):
        dev.spill_mark(5)
    order = np.arange(sp.NQ)
    _compare(orc, c, _launch(dev, c, order), order, "before the mark")
    slots = _clean(dev, sp.NQ, "before the mark")
    dev.spill_mark(5)
    w, e, wb, eb = dev.spill_residue()
    assert (w, e) == (1, 0) and wb >= slots * WORDS_PER_SLOT * 4, (w, e, wb)
    with pytest.raises(ValueError):
        dev.spill_mark(wb // 4)  # one past the area
    # bit 0 of word 5 is row 160 on slot 0: left in place it would be "visited" for every query of that slot
    p = sp.case(orc, "plain")
    got = dev.search(p["queries"], K, p["ef"])
    _compare(orc, p, got, order, "after the mark")
    w, e, wb, eb = dev.spill_residue()
    assert (w, e) == (0, 0) and wb > 0, (w, e, wb)


# ---- b. every family, dirty list kept and overflowed ------------------------------------------------------
@pytest.mark.parametrize("dirty_cap", [None, "3"])
@pytest.mark.parametrize("family,dim", [(f, 64) for f in sp.FAMILIES] + [("hop", 960), ("range_more", 960)])
def test_family_leaves_its_slots_clean(native, orc, monkeypatch, family, dim, dirty_cap):
    if dirty_cap:
        monkeypatch.setenv("ALAYA_DIRTY_CAP", dirty_cap)
    c = sp.case(orc, family, dim)
    sp.check_inputs(c, int(dirty_cap) if dirty_cap else 0)
    dev = _device(native, c)
    order = _order(c)
    for tag, o in (("forward", order), ("reversed", order[::-1])):
        what = (family, dim, dirty_cap, tag)
        got = _launch(dev, c, o)
        _clean(dev, len(o), what, sq8=family in sp.SQ8_FAMILIES)
        _compare(orc, c, got, o, what)


# ---- c. one family after another on the same scratch ------------------------------------------------------
def _step(orc, dev, c, what, sq8=False):
    order = _order(c)
    got = _launch(dev, c, order)
    _clean(dev, len(order), what, sq8=sq8)
    _compare(orc, c, got, order, what)


@pytest.mark.parametrize("dirty_cap", [None, "3"])
def test_f32_families_in_sequence_on_one_index(native, orc, monkeypatch, dirty_cap):
    """The radius mode's batch (its flood fill included), then the plain search, the through search, the fixed
    range search, the filtered search and the plain search again: each on what the one before left."""
    if dirty_cap:
        monkeypatch.setenv("ALAYA_DIRTY_CAP", dirty_cap)
    dev = _device(native, sp.case(orc, "plain"))
    for i, family in enumerate(("range_more", "plain", "hop", "range", "filtered", "plain")):
        _step(orc, dev, sp.case(orc, family), ("f32 sequence", i, family, dirty_cap))


@pytest.mark.parametrize("dirty_cap", [None, "3"])
def test_sq8_families_in_sequence_on_one_index(native, orc, monkeypatch, dirty_cap):
    """Forced 64-entry tables: the range search with an infinite slack, the search, the filtered search -- then
    the search at a larger ef with the table size left to the launch (it depends on ef), so the per-slot table
    layout moves over what the earlier launches left."""
    if dirty_cap:
        monkeypatch.setenv("ALAYA_DIRTY_CAP", dirty_cap)
    dev = _device(native, sp.case(orc, "sq8"))
    for i, family in enumerate(("range_sq8", "sq8", "filtered_sq8")):
        _step(orc, dev, sp.case(orc, family), ("sq8 sequence", i, family, dirty_cap), sq8=True)
    before = dev.spill_residue()[3]
    monkeypatch.delenv("ALAYA_SPILL_TABLE")
    c = sp.case(orc, "sq8")
    view = sc.view_of(orc, c["base"], c["arrays"], 0, c["quant"], sp.ORDER)
    want = [view.search(x, K, 96, with_counters=True) for x in c["queries"]]
    wide = dict(c, ef=96, want=want, visited=[int(w[2][0]) + 1 for w in want], table=1 << _table_log2(96))
    # (every query spills; tables of this size need not fill their buckets, so the bitset may stay unused)
    assert min(wide["visited"]) > sp.FILL_LIMIT, f"vacuous: an ef 96 query marks {min(wide['visited'])} rows and need not spill"
    order = _order(wide)
    got = _launch(dev, wide, order)
    what = ("sq8 sequence", 3, "sq8 at ef 96", dirty_cap)
    _clean(dev, len(order), what, sq8=True, table_log2=_table_log2(96))
    assert dev.spill_residue()[3] > before, what  # larger tables: every slot's table starts elsewhere
    _compare(orc, wide, got, order, what)


def _table_log2(ef, n=sp.N):
    """log2 entries of a slot's spill table when ALAYA_SPILL_TABLE does not force it (csrc/capi.cpp,
    spill_table_log2): about 32 ef entries, at least 64, and no more buckets of 8 than the id hash has values."""
    bits = max(1, int(np.ceil(np.log2(max(n, 2)))))
    return min(max(6, int(np.ceil(np.log2(32 * ef)))), bits + 3)


def _index_view(orc, idx, rows, removed):
    l0, levels, off, ue, ep, ur, _ = idx.native().graph_arrays()
    n = len(rows)
    valid = np.full((n + 7) // 8, 0xFF, np.uint8)
    for v in removed:
        valid[v >> 3] &= ~np.uint8(1 << (v & 7))
    return orc.IndexView(rows, l0, levels, off, ue, ur, ep, metric=0, valid=valid if removed else None)


def test_row_count_changes_between_launches(native, orc):
    """search; Index.insert and Index.remove (1899 -> 1902 rows: 60 words per slot, where 1888 rows would still
    take 59); search; Index.add of 98 rows (63 words per slot); search.  The bulk add's build searches run on
    the same areas (run_build_steps sizes its visited set with size_visited and calls prepare_spill), so the
    read-back right after add, before any search, covers them too."""
    import alayalite_amd

    base, _ = dc.rows(64)
    distinct = sp.queries_of(base)
    order = _repeated(1)  # (the plain kernel through Index: no grid knob, so 8 queries per slot by batch size)
    queries = np.ascontiguousarray(distinct[order])
    idx = alayalite_amd.Client().create_index("spill_clean_rows", capacity=sp.N)
    idx.fit(base[:1899].copy(), ef_construction=100, num_threads=1)
    nat = idx.native()
    nat.set_hash_log2(sp.HASH_LOG2)
    nat.set_visited_mode(1)
    removed = []

    def search(n, what):
        ids, dists = idx.batch_search_with_distance(queries.copy(), K, 24)
        cnt = nat.last_counters()
        assert nat.last_plan()["hash_log2"] == sp.HASH_LOG2
        groups, waves = nat.last_launch()
        slots = groups * waves
        assert slots >= 1 and len(queries) >= 8 * slots, f"vacuous: {len(queries)} queries on {groups} x {waves} slots {what}"
        w, e, wb, eb = nat.spill_residue()
        assert wb >= slots * ((n + 31) // 32) * 4 > 0, (what, wb, groups, waves)
        assert (w, e) == (0, 0), (what, w, e, wb, eb)
        view = _index_view(orc, idx, base[:n], removed)
        want = [view.search(q, K, 24, with_counters=True) for q in distinct]
        assert min(int(r[2][0]) for r in want) + 1 > sp.FILL_LIMIT, f"vacuous: a query does not spill {what}"
        assert np.array_equal(ids, np.stack([want[j][0] for j in order])), what
        assert np.array_equal(dists.view(np.uint32), np.stack([want[j][1] for j in order]).view(np.uint32)), what
        assert np.array_equal(np.asarray(cnt, np.int64), np.array([tuple(want[j][2]) for j in order], np.int64)), what

    search(1899, "fitted")
    for i in range(1899, 1902):
        assert idx.insert(base[i].copy(), 48) == i
    for v in (8, 160, 1900):
        idx.remove(v)
        removed.append(v)
    search(1902, "after insert and remove")
    ids = idx.add(base[1902:2000].copy(), ef_construction=100)
    assert len(ids) == 98 and idx.get_data_num() == 2000
    w, e, wb, eb = nat.spill_residue()
    assert (w, e) == (0, 0) and wb > 0, ("after add", w, e, wb)
    search(2000, "after add")


# ---- d. device entries on two streams ----------------------------------------------------------------------
def test_device_entries_hand_the_scratch_from_stream_to_stream(native, orc):
    """filtered_search_device on one torch stream, range_search_device on another right behind it, one sync at
    the end: the second launch waits for the first on the device (scratch_acquire), on slots the first spilled."""
    import torch

    f, r = sp.case(orc, "filtered"), sp.case(orc, "range")
    dev = _device(native, f)
    nq, cap = sp.NQ, sp.RANGE_CAP["range"]
    d0 = torch.device("cuda", 0)
    one, two = torch.cuda.Stream(d0), torch.cuda.Stream(d0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d0)  # noqa: E731
    q = up(f["queries"])
    wd = up(sp.words(f["allow"]).view(np.int32))
    radii = up(r["radii"])
    ids = torch.full((nq, K), 7, dtype=torch.int32, device=d0)
    dd = torch.full((nq, K), 7.0, dtype=torch.float32, device=d0)
    cc = torch.full((nq, 4), 7, dtype=torch.int32, device=d0)
    r_n = torch.full((nq,), 7, dtype=torch.int32, device=d0)
    r_ids = torch.full((nq, cap), 7, dtype=torch.int32, device=d0)
    r_d = torch.full((nq, cap), 7.0, dtype=torch.float32, device=d0)
    r_c = torch.full((nq, 4), 7, dtype=torch.int32, device=d0)
    torch.cuda.synchronize(d0)  # the uploads and fills, on the current stream
    dev.filtered_search_device(q.data_ptr(), nq, K, f["ef"], wd.data_ptr(), 1, 0, ids.data_ptr(), dd.data_ptr(),
                               cc.data_ptr(), one.cuda_stream)
    dev.range_search_device(q.data_ptr(), nq, r["ef"], radii.data_ptr(), cap, wd.data_ptr(), 1, 0, r_n.data_ptr(),
                            r_ids.data_ptr(), r_d.data_ptr(), r_c.data_ptr(), two.cuda_stream)
    one.synchronize()
    two.synchronize()
    order = np.arange(nq)
    _clean(dev, nq, "two streams")
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    _compare(orc, f, (u32(ids), dd.cpu().numpy(), u32(cc)), order, "filtered, stream one")
    _compare(orc, r, (u32(r_n), u32(r_ids), r_d.cpu().numpy(), u32(r_c)), order, "range, stream two")
