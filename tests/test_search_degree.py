"""The device graph search at level-0 degrees other than 32 (every other search suite builds R = 32).

The C ABI takes any degree 1..64 (alaya_graph_import, alaya_index_set_graph, alaya_graph_load,
alaya_graph_build_hnsw), and a good part of hnsw_search_kernel depends on R or on the number of fresh
candidates of one expansion, which R = 32 caps at 32.  The bar is the one of every search test
(test_gpu._check): ids equal, distance bit patterns equal, all four counters equal to the oracle's
``view.search(..., with_counters=True)``; where a feature must have run, its stats call says so.

Inputs (tests/degree_common.py): gist_like(2000, 12, dim, 5 centres) rows, Graph.build at R in
{2, 8, 16, 24, 48, 64}, and, derived from the R = 64 build, rows truncated to odd widths, exact 64-NN
rows (up to 64 fresh candidates per expansion) and rows with a repeated id.  A CPU test replays the
search and pins that the inputs really reach the paths: expansions that start with a full pool and
have more than 32 (a second screen pass) or more than 48 fresh candidates.

Kernel lines (alayalite_amd/csrc; search_kernels.hip unless another file is named) per group:
  1 plain      adjacency load, end mask and count :911-915 and the loads of the predicted next row
               :957 / :1132, which serve most pops (lane < p.R; odd R: row starts at no multiple of 16
               bytes; R = 64: no idle lane), dedup_edges loop :919-924, fresh-id compaction
               :964-966, pool_merge with up to 64 newcomers :1127 (search_device.h:1484, the register
               merge of the d <= 256 kernels at ef <= 128 and the binary-search merge), the overlay
               descent of query_begin :112-248 with upper_R = 64 (64 live lanes in its min reduction).
  2 screen     second pass of screen_distances / screen_distances_u8 / screen_dots_int
               (search_device.h:361, :439, :664: base = 32), keep and compaction :1085-1096 over up to
               64 lanes, the nd <= 8 / nd <= 16 / full choice of space_distances :1104-1113.
  3 scout      the gate ix->R <= kScoutR (capi.cpp:590); at R < 32 scout_loop stores `mine < R`
               bounds of a memo row (:658, :707) and the searcher reads bound[row][lane & 31] (:983-987).
  4 spill      the trigger vs.count + 64 > vs.limit :925 with up to 64 inserts per expansion.
  5 helpers    the memo of W * kHelpMemoSlots * R * 8 bytes (capi.cpp:555-566: placement or the
               fallback), its index (wave * kHelpSlots + hs) * p.R :998-999 and help_siblings :477-571.
  6 SQ8        the same expansion loop in the kSpace 1 / 2 kernels (spill_prefetch :1029 under lane < p.R).
  7 build      the graph alaya_index_build_graph leaves installed at R = 8 / 64 (capi.cpp:1776).
  8 updates    alaya_index_insert's search_solo for k = R neighbours (capi.cpp:1469-1478; R = 64 > ef:
               slots past the pool are (0, 0.0)), write_edges_locked rows of R ids (capi.cpp:1368-1376).
  9 ABI        R checks of alaya_graph_import (capi.cpp:1136) and alaya_index_set_graph (:1253),
               alaya_graph_load at max_nbrs 16 and 64.
"""

import ctypes as C

import numpy as np
import pytest

import degree_common as dc
import refformat as rf
from build_common import SEED, assert_graph_equals, assert_search_equals, restated, rows_of

gpu = pytest.mark.gpu

KEF = [(10, 16), (10, 64), (10, 200), (1, 1)]
_totals = {}
_bounds = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("ALAYA_SEARCH_SCREEN", "ALAYA_SEARCH_SCOUT", "ALAYA_SEARCH_SCOUT_MISS", "ALAYA_SEARCH_SCOUT_GRID",
                 "ALAYA_TWO_WAVES", "ALAYA_HELPERS", "ALAYA_HELP_FLAGS", "ALAYA_SEARCH_WAVES"):
        monkeypatch.delenv(name, raising=False)


def _input(native, dim, deg, metric=0):
    """deg: an int = built at that R; "t<w>" = the R = 64 build truncated to w; "dense"; "dup"."""
    if isinstance(deg, int):
        return dc.built(native, dim, metric, deg)
    if deg == "dense":
        return dc.dense(native, dim, metric)
    if deg == "dup":
        return dc.duplicated(native, dim, metric)
    return dc.truncated(native, dim, metric, int(deg[1:]))


def _totals_of(native, orc, dim, deg, ef):
    key = (dim, deg, ef)
    if key not in _totals:
        base, queries, arrays = _input(native, dim, deg)
        if dim not in _bounds and dim >= 512:
            _bounds[dim] = dc.int_bounds(native, base, queries)
        _totals[key] = dc.replay_totals(orc, dc.view_of(orc, base, arrays), queries, ef, _bounds.get(dim))
    return _totals[key]


def _bits(out):
    return [np.asarray(a).view(np.uint32) for a in out]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


# ---- preconditions (no GPU) -------------------------------------------------------------------------
SCREENED_WIDE = [(dim, deg, ef) for dim in (512, 960) for deg in (48, 64) for ef in (48, 96)] + \
                [(512, "dense", 48), (512, "dense", 96)]


def test_inputs_reach_the_wide_paths(native, orc):
    """Every screened input of R >= 48 below has, over its 12 queries, at least 10 expansions that
    begin with a full pool and have more than 32 fresh candidates (the screen functions' second pass,
    keep over more than 32 lanes), and the dense rows have at least 10 with more than 48.  At d = 128
    the dense rows give at least 10 expansions of more than 48 candidates, pool full or not (at ef 200
    the pool fills late), which is what the merge sees.  An input that falls short gets another ef or
    other centres, not a lower floor."""
    for dim, deg, ef in SCREENED_WIDE:
        t = _totals_of(native, orc, dim, deg, ef)
        print(dim, deg, ef, t)
        assert t["over32"] >= 10, (dim, deg, ef, t)
    # (ef 48: 21 such expansions on every build tried; ef 96 has 10, too close to the floor to pin)
    assert _totals_of(native, orc, 512, "dense", 48)["over48"] >= 10
    for ef in (64, 200):
        t = _totals_of(native, orc, 128, "dense", ef)
        print(128, "dense", ef, t)
        assert t["any48"] >= 10 and t["over32"] >= 10 and t["most"] > 48, t
    assert dc.duplicated_rows_edited(native, 128) >= 50
    l0 = dc.duplicated(native, 128)[2][0]
    assert any(len(set(r[r != dc.EMPTY].tolist())) < int((r != dc.EMPTY).sum()) for r in l0)


def test_degree_out_of_range_is_an_error_host(native):
    """alaya_graph_import (Graph.from_arrays): R = 0 and R = 65 are argument errors."""
    eps = np.array([1], np.uint32)
    for width in (0, 65):
        with pytest.raises(ValueError, match="R must be 1..64"):
            native.Graph.from_arrays(np.zeros((10, width), np.uint32), None, None, None, 0, 0, eps)
    for width in (1, 64):
        g = native.Graph.from_arrays(np.full((10, width), 3, np.uint32), None, None, None, 0, 0, eps)
        assert g.arrays()[0].shape == (10, width)


def test_restatement_defines_k_above_ef(native, orc, c1):
    """k > ef reads past LinearPool in the reference (test_gpu.test_k_larger_than_ef).  The engine
    defines it -- the first ef slots are the pool, the rest (id 0, 0.0) -- and so must the oracle, whose
    Updater asks for k = R results at the insert's ef (R = 64, ef 48 below): it once read past its pool
    there and linked the new node to whatever ids the heap held."""
    base, queries = c1
    l0, levels, off, ue, ep, upper_r, _ = native.Graph.build(base, 0, 64, 100, 1, 100).arrays()
    view = orc.IndexView(base, l0, levels, off, ue, upper_r, ep)
    for q in queries:
        ids, d = view.search(q, 64, 48)
        p_ids, p_d = view.search(q, 48, 48)
        assert np.array_equal(ids[:48], p_ids) and np.array_equal(d[:48].view(np.uint32), p_d.view(np.uint32))
        assert not ids[48:].any() and not d[48:].view(np.uint32).any()
    b_ids, b_d, _, _ = view.batch_search(queries, 64, 48)
    assert not b_ids[:, 48:].any() and not b_d[:, 48:].view(np.uint32).any()
    up = orc.Updater(view, 1001)
    assert up.insert(queries[0], queries[0], 48) == 1000
    row = up.l0()[1000]
    assert np.array_equal(row[:48], view.search(queries[0], 48, 48)[0]) and not row[48:].any()


# ---- 1. plain kernels -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R", [2, 8, 16, 24, 48, 64])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dim", [100, 128, 256])
def test_plain_built_degrees(native, orc, dim, metric, R):
    """d = 100 the runtime-d kernel, 128 / 256 the small-row kernels (register merge at ef <= 128,
    binary-search merge at ef 200); R = 64: a full wave of adjacency lanes and upper_R = 64."""
    base, queries, arrays = dc.built(native, dim, metric, R)
    view = dc.view_of(orc, base, arrays, metric)
    dev = dc.device_of(native, base, arrays, metric)
    for k, ef in KEF:
        dc.check(view, dev, queries, k, ef)


@gpu
@pytest.mark.parametrize("width", [1, 7, 33, 63])
@pytest.mark.parametrize("metric", [0, 1])
def test_plain_truncated_rows(native, orc, metric, width):
    """Odd widths: row u starts at byte 4 * width * u, aligned to 4 bytes only; the overlay stays 64 wide."""
    base, queries, arrays = dc.truncated(native, 128, metric, width)
    view = dc.view_of(orc, base, arrays, metric)
    dev = dc.device_of(native, base, arrays, metric)
    for k, ef in KEF:
        dc.check(view, dev, queries, k, ef)


@gpu
@pytest.mark.parametrize("ef", [64, 200])
@pytest.mark.parametrize("kind", ["dense", "dup"])
def test_plain_dense_and_duplicated_rows(native, orc, kind, ef):
    """Exact 64-NN rows: up to 64 newcomers in one merge (33..64 never happen at R = 32).  Repeated
    ids in rows of 40..63 entries: the dedup loop over lanes 32..63."""
    base, queries, arrays = _input(native, 128, kind)
    dc.check(dc.view_of(orc, base, arrays), dc.device_of(native, base, arrays), queries, 10, ef)


@gpu
@pytest.mark.parametrize("ef", [70, 128, 129])
@pytest.mark.parametrize("kind", [64, "dense"])
def test_plain_ties_wide_merge(native, orc, kind, ef):
    """test_gpu.test_search_ties_pool_merge's rows at R = 64: among up to 64 tied newcomers the merge
    order alone decides (ef 70 / 128: register merge, 129: binary-search merge)."""
    b, q = dc.tie_rows(128, 128 + 64)
    if kind == "dense":
        _, _, (_, levels, off, ue, ep, upper_r) = dc.built(native, 128, 0, 64, data=("ties", b, q))
        arrays = (dc.exact_neighbours(b, 64), levels, off, ue, ep, upper_r)
    else:
        arrays = dc.built(native, 128, 0, 64, data=("ties", b, q))[2]
    dc.check(dc.view_of(orc, b, arrays), dc.device_of(native, b, arrays), q, 10, ef)


# ---- 2. screen --------------------------------------------------------------------------------------
def _screen_case(native, orc, dim, deg, ef, fmt):
    """One screened search against the oracle, and against the replay: the screened count where a second
    pass exists, and under the integer screen (whose bound the host restates bit for bit from exact
    integer sums) the screened-out count too -- a second pass that ran but left wrong sums changes no
    counter and often no id, but it changes which candidates are dropped."""
    base, queries, arrays = _input(native, dim, deg)
    view = dc.view_of(orc, base, arrays)
    dev = dc.device_of(native, base, arrays)
    _, _, cnt = dc.check(view, dev, queries, 10, ef)
    screened, out = dev.screen_stats()
    print(f"dim {dim} deg {deg} ef {ef}: screened {screened}, out {out}, n_dist {int(cnt[:, 0].sum())}")
    assert 0 < out <= screened <= int(cnt[:, 0].sum())
    if deg == "dense" or (isinstance(deg, int) and deg >= 48):
        t = _totals_of(native, orc, dim, deg, ef)
        assert t["over32"] >= 10
        assert (t["n_dist"], t["n_expand"]) == (int(cnt[:, 0].sum()), int(cnt[:, 1].sum()))
        # a skipped second pass cannot hide behind unchanged ids
        assert screened == t["screened"], (screened, t)
    if fmt == "9":
        t = _totals_of(native, orc, dim, deg, ef)
        print(f"  replay: screened {t['screened']}, out by the host's bounds {t['out9']}")
        assert (screened, out) == (t["screened"], t["out9"]), (screened, out, t)
    return dev


@gpu
@pytest.mark.parametrize("ef", [48, 96])
@pytest.mark.parametrize("deg", [16, 48, 64, "t33"])
@pytest.mark.parametrize("dim", [512, 960])
@pytest.mark.parametrize("fmt", ["1", "8", "9"])
def test_screen_degrees(native, orc, monkeypatch, fmt, dim, deg, ef):
    """The three screen formats (f16 rows, 8-bit records in f32, integer dot products) past one pass of
    32 rows.  (Under format 9 at d = 960 the scout is on by default where the plan admits it: R <= 32.)"""
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", fmt)
    _screen_case(native, orc, dim, deg, ef, fmt)


@gpu
@pytest.mark.parametrize("ef", [48, 96])
@pytest.mark.parametrize("fmt", ["1", "8", "9"])
def test_screen_dense_rows(native, orc, monkeypatch, fmt, ef):
    """More than 48 fresh candidates with the pool full: both passes nearly full, keep over 64 lanes."""
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", fmt)
    assert _totals_of(native, orc, 512, "dense", 48)["over48"] >= 10
    _screen_case(native, orc, 512, "dense", ef, fmt)


@gpu
@pytest.mark.parametrize("fmt", ["1", "8", "9"])
def test_screen_two_waves_r64(native, orc, monkeypatch, fmt):
    """The two-waves-per-SIMD screening kernels (one row per lane group) at R = 64."""
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", fmt)
    monkeypatch.setenv("ALAYA_TWO_WAVES", "1")
    _screen_case(native, orc, 960, 64, 96, fmt)


# ---- 3. scout ---------------------------------------------------------------------------------------
SCOUT_EF = 48


def _scout_run(native, orc, monkeypatch, dim, R, scout):
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "9")
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT", str(scout))
    base, queries, arrays = dc.built(native, dim, 0, R)
    dev = dc.device_of(native, base, arrays)
    out = dc.check(dc.view_of(orc, base, arrays), dev, queries, 10, SCOUT_EF)
    return out, dev.screen_stats(), dev.scout_stats(), dev.last_launch(), dev.last_plan()


@gpu
@pytest.mark.parametrize("R", [16, 24])
@pytest.mark.parametrize("dim", [768, 960])
@pytest.mark.parametrize("scout", [1, 2])
def test_scout_narrow_rows(native, orc, monkeypatch, scout, dim, R):
    """R < 32: the scout writes R bounds of a 32-entry memo row, the searcher reads its own adjacency
    position's; mode 2 checks every taken bound against the searcher's own."""
    off, off_screen, off_scout, off_launch, off_plan = _scout_run(native, orc, monkeypatch, dim, R, 0)
    on, on_screen, (expansions, hits, records, bad), launch, plan = _scout_run(native, orc, monkeypatch, dim, R, scout)
    print(f"dim {dim} R {R}: screened expansions {expansions}, memo hits {hits}, records {records}, screen {on_screen}")
    assert off_plan["scout"] == 0 and off_scout == (0, 0, 0, 0) and off_launch[1] == 1
    assert plan["scout"] == (1 if scout == 1 else 3)
    assert 0 < hits <= expansions and bad == 0
    assert _same(on, off) and on_screen == off_screen and on_screen[1] > 0
    assert launch[1] == 2


@gpu
@pytest.mark.parametrize("R", [48, 64])
@pytest.mark.parametrize("dim", [768, 960])
@pytest.mark.parametrize("scout", [1, 2])
def test_scout_absent_above_32(native, orc, monkeypatch, scout, dim, R):
    """R > kScoutR: a memo row holds one screen pass, so the plan stands without scouts."""
    _, screen, stats, launch, plan = _scout_run(native, orc, monkeypatch, dim, R, scout)
    assert plan["scout"] == 0 and stats == (0, 0, 0, 0) and launch[1] == 1
    assert screen[1] > 0


# ---- 4. visited spill -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("log2", [7, 8])
def test_visited_spill_dense_rows(native, orc, log2, mode):
    """128- and 256-slot tables under up to 64 inserts per expansion: the spill must begin while the
    table still has room for a whole expansion."""
    base, queries, arrays = dc.dense(native, 128)
    dev = dc.device_of(native, base, arrays)
    dev.set_hash_log2(log2)
    dev.set_visited_mode(mode)
    dc.check(dc.view_of(orc, base, arrays), dev, queries, 10, 200)


# ---- 5. helpers -------------------------------------------------------------------------------------
def _helped(orc, dev, view, queries, ef, search):
    """Batches of 1 and 7 with helpers off and on: bit-equal to each other and to the oracle.
    Returns per batch (memo distances, waves per group) of the helped run."""
    seen = []
    for nq in (1, 7):
        qs = queries[:nq]
        dev.set_helpers(0)
        plain = search(qs)
        dev.set_helpers(1)
        helped = search(qs)
        stats, launch = dev.help_stats(), dev.last_launch()
        assert _same(helped, plain)
        for i, q in enumerate(qs):
            o_ids, o_d, o_c = view.search(q, 10, ef, with_counters=True)
            assert np.array_equal(helped[0][i], o_ids), (nq, i)
            assert np.array_equal(helped[1][i].view(np.uint32), o_d.view(np.uint32)), (nq, i)
            assert tuple(helped[2][i]) == tuple(o_c), (nq, i)
        assert stats[0] <= int(helped[2][:, 0].sum())
        seen.append((stats[0], launch[1]))
    return seen


@gpu
@pytest.mark.parametrize("ef", [40, 128])
@pytest.mark.parametrize("R", [16, 64])
def test_helpers_f32(native, orc, R, ef):
    """d = 128 f32: the memo (4 searchers x 2 requests x R x 8 bytes: 1 KB at R = 16, 4 KB at R = 64)
    is larger than the 512-byte query region, so plan_search lays it over the memo wave's pool and
    visited table, which needs wave_lds >= 512 + 768 + memo.  At R = 64 that is 5,376 bytes; the wave's
    fixed part is 1,632 (ef 40) / 2,336 (ef 128) bytes and size_visited gives four-wave groups at 16
    waves per CU a table of 8 KB (ef 40, wide) / 4 KB (ef 128, compact) or more, so the memo is placed at
    both R: helpers run (four waves per group) and memo distances are taken."""
    base, queries, arrays = dc.built(native, 128, 0, R)
    dev = dc.device_of(native, base, arrays)
    seen = _helped(orc, dev, dc.view_of(orc, base, arrays), queries, ef, lambda qs: dev.search(qs, 10, ef))
    print(f"R {R} ef {ef}: (memo distances, waves per group) {seen}")
    assert all(w == 4 for _, w in seen)
    assert sum(m for m, _ in seen) > 0


def _sq8_memo_fits(R, ef):
    """plan_search's rule (capi.cpp:555-566) for the AVX-512-order SQ8 kernel at d = 128: the search runs
    on the spill table, so the first level is 128 wide slots (512 bytes, size_visited) and a wave's region
    is 512 (query) + 768 (three 64-entry lists) + 2 pool arrays + 512 bytes."""
    pool = 2 * (((ef + 1) * 4 + 15) // 16 * 16)
    return 512 + 768 + pool + 512 >= 512 + 768 + 4 * 2 * R * 8


@gpu
@pytest.mark.parametrize("ef", [40, 128])
@pytest.mark.parametrize("R", [16, 64])
@pytest.mark.parametrize("metric", [1, 0])
def test_helpers_sq8_128(native, orc, metric, R, ef):
    """test_helped_sq8_128_memo_over_the_table's shape.  The wave region is small here (_sq8_memo_fits):
    2,144 bytes at ef 40 and 2,848 at ef 128, against 1,280 + memo = 2,304 (R = 16) / 5,376 (R = 64).  So
    the memo is placed only at R = 16, ef 128; elsewhere -- R = 64 at both ef -- plan_search falls back
    to the search without helpers, whose help_stats() are zero."""
    base, queries, arrays = dc.built(native, 128, metric, R)
    mn, mx = native.sq8_train(base)
    codes = native.sq8_encode(base, mn, mx, 4)
    view = dc.view_of(orc, base, arrays, metric, sq8=(codes, mn, mx, 2))
    dev = dc.device_of(native, base, arrays, metric)
    dev.set_sq8(codes, mn, mx, 2)
    seen = _helped(orc, dev, view, queries, ef, lambda qs: dev.search_sq8(qs, 10, ef, 0))
    print(f"metric {metric} R {R} ef {ef}: (memo distances, waves per group) {seen}")
    if _sq8_memo_fits(R, ef):
        assert (R, ef) == (16, 128)
        assert all(w == 4 for _, w in seen) and sum(m for m, _ in seen) > 0
    else:
        assert all(m == 0 for m, _ in seen)
        assert seen[0][1] == 1  # one query, no helpers: one wave


# ---- 6. SQ8 -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R", [16, 64])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dim", [128, 768])
@pytest.mark.parametrize("order", [2, 1])
def test_sq8_degrees(native, orc, order, dim, metric, R):
    """test_sq8_search_and_rerank_bit_exact at R = 16 / 64: the SQ8 graph search and the reference rerank."""
    base, queries, arrays = dc.built(native, dim, metric, R)
    mn, mx = native.sq8_train(base)
    codes = native.sq8_encode(base, mn, mx, 4)
    view = dc.view_of(orc, base, arrays, metric, sq8=(codes, mn, mx, order))
    dev = dc.device_of(native, base, arrays, metric)
    dev.set_sq8(codes, mn, mx, order)
    k, ef = 10, 40
    s_ids, s_d, s_c = dev.search_sq8(queries, k, ef, False)
    r_ids, r_d, _ = dev.search_sq8(queries, k, ef, True)
    for i, q in enumerate(queries):
        o_ids, o_d, o_c = view.search(q, k, ef, with_counters=True)
        assert np.array_equal(s_ids[i], o_ids), (i, s_ids[i], o_ids)
        assert np.array_equal(s_d[i].view(np.uint32), o_d.view(np.uint32))
        assert tuple(s_c[i]) == tuple(o_c)
        rr_ids, rr_d = view.rerank(q, o_ids, k, ef)
        assert np.array_equal(r_ids[i], rr_ids), (i, r_ids[i], rr_ids)
        assert np.array_equal(r_d[i].view(np.uint32), rr_d.view(np.uint32))


# ---- 7. installed device build ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R", [8, 64])
def test_installed_graph_searches_at_degree(native, orc, R):
    """test_installed_graph_is_the_restated_one at R = 8 / 64: the graph the build leaves on the device
    searches as the CPU search does on the restatement's arrays."""
    spec = ("uniform", 2000, 48, 11)
    base = rows_of(spec)
    ref = restated(spec, R=R)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0, None)
    g, stats = dev.build_graph(R, 100, SEED, 0, 0, 2)
    assert_graph_equals(g, stats, ref)
    view = orc.IndexView(base, ref[0], ref[1], ref[2], ref[3], ref[5], ref[4], metric=0)
    q = np.random.default_rng(6).random((24, 48), dtype=np.float32)
    for ef in (50, 16):
        assert_search_equals(view, dev, q, 10, ef)


# ---- 8. online updates through the C ABI ------------------------------------------------------------
def _update_lib():
    from binding_replay import load_lib

    lib = load_lib()
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    sig = {
        "alaya_index_enable_updates": (i32, [vp, vp, vp, u64, u64, vp]),
        "alaya_index_insert": (i32, [vp, vp, vp, u32, C.POINTER(u64)]),
        "alaya_index_remove": (i32, [vp, u64]),
        "alaya_index_export_graph": (i32, [vp, C.POINTER(vp)]),
        "alaya_graph_info": (i32, [vp, C.POINTER(u64), C.POINTER(u32), vp, vp, vp, vp, vp, vp]),
        "alaya_graph_export": (i32, [vp, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@gpu
@pytest.mark.parametrize("ef", [48, 100])
@pytest.mark.parametrize("R", [16, 64])
def test_updates_at_degree_through_the_abi(native, orc, R, ef):
    """test_updates._engine_vs_restatement's op sequence (d = 24, 120 inserts, a remove every seventh)
    through alaya_index_enable_updates / _insert / _remove / _export_graph, against orc.Updater.  At
    R = 64 with ef 48 the insert's own search asks for k = R > ef results: slots past the pool are
    (id 0, 0.0) in the engine and the restatement alike."""
    lib = _update_lib()

    def ok(rc):
        assert rc == 0, lib.alaya_last_error().decode()

    rng = np.random.default_rng(40 + R)
    n0, d, cap = 600, 24, 750
    base = rng.standard_normal((n0 + 200, d)).astype(np.float32)
    fit_rows = np.ascontiguousarray(base[:n0])
    l0, levels, off, ue, ep, ur, _ = native.Graph.build(fit_rows, 0, R, 100, 1, 100).arrays()
    up = orc.Updater(orc.IndexView(fit_rows, l0, levels, off, ue, ur, ep), cap)
    ix, g, exported = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(lib.alaya_index_create(0, C.byref(ix)))
    try:
        ok(lib.alaya_index_set_base(ix, _p(fit_rows), n0, d, 0, None))
        ue_arg = ue if ue.size else np.zeros(1, np.uint32)
        ok(lib.alaya_graph_import(n0, R, _p(l0), _p(levels), _p(off), _p(ue_arg), ue.size, ur, ep, None, 0, C.byref(g)))
        ok(lib.alaya_index_set_graph(ix, g))
        ok(lib.alaya_index_enable_updates(ix, g, _p(fit_rows), n0, cap, None))
        for i in range(n0, n0 + 120):
            row = np.ascontiguousarray(base[i])
            new_id = C.c_uint64()
            ok(lib.alaya_index_insert(ix, _p(row), _p(row), ef, C.byref(new_id)))
            assert new_id.value == up.insert(row, row, ef)
            if i % 7 == 0:
                r = int(rng.integers(0, i))
                up.remove(r)
                ok(lib.alaya_index_remove(ix, r))
        ok(lib.alaya_index_export_graph(ix, C.byref(exported)))
        n, gr = C.c_uint64(), C.c_uint32()
        ok(lib.alaya_graph_info(exported, C.byref(n), C.byref(gr), None, None, None, None, None, None))
        assert (n.value, gr.value) == (n0 + 120, R)
        got = np.zeros((n.value, R), np.uint32)
        ok(lib.alaya_graph_export(exported, _p(got), None, None, None, None))
        want = up.l0()
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (bad.size, int(bad[0]), got[bad[0]], want[bad[0]])
        qs = rng.standard_normal((16, d)).astype(np.float32)
        ids = np.zeros((16, 10), np.uint32)
        dists = np.zeros((16, 10), np.float32)
        ok(lib.alaya_index_batch_search(ix, _p(qs), 16, 10, 64, _p(ids), _p(dists), None))
        for i, q in enumerate(qs):
            o_ids, o_d = up.search(q, 10, 64)
            assert np.array_equal(ids[i], o_ids), (i, ids[i], o_ids)
            assert np.array_equal(dists[i].view(np.uint32), o_d.view(np.uint32)), i
    finally:
        for h in (g, exported):
            if h:
                lib.alaya_graph_free(h)
        lib.alaya_index_destroy(ix)


# ---- 9. ABI edges -----------------------------------------------------------------------------------
@gpu
def test_set_graph_rejects_degree_above_64(native, c1):
    """alaya_index_set_graph: a host graph wider than a wave (the host builder makes one) is refused with
    an argument error before anything is uploaded, and the index keeps the graph it had.  (No call of the
    ABI yields a graph object of R = 0 -- alaya_graph_import and alaya_graph_load refuse it -- so that
    half of the check is reachable on the host only: test_degree_out_of_range_is_an_error_host.)"""
    base, queries = c1
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0, None)
    good = native.Graph.build(base, 0, 64, 100, 8, 100)
    dev.set_graph(good)
    before = dev.search(queries, 10, 32)
    wide = native.Graph.build(base, 0, 65, 100, 8, 100)
    assert wide.arrays()[0].shape[1] == 65
    with pytest.raises(ValueError, match="1..64"):
        dev.set_graph(wide)
    assert _same(dev.search(queries, 10, 32), before)


@gpu
@pytest.mark.parametrize("R", [16, 64])
def test_reference_format_file_at_degree(native, orc, tmp_path, R):
    """A graph file in the reference's layout with max_nbrs_ = 16 / 64 (test_format.py covers 32):
    alaya_graph_load gives back the arrays, and the device searches them like the oracle."""
    base, queries, arrays = dc.built(native, 128, 0, R)
    l0, levels, off, ue, ep, upper_r = arrays
    path = str(tmp_path / f"ref{R}.index")
    rf.write_graph(path, 4, l0, dc.N + 100, overlay=(ep, rf.overlay_lists(levels, off, ue, upper_r)))
    g = native.Graph.load(path, 4)
    gl0, glev, goff, gue, gep, gR, _ = g.arrays()
    assert gl0.shape == (dc.N, R) and gR == R and gep == ep
    assert np.array_equal(gl0, l0) and np.array_equal(glev, levels)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0, None)
    dev.set_graph(g)
    view = orc.IndexView(base, gl0, glev, goff, gue, gR, gep)
    for k, ef in KEF:
        dc.check(view, dev, queries, k, ef)
        dc.check(dc.view_of(orc, base, arrays), dev, queries, k, ef)
