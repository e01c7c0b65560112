"""alaya_index_extend_graph (DeviceIndex.extend_graph): rows appended by continuing the batched device
build on the installed graph, against the CPU restatement of the build over ALL rows
(oracle.build_hnsw_batched), bit for bit.

The property: when n0 is a batch boundary of the schedule for all rows, build(first n0) followed by
extend(the rest) -- in one call or in several, each starting at a boundary -- is build(all): l0,
levels, upper_off, upper_edges, ep, and, summed over the parts, batches / prunes / appends /
heuristic_dists (max_batch: the largest part's, max_level: the final one).  Boundaries come from
native.build_batches, whose rule and the facts about the seeds used here are checked without a device
in test_extend_schedule.py.  Off a boundary the graph is another one: structure, levels and
determinism are checked.  Refusals leave the index as it was."""

import numpy as np
import pytest
from build_common import (HUB_SEED, SEED, assert_graph_equals, assert_search_equals, check_structure, restated,
                          rows_of)

pytestmark = pytest.mark.gpu

SUMMED = ("batches", "prunes", "appends", "heuristic_dists")
MAIN = ("uniform", 3000, 32, 9)


def _ends(native, spec, **kw):
    """Batch ends of the whole schedule for `spec` under the restated() parameters in kw."""
    lv = np.ascontiguousarray(restated(spec, **kw)[1], np.uint32)
    return native.build_batches(lv, 1, 0, kw.get("batch_div", 0), kw.get("max_batch", 0)).tolist()


def _end_in(ends, lo, hi):
    got = [e for e in ends if lo <= e < hi]
    assert got, (lo, hi)
    return got[0]


def _grow(native, spec, cuts, metric=0, R=32, efc=100, batch_div=0, max_batch=0, refine=2, seed=SEED, valid=None,
          before_extend=None):
    """build(rows[:cuts[0]]) then one extend per further cut, the last one to the end of the rows."""
    base = rows_of(spec)
    dev = native.DeviceIndex(0)
    dev.set_base(base[:cuts[0]], metric, valid)
    g, st = dev.build_graph(R, efc, seed, batch_div, max_batch, refine)
    parts = [st]
    if before_extend:
        before_extend(dev)
    for a, b in zip(cuts, list(cuts[1:]) + [len(base)]):
        g, st = dev.extend_graph(base[a:b], efc, seed, batch_div, max_batch, refine)
        parts.append(st)
    total = {k: sum(int(p[k]) for p in parts) for k in SUMMED}
    total["max_batch"] = max(int(p["max_batch"]) for p in parts)
    total["max_level"] = int(parts[-1]["max_level"])
    return dev, g, total


def _same(native, spec, cuts, **kw):
    extra = {k: kw.pop(k) for k in ("valid", "before_extend") if k in kw}
    ref = restated(spec, **kw)
    dev, g, total = _grow(native, spec, cuts, **kw, **extra)
    assert_graph_equals(g, total, ref)
    return dev, g, ref


# ---- boundary equality ---------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [[1029], [116], [116, 1029], [1029, 1093, 2000]])
def test_boundary_equality_default_schedule(native, cuts):
    """1029 and 1093 are size boundaries, 116 follows the row that raised the max level (the extension
    starts from the new entry point).  Chains carry the state between calls and grow upper_edges; the
    last chain's 2000 is the first boundary at or after it."""
    ends = _ends(native, MAIN)
    cuts = [c if c in ends else _end_in(ends, c, 3000) for c in cuts]
    assert all(c in ends for c in cuts)
    _same(native, MAIN, cuts)


def test_level_raise_inside_the_extension_hub_seed(native):
    ends = _ends(native, MAIN, seed=HUB_SEED)
    lv = restated(MAIN, seed=HUB_SEED)[1]
    assert lv[937] > lv[:937].max() and 938 in ends  # row 937 raises the max level and closes its batch
    n0 = _end_in(ends, 600, 937)
    _same(native, MAIN, [n0], seed=HUB_SEED)


def test_level_raise_inside_the_extension_r8(native):
    lv = restated(MAIN, R=8)[1]
    last = max(j for j in range(1, 3000) if lv[j] > lv[:j].max())
    assert last > 1200 and int(lv.max()) == 5
    ends = _ends(native, MAIN, R=8)
    n0 = _end_in(ends, 1000, last)
    _same(native, MAIN, [n0], R=8)


@pytest.mark.parametrize("n0", [1, 2, 431])
def test_sequential_schedule_every_row_is_a_boundary(native, n0):
    _same(native, ("uniform", 1000, 32, 9), [n0], batch_div=1, max_batch=1, refine=0)


@pytest.mark.parametrize("batch_div,max_batch,refine", [(2, 64, 2), (1, 0, 1)])
def test_other_schedules(native, batch_div, max_batch, refine):
    kw = dict(batch_div=batch_div, max_batch=max_batch, refine=refine)
    ends = _ends(native, ("uniform", 2500, 32, 9), **kw)
    _same(native, ("uniform", 2500, 32, 9), [_end_in(ends, 500, 2500)], **kw)


@pytest.mark.parametrize("spec,metric", [(("uniform", 3000, 24, 324), 1), (("uniform", 3000, 100, 400), 0),
                                         (("uniform", 3000, 128, 428), 0), ("tied_integers", 0),
                                         ("duplicate_block", 0)])
def test_widths_metric_and_ties(native, spec, metric):
    """d = 24 and 100 run the runtime-d build search (IP once), d = 128 a specialised one; tied and
    duplicate rows make the pool's arrival order and the prune's id order part of the result."""
    ends = _ends(native, spec, metric=metric)
    n = len(rows_of(spec))
    _same(native, spec, [_end_in(ends, n // 3, n)], metric=metric)


def test_wide_rows_and_searches_follow(native, orc):
    """d = 960: the specialised build search, and a query search before the extension so the index
    holds a screening copy of its rows; the searches afterwards must see the new rows' records and
    norms (ids, distance bits and counters of the CPU search on the restated graph)."""
    spec = ("uniform", 1200, 960, 1260)
    base = rows_of(spec)
    q = np.random.default_rng(960).random((12, 960), dtype=np.float32)
    ends = _ends(native, spec)
    dev, _, ref = _same(native, spec, [_end_in(ends, 400, 1200)], before_extend=lambda dev: dev.search(q, 10, 50))
    view = orc.IndexView(base, ref[0], ref[1], ref[2], ref[3], ref[5], ref[4], metric=0)
    assert_search_equals(view, dev, q, 10, 50)


def test_all_ones_bitmap_is_the_plain_build(native):
    ends = _ends(native, MAIN)
    n0 = _end_in(ends, 1000, 3000)
    _same(native, MAIN, [n0], valid=np.full((n0 + 7) // 8, 255, np.uint8))


# ---- off a boundary ------------------------------------------------------------------------------
def test_non_boundary_structure_levels_and_determinism(native):
    ends = _ends(native, MAIN)
    n0 = 1000
    assert n0 not in ends
    ref_levels = restated(MAIN)[1]
    _, g1, _ = _grow(native, MAIN, [n0])
    l0, levels = check_structure(g1.arrays(), 3000, 32)
    assert np.array_equal(levels, ref_levels)  # rows [0, n0) keep theirs, the rest is the full draw's tail
    _, g2, _ = _grow(native, MAIN, [n0])
    for a, b in zip(g1.arrays(), g2.arrays()):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


# ---- refusals ------------------------------------------------------------------------------------
def _searches(dev, q):
    ids, d, _ = dev.search(q, 10, 50)
    return ids.copy(), d.view(np.uint32).copy()


def test_refusals_leave_the_index_unchanged(native):
    base = rows_of(MAIN)
    q = np.random.default_rng(3).random((8, 32), dtype=np.float32)
    dev = native.DeviceIndex(0)
    dev.set_base(base[:1029], 0, None)
    with pytest.raises(ValueError):  # no graph yet
        dev.extend_graph(base[1029:])
    g, _ = dev.build_graph(32, 100, SEED, 0, 0, 2)
    l0, levels, off, ue, ep, upper_r = g.arrays()[:6]
    before = _searches(dev, q)
    with pytest.raises(ValueError):  # wrong row width
        dev.extend_graph(np.zeros((5, 33), np.float32))
    after = _searches(dev, q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # a graph without overlay (NSG style: level-0 rows and entry points only)
    flat = native.DeviceIndex(0)
    flat.set_base(base[:1029], 0, None)
    flat.set_graph(native.Graph.from_arrays(l0, None, None, None, 0, 0, np.array([ep], np.uint32)))
    before = _searches(flat, q)
    with pytest.raises(ValueError):
        flat.extend_graph(base[1029:])
    after = _searches(flat, q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # odd max_nbrs: the same graph with its rows cut to 31 ids
    odd = native.DeviceIndex(0)
    odd.set_base(base[:1029], 0, None)
    ue31 = np.ascontiguousarray(ue.reshape(-1, 32)[:, :31]).reshape(-1)
    odd.set_graph(native.Graph.from_arrays(np.ascontiguousarray(l0[:, :31]), levels, off // 32 * 31, ue31, 31, ep, None))
    before = _searches(odd, q)
    with pytest.raises(ValueError):
        odd.extend_graph(base[1029:])
    after = _searches(odd, q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
