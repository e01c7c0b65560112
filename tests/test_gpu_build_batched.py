"""The batched device HNSW build (alaya_index_build_graph at batch sizes above one: build_search,
build_select, build_apply, the edge sort and the host's batch schedule) against its CPU restatement
(oracle.build_hnsw_batched, oracle/oracle_build_batched.cpp), bit for bit.

Every comparison is exact: l0, levels, upper_off, upper_edges, ep, upper_R, and the counters
batches / max_batch / max_level / prunes / appends / heuristic_dists.  The restatement itself is
validated without a GPU in test_oracle_build_batched.py.  Cases: every search-kernel width class and
both metrics at the default schedule; doubling, tiny and refined schedules; row widths R = 2 .. 64
and ef_construction below M; a hub row that receives hundreds of reverse edges in one step; tied and
duplicate rows; the build search's visited-table spill; and the graph left installed on the device."""

import numpy as np
import pytest
from build_common import (HUB_SEED, SEED, assert_graph_equals, assert_search_equals, restated, rows_of)

pytestmark = pytest.mark.gpu


def _build(native, spec, metric=0, R=32, efc=100, batch_div=0, max_batch=0, refine=2, seed=SEED, prepare=None):
    dev = native.DeviceIndex(0)
    dev.set_base(rows_of(spec), metric, None)
    if prepare:
        prepare(dev)
    g, stats = dev.build_graph(R, efc, seed, batch_div, max_batch, refine)
    return dev, g, stats


def _same(native, spec, **kw):
    """Device build == restatement for one input and one parameter set; returns (dev, graph, ref)."""
    prepare = kw.pop("prepare", None)
    ref = restated(spec, **kw)
    dev, g, stats = _build(native, spec, prepare=prepare, **kw)
    assert_graph_equals(g, stats, ref)
    return dev, g, ref


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d,n", [(24, 3000), (64, 3000), (100, 3000), (128, 3000), (768, 1200), (960, 1200)])
def test_widths_and_metrics_default_schedule(native, orc, d, n, metric):
    """d = 128 / 768 / 960 run the specialised search kernels, the rest the runtime-d one (100 is
    no multiple of 8); select and apply always run the runtime-d distance loop."""
    spec = ("uniform", n, d, 300 + d)
    dev, _, ref = _same(native, spec, metric=metric)
    assert ref[6]["max_batch"] > 64  # real batches
    view = orc.IndexView(rows_of(spec), ref[0], ref[1], ref[2], ref[3], ref[5], ref[4], metric=metric)
    q = np.random.default_rng(d).random((12, d), dtype=np.float32)
    assert_search_equals(view, dev, q, 10, 50)


@pytest.mark.parametrize("batch_div,max_batch,refine", [(1, 0, 0), (1, 0, 1), (2, 64, 2), (64, 0, 1), (16, 0, 3)])
def test_schedules(native, batch_div, max_batch, refine):
    """(1, 0, *) doubles the batch every step; (2, 64, *) caps it; (64, 0, *) keeps it tiny with many
    single-point batches, which skip their refine steps; refine 3 repeats the level-0 pass."""
    _, _, ref = _same(native, ("uniform", 2500, 32, 9), batch_div=batch_div, max_batch=max_batch, refine=refine)
    st = ref[6]
    if max_batch:
        assert st["max_batch"] <= max_batch
    if batch_div == 1:
        assert st["max_batch"] > 512


@pytest.mark.parametrize("R,efc", [(2, 100), (8, 100), (32, 100), (64, 100), (32, 4)])
def test_row_widths_and_small_ef(native, R, efc):
    """R = 2 is M = 1; R = 64 is a full wave per row and up to 128 candidates in a prune; efc 4 is
    below M = 16, so ef = M and most pools hold fewer than M candidates (the keep-all path)."""
    _same(native, ("uniform", 2000, 48, 11), R=R, efc=efc)


@pytest.mark.parametrize("refine", [0, 2])
@pytest.mark.parametrize("R", [32, 64])
def test_hub_many_reverse_edges_to_one_row(native, R, refine):
    kw = dict(R=R, batch_div=1, refine=refine, seed=HUB_SEED)
    assert restated("hub", **kw)[6]["max_incoming"] > 128  # precondition: three apply groups
    _same(native, "hub", **kw)


@pytest.mark.parametrize("name", ["tied_integers", "duplicate_block"])
def test_ties(native, name):
    """Arrival order in the pool and (distance, id) order in the prune are part of the definition."""
    _same(native, name)


@pytest.mark.parametrize("log2,mode", [(6, 1), (6, 2), (6, 3), (14, 0)])
def test_build_search_visited_spill(native, log2, mode):
    """A 64-slot visited table spills to the global bitset at the first expansion, in each layout
    (1 compact, 2 wide, 3 compact with short probes); a 2^14-slot one never does.  Same graph."""

    def prepare(dev):
        dev.set_hash_log2(log2)
        dev.set_visited_mode(mode)

    _same(native, ("uniform", 3000, 64, 364), prepare=prepare)


def test_installed_graph_is_the_restated_one(native, orc):
    """The graph left on the device by the build (not its host copy) searches exactly as the CPU
    search restatement does on the *restatement's* arrays."""
    spec = ("uniform", 3000, 96, 5)
    base = rows_of(spec)
    dev, _, ref = _same(native, spec)
    view = orc.IndexView(base, ref[0], ref[1], ref[2], ref[3], ref[5], ref[4], metric=0)
    q = np.random.default_rng(6).random((40, 96), dtype=np.float32)
    assert_search_equals(view, dev, q, 10, 50)
