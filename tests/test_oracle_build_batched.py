"""The CPU restatement of the batched device build (oracle/oracle_build_batched.cpp), validated
without a GPU before test_gpu_build_batched.py holds the device build to it bit for bit:
  * with single-point batches and no refine it is the sequential algorithm, so on tie-free rows its
    graph equals the restatement of HNSWBuilder::build_graph (oracle_build.cpp) exactly;
  * at real batch sizes its graphs satisfy the structural invariants and the recall floor that
    test_gpu_build.py asks of the device build;
  * the hub input really brings one destination more than 128 reverse edges in one step (three
    groups of 64 in apply), and the tie inputs are well-formed."""

import numpy as np
import pytest
from build_common import HUB_SEED, check_structure, exact_topk, recall, restated, rows_of, uniform


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("n,d", [(1500, 24), (600, 96)])
def test_single_point_batches_are_the_sequential_build(orc, n, d, metric):
    base = uniform(n, d, 17)
    seq = orc.build_hnsw(base, metric, 32, 100, 100)
    bat = orc.build_hnsw_batched(base, metric, 32, 100, 100, batch_div=1, max_batch=1, refine=0)
    for a, b in zip(seq, bat[:6]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    st = bat[6]
    assert st["batches"] == n - 1 and st["max_batch"] == 1 and st["max_incoming"] == 1
    assert st["max_level"] == int(seq[1].max())


@pytest.mark.parametrize("refine", [0, 1, 2])
def test_structure_and_recall_floor_at_default_batches(orc, refine):
    """2000 x 32, default schedule: the floor test_batch_schedules asks of the device build
    (recall@10 >= 0.9 at ef 64), measured with the restated search."""
    spec = ("uniform", 2000, 32, 9)
    base = rows_of(spec)
    ref = restated(spec, refine=refine)
    l0, levels = check_structure(ref, 2000, 32)
    st = ref[6]
    assert st["max_batch"] > 64 and st["batches"] > 10 and st["max_level"] == int(levels.max())
    view = orc.IndexView(base, *ref[:3], ref[3], ref[5], ref[4], metric=0)
    q = np.random.default_rng(90).random((50, 32), dtype=np.float32)
    ids = np.array([view.search(v, 10, 64)[0] for v in q])
    assert recall(ids, exact_topk(base, q, 10, 0)) >= 0.9


@pytest.mark.parametrize("R,refine", [(32, 0), (32, 2), (64, 0), (64, 2)])
def test_hub_reaches_three_apply_groups(R, refine):
    ref = restated("hub", R=R, batch_div=1, refine=refine, seed=HUB_SEED)
    check_structure(ref, 768, R)
    assert ref[6]["max_incoming"] > 128
    assert ref[6]["prunes"] > 0  # row 7 at the least: its incoming edges exceed any capacity


@pytest.mark.parametrize("name,n", [("tied_integers", 2000), ("duplicate_block", 1500)])
def test_tie_inputs_build_well_formed_graphs(name, n):
    ref = restated(name)
    check_structure(ref, n, 32)
    assert ref[6]["prunes"] > 0 and ref[6]["max_batch"] > 64


def test_thread_count_does_not_change_the_result(orc):
    """Work items of a step are spread over threads; twice the same graph and counters."""
    base = uniform(1200, 20, 3)
    a = orc.build_hnsw_batched(base, 0, 16, 40, 100)
    b = orc.build_hnsw_batched(base, 0, 16, 40, 100)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
