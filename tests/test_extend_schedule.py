"""The batch schedule of the device build continued from a row count (alaya_build_batches, the host
function alaya_index_extend_graph schedules with) against a restatement of its rule: batch size
max(1, min(max_batch, inserted / batch_div)), and a row above the graph's max level closes its batch
and becomes the entry point.  Levels are the CPU build restatement's (oracle.build_hnsw_batched).
No device needed.

The facts the device tests of the extension rely on (tests/test_gpu_extend.py) are asserted here, not
trusted: which rows raise the max level under the seeds used, and where batches end."""

import numpy as np
import pytest
from build_common import HUB_SEED, SEED, restated

SPEC = ("uniform", 3000, 8, 9)
SCHEDULES = [(0, 0), (1, 1), (2, 64), (64, 0)]


def schedule_ends(levels, start, ep, batch_div, max_batch):
    batch_div, max_batch = batch_div or 16, max_batch or 65536
    n, maxl, i, ends = len(levels), int(levels[ep]), start, []
    while i < n:
        end = min(n, i + max(1, min(max_batch, i // batch_div)))
        for j in range(i, end):
            if levels[j] > maxl:
                end, maxl = j + 1, int(levels[j])
                break
        ends.append(end)
        i = end
    return ends


def entry_point(levels, n0):
    """The entry point of a graph over rows [0, n0): the first row of the highest level."""
    return int(np.argmax(levels[:n0]))


def raises(levels):
    """Row counts just after a row that raised the max level (row 0 aside)."""
    return [j + 1 for j in range(1, len(levels)) if levels[j] > levels[:j].max()]


def levels_of(R, seed):
    return np.ascontiguousarray(restated(SPEC, R=R, seed=seed)[1], np.uint32)


@pytest.mark.parametrize("R,seed", [(32, SEED), (8, SEED), (32, HUB_SEED)])
@pytest.mark.parametrize("batch_div,max_batch", SCHEDULES)
def test_whole_schedule(native, R, seed, batch_div, max_batch):
    lv = levels_of(R, seed)
    ends = native.build_batches(lv, 1, 0, batch_div, max_batch)
    assert ends.dtype == np.uint64
    assert ends.tolist() == schedule_ends(lv, 1, 0, batch_div, max_batch)
    assert ends[-1] == len(lv)
    if max_batch == 1:
        assert ends.tolist() == list(range(2, len(lv) + 1))


@pytest.mark.parametrize("R,batches", [(32, 111), (8, 112)])
def test_batch_count_is_the_restated_builds(native, R, batches):
    ref = restated(SPEC, R=R)
    ends = native.build_batches(np.ascontiguousarray(ref[1], np.uint32), 1, 0, 0, 0)
    assert len(ends) == ref[6]["batches"] == batches


@pytest.mark.parametrize("R,seed", [(32, SEED), (8, SEED), (32, HUB_SEED)])
@pytest.mark.parametrize("batch_div,max_batch", SCHEDULES)
def test_continued_from_a_boundary_is_the_rest_of_the_schedule(native, R, seed, batch_div, max_batch):
    lv = levels_of(R, seed)
    full = native.build_batches(lv, 1, 0, batch_div, max_batch).tolist()
    for at in (0, len(full) // 3, len(full) - 2):
        n0 = full[at]
        rest = native.build_batches(lv, n0, entry_point(lv, n0), batch_div, max_batch).tolist()
        assert rest == full[at + 1:]
        assert rest == schedule_ends(lv, n0, entry_point(lv, n0), batch_div, max_batch)


@pytest.mark.parametrize("batch_div,max_batch", SCHEDULES)
def test_continued_from_mid_batch(native, batch_div, max_batch):
    lv = levels_of(32, SEED)
    for n0 in (1000, 1777):
        ep = entry_point(lv, n0)
        got = native.build_batches(lv, n0, ep, batch_div, max_batch).tolist()
        assert got == schedule_ends(lv, n0, ep, batch_div, max_batch)
        assert got[-1] == len(lv)


def test_facts_the_device_tests_use(native):
    lv = levels_of(32, SEED)
    ends = native.build_batches(lv, 1, 0, 0, 0).tolist()
    assert 116 in raises(lv) and 116 in ends and entry_point(lv, 116) == 115
    assert 1029 in ends and 1093 in ends and 1029 not in raises(lv) and 1093 not in raises(lv)
    hub = levels_of(32, HUB_SEED)
    assert raises(hub) == [8, 938]
    hub_ends = native.build_batches(hub, 1, 0, 0, 0).tolist()
    assert 938 in hub_ends and any(600 <= e < 937 for e in hub_ends)
    r8 = levels_of(8, SEED)
    assert raises(r8)[-1] == 1311 and int(r8.max()) == 5
    assert any(1000 <= e < 1310 for e in native.build_batches(r8, 1, 0, 0, 0).tolist())


def test_count_only_and_refusals(native):
    lv = levels_of(32, SEED)
    assert len(native.build_batches(lv, len(lv), 0, 0, 0)) == 0  # nothing left to schedule
    with pytest.raises(ValueError):
        native.build_batches(lv, 0, 0, 0, 0)  # a graph has at least its first row
    with pytest.raises(ValueError):
        native.build_batches(lv, 5, 5, 0, 0)  # the entry point is a row of the graph
    with pytest.raises(ValueError):
        native.build_batches(lv, len(lv) + 1, 0, 0, 0)
