"""Exact range search without a GPU: the scan's launch plan (alaya_flat_range_plan, pure host arithmetic), the
Python argument checks, and the numpy reference itself on a hand-made case."""

import itertools

import numpy as np
import pytest

import flat_range_common as rc
from alayalite_amd import utils

N_ELIGIBLE = [0, 1, 31, 10 ** 4, 10 ** 6, 10 ** 7]
NQ = [1, 5, 37, 1000, 10 ** 6]
CAPS = [1, 7, 1024, 4096]
STRIDES = [32, 128, 960]
CUS = 256
GRID = list(itertools.product(N_ELIGIBLE, NQ, CAPS, STRIDES))


def _clear(monkeypatch):
    monkeypatch.delenv(rc.CHUNK_ENV, raising=False)
    monkeypatch.delenv(rc.STAGING_ENV, raising=False)


def _check(plan, n, nq, cap, stride, staging_cap):
    rows, chunks, tile, sub, slots, staging = plan
    what = (n, nq, cap, stride, plan)
    assert tile in (4, 8, 16) and rows > 0 and rows % rc.PASS_ROWS == 0, what
    # coverage: the chunks cover the id list without an empty one, the launches cover the queries
    assert chunks * rows >= n and (chunks == 0 or (chunks - 1) * rows < n), what
    assert (chunks == 0) == (n == 0), what
    assert sub > 0 and sub % tile == 0 and -(-nq // sub) * sub >= nq, what
    # a (chunk, query) list is as long as the cap, or the chunk where that is shorter
    assert slots == min(cap, rows), what
    # the staging: lists and counts of one launch, within the cap for any nq
    assert staging == chunks * min(nq, sub) * (slots * 8 + 4) and staging <= staging_cap, what
    # one workgroup's LDS: its queries alone
    assert tile * stride * 4 <= 160 * 1024, what
    return rows, chunks, tile, sub


@pytest.mark.parametrize("forced", [None, 32, 100, 4096])
def test_plan_conditions(native, monkeypatch, forced):
    """Coverage, the 256 MiB staging cap, the tile and chunk rules of the exact filtered scan, forced chunk rows."""
    _clear(monkeypatch)
    if forced is not None:
        monkeypatch.setenv(rc.CHUNK_ENV, str(forced))
    split = 0
    for n, nq, cap, stride in GRID:
        plan = native.flat_range_plan(n, nq, cap, stride, CUS)
        rows, chunks, tile, sub = _check(plan, n, nq, cap, stride, rc.CAP)
        split += sub < nq
        # the tile: 4 / 8 / 16 by the number of queries (these strides fit two workgroups of 16 per CU)
        assert tile == (4 if nq <= 4 else 8 if nq <= 8 else 16), (n, nq, cap, stride, plan)
        q_tiles = -(-nq // tile)
        max_chunks = max(1, 2 * CUS // q_tiles)
        passes = -(-n // rc.PASS_ROWS)
        if forced is None:
            want = rc.PASS_ROWS * max(1, -(-passes // max_chunks))
        else:
            want = -(-forced // rc.PASS_ROWS) * rc.PASS_ROWS
        # honoured wherever one query tile's staging stays under the cap at that chunk size
        if -(-n // want) * tile * (min(cap, want) * 8 + 4) <= rc.CAP:
            assert rows == want, (n, nq, cap, stride, plan)
        else:
            assert rows > want, (n, nq, cap, stride, plan)
        if forced is None:
            assert chunks <= max_chunks, (n, nq, cap, stride, plan)
    assert split > 0  # the grid reaches batches that have to be split


def test_plan_zero_rows_and_tiles(native, monkeypatch):
    _clear(monkeypatch)
    plan = native.flat_range_plan(0, 100, 1024, 128, CUS)
    assert plan[1] == 0 and plan[5] == 0 and plan[3] >= 100
    # wide rows take a smaller tile; rows too wide for four queries are refused
    assert native.flat_range_plan(100, 100, 10, 2048, CUS)[2] == 8
    assert native.flat_range_plan(100, 100, 10, 4096, CUS)[2] == 4
    assert native.flat_range_plan(100, 100, 10, 960, CUS)[2] == 16
    assert native.flat_range_plan(100, 3, 10, 960, CUS)[2] == 4
    with pytest.raises(Exception):
        native.flat_range_plan(100, 10, 10, 1 << 14, CUS)
    for cap in (0, 4097):
        with pytest.raises(Exception):
            native.flat_range_plan(100, 10, cap, 128, CUS)


@pytest.mark.parametrize("staging", [1, 100_000, 1 << 20, 1 << 24])
def test_plan_forced_staging(native, monkeypatch, staging):
    """The staging knob: the cap holds for any nq and C, raised only to what one tile of one chunk needs."""
    _clear(monkeypatch)
    monkeypatch.setenv(rc.STAGING_ENV, str(staging))
    launches = 0
    for n, nq, cap, stride in GRID:
        plan = native.flat_range_plan(n, nq, cap, stride, CUS)
        tile = plan[2]
        _check(plan, n, nq, cap, stride, max(staging, tile * (cap * 8 + 4)))
        launches += -(-nq // plan[3]) > 1
    assert launches > 0
    # the knob and the chunk knob together: 5000 rows in chunks of 64, one tile of 16 per launch
    monkeypatch.setenv(rc.CHUNK_ENV, "64")
    monkeypatch.setenv(rc.STAGING_ENV, str(79 * 16 * (64 * 8 + 4)))
    assert native.flat_range_plan(5000, 17, 256, 16, CUS) == (64, 79, 16, 16, 64, 79 * 16 * 516)


def test_argument_checks():
    """What Index.exact_range_search and calc_range_gt_device refuse before anything reaches the device."""
    radii = utils.exact_range_args(3, 1.5, 10)
    assert radii.dtype == np.float32 and radii.shape == (3,) and (radii == 1.5).all() and radii.flags.c_contiguous
    assert np.array_equal(utils.exact_range_args(3, [1, -np.inf, np.inf], 4096), np.array([1, -np.inf, np.inf], np.float32))
    for bad in ([1.0, 2.0], np.zeros((3, 1)), np.zeros((1, 3))):
        with pytest.raises(ValueError, match="radius"):
            utils.exact_range_args(3, bad, 10)
    for bad in (np.nan, [1.0, np.nan, 2.0]):
        with pytest.raises(ValueError, match="NaN"):
            utils.exact_range_args(3, bad, 10)
    for cap in (0, -1, 4097):
        with pytest.raises(ValueError, match="max_results"):
            utils.exact_range_args(3, 1.0, cap)
    with pytest.raises(ValueError, match="groups needs allow"):
        utils.exact_range_args(3, 1.0, 10, None, np.zeros(3, np.uint32))
    utils.exact_range_args(3, 1.0, 10, np.ones(8, bool), np.zeros(3, np.uint32))
    data, q = np.zeros((8, 4), np.float32), np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="NaN"):
        utils.calc_range_gt_device(data, q, np.nan)
    with pytest.raises(ValueError, match="max_results"):
        utils.calc_range_gt_device(data, q, 1.0, max_results=5000)
    with pytest.raises(ValueError, match="radius"):
        utils.calc_range_gt_device(data, q, [1.0, 2.0])
    with pytest.raises(ValueError, match="allow"):
        utils.calc_range_gt_device(data, q, 1.0, allow=np.ones((2, 8), bool))
    with pytest.raises(ValueError, match="metric"):
        utils.calc_range_gt_device(data, q, 1.0, metric="l1")


def test_reference_on_a_hand_made_case(orc):
    """Points on a line, a tie at the radius, a removed row, a mask, equal distances and truncation."""
    base = np.array([[0], [1], [-1], [2], [-2], [3], [1], [0.5]], np.float32)
    q = np.array([[0.0], [1.0]], np.float32)
    # query 0: squared distances 0 1 1 4 4 9 1 .25; radius 1 takes ids 0 1 2 6 7, the tie at the radius included
    c, i, d = rc.reference(orc, 0, base, q, np.array([1.0, 0.0], np.float32), 8)
    assert c.tolist() == [5, 2]
    assert i[0].tolist() == [0, 7, 1, 2, 6] + [rc.EMPTY] * 3 and d[0].tolist()[:5] == [0.0, 0.25, 1.0, 1.0, 1.0]
    assert i[1].tolist() == [1, 6] + [rc.EMPTY] * 6 and (d[1][2:] == rc.FLT_MAX).all()
    # one ulp below the radius: the three rows at distance 1 are out
    c, i, _ = rc.reference(orc, 0, base, q[:1], np.nextafter(np.float32(1), np.float32(0)), 8)
    assert c.tolist() == [2] and i[0].tolist()[:2] == [0, 7]
    # a removed row and a mask
    valid = np.ones(8, bool)
    valid[1] = False
    allow = np.ones(8, bool)
    allow[7] = False
    c, i, _ = rc.reference(orc, 0, base, q[:1], 1.0, 8, allow, valid)
    assert c.tolist() == [3] and i[0].tolist()[:3] == [0, 2, 6]
    # truncation keeps the smallest ids, then orders them by (distance, id): 0 1 2 -> 0, 1, 2; the nearer 7 is lost
    c, i, d = rc.reference(orc, 0, base, q[:1], 1.0, 3)
    assert c.tolist() == [5] and i[0].tolist() == [0, 1, 2] and d[0].tolist() == [0.0, 1.0, 1.0]
    # IP: equal distances (here zeros, of either sign) order by id; radius -inf takes nothing, +inf everything
    c, i, d = rc.reference(orc, 1, base, np.array([[0.0]], np.float32), 0.0, 8)
    assert c.tolist() == [8] and i[0].tolist() == list(range(8)) and (d[0] == 0).all()
    assert rc.reference(orc, 1, base, q, -np.inf, 4)[0].tolist() == [0, 0]
    assert rc.reference(orc, 1, base, q, np.inf, 4)[0].tolist() == [8, 8]
    # the CSR form
    c, i, d = rc.reference(orc, 0, base, q, np.array([1.0, 0.0], np.float32), 3)
    lims, ci, cd = rc.csr_of(c, i, d, 3)
    assert lims.tolist() == [0, 3, 5] and ci.tolist() == [0, 1, 2, 1, 6]
    lims2, ci2, cd2 = utils.range_csr(c, i, d, 3)
    assert np.array_equal(lims, lims2) and np.array_equal(ci, ci2) and np.array_equal(cd, cd2)
