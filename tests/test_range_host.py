"""The range search's restatement (tests/range_common.py) and the inputs of test_range_gpu.py, without a GPU.

The restatement is filter_common's replay read another way, so what is pinned here is that the inputs
reach the paths the GPU cases are about: how many pairs a query offers (the append list's length at
radius FLT_MAX: above every cap below 4096 that the GPU cases use, below 4096 itself), how many of them
tie, that the all-zero IP query offers nothing but -0.0, and that cap 2 is straddled by one append.  The
figures were measured with the oracle on these inputs.  Then utils.range_csr."""

import numpy as np
import pytest

import filter_common as fc
import range_common as rc


def _pair_counts(rs):
    return [len(r["pairs"]) for r in rs]


def _equal_neighbours(r):
    ds = sorted(float(d) for _, d in r["pairs"])
    return sum(a == b for a, b in zip(ds, ds[1:]))


@pytest.mark.parametrize("dim,metric,ef,lo,hi", [(64, 0, 40, 448, 553), (64, 1, 40, 428, 569), (960, 0, 40, 577, 657),
                                                 (64, 0, 1, 13, 98)])
def test_pairs_per_query(orc, dim, metric, ef, lo, hi):
    n = _pair_counts(rc.replays(orc, dim, metric, "gist", ef))
    print(dim, metric, ef, "pairs per query:", min(n), "to", max(n))
    assert min(n) == lo and max(n) == hi, (dim, metric, ef, min(n), max(n))


@pytest.mark.parametrize("dim,lo,hi,tlo,thi", [(16, 266, 336, 241, 316), (128, 444, 558, 373, 485)])
def test_tie_rows_tie(orc, dim, lo, hi, tlo, thi):
    rs = rc.replays(orc, dim, 0, "tie", 20)
    n = _pair_counts(rs)
    ties = [_equal_neighbours(r) for r in rs]
    print(dim, "pairs:", min(n), "to", max(n), "equal neighbours:", min(ties), "to", max(ties))
    assert min(n) == lo and max(n) == hi, (dim, min(n), max(n))
    assert min(ties) == tlo and max(ties) == thi, (dim, min(ties), max(ties))


def test_all_zero_ip_query_measures_minus_zero(orc):
    r = rc.zero_query_replay(orc)
    assert len(r["pairs"]) == 544
    bits = np.array([d for _, d in r["pairs"]], np.float32).view(np.uint32)
    assert (bits == 0x80000000).all()
    # +0.0 and -0.0 as radius both take them all; the largest negative number takes none
    assert len(rc.hits(r, 0.0)) == len(rc.hits(r, -0.0)) == 544 and not rc.hits(r, -1e-30)


@pytest.mark.parametrize("dim,metric", [(64, 0), (64, 1), (100, 0), (128, 0), (128, 1), (960, 0)])
def test_cap_two_is_straddled_by_one_append(orc, dim, metric):
    """Radius FLT_MAX, cap 2: the entry is hit 1, and the entry's first expansion offers at least two more at
    once, so that append begins below the cap and ends past it."""
    _, _, arrays = fc.graph(orc, dim, metric)
    l0 = arrays[0]
    for i, r in enumerate(rc.replays(orc, dim, metric, "gist", 40)):
        entry = r["pairs"][0][0]
        fresh = [int(v) for v in l0[entry] if v != fc.EMPTY and v != entry]
        assert len(set(fresh)) >= 2, (dim, metric, i, fresh)
        assert [v for v, _ in r["pairs"][1:1 + len(fresh)]] == fresh, (dim, metric, i)
        n, ids, _ = rc.want_row(r, fc.FLT_MAX, 2)
        assert n == len(r["pairs"]) and set(ids.tolist()) == {entry, fresh[0]}


def test_restatement_on_a_hand_made_stream():
    r = dict(pairs=[(7, np.float32(2.0)), (3, np.float32(-0.0)), (9, np.float32(0.0)), (1, np.float32(2.0)),
                    (5, np.float32(1.0)), (2, np.float32(0.5))])
    n, ids, d = rc.want_row(r, 2.0, 8)
    assert n == 6 and ids.tolist() == [3, 9, 2, 5, 1, 7] + [fc.EMPTY] * 2
    assert d.view(np.uint32)[0] == 0x80000000 and d.view(np.uint32)[1] == 0 and (d[6:] == fc.FLT_MAX).all()
    n, ids, d = rc.want_row(r, 2.0, 4)  # truncated: the first four to arrive, not the four nearest
    assert n == 6 and ids.tolist() == [3, 9, 1, 7]
    n, ids, d = rc.want_row(r, np.nextafter(np.float32(2.0), np.float32(-np.inf)), 4)
    assert n == 4 and ids.tolist() == [3, 9, 2, 5]
    assert rc.want_row(r, np.nextafter(np.float32(-0.0), np.float32(-np.inf)), 4)[0] == 0


# ---- utils.range_csr -------------------------------------------------------------------------------
def test_range_csr():
    from alayalite_amd.utils import range_csr

    cap = 3
    counts = np.array([2, 0, 5, 3], np.uint32)  # a short list, an empty one, a truncated one, a full one
    ids = np.array([[4, 8, fc.EMPTY], [fc.EMPTY] * 3, [1, 2, 3], [6, 5, 7]], np.uint32)
    dists = np.array([[.1, .2, fc.FLT_MAX], [fc.FLT_MAX] * 3, [.3, .4, .5], [.6, .7, .8]], np.float32)
    lims, out_ids, out_d = range_csr(counts, ids, dists, cap)
    assert lims.dtype == np.int64 and lims.tolist() == [0, 2, 2, 5, 8]
    assert (np.diff(lims) >= 0).all() and (np.diff(lims) == np.minimum(counts, cap)).all()
    assert out_ids.dtype == np.uint32 and out_ids.tolist() == [4, 8, 1, 2, 3, 6, 5, 7]
    assert out_d.dtype == np.float32 and np.array_equal(out_d, np.array([.1, .2, .3, .4, .5, .6, .7, .8], np.float32))
    wide = range_csr(counts, ids.astype(np.uint64), dists, cap)[1]
    assert wide.dtype == np.uint64 and wide.tolist() == out_ids.tolist()
    lims0, ids0, d0 = range_csr(np.zeros(0, np.uint32), np.zeros((0, cap), np.uint32), np.zeros((0, cap), np.float32), cap)
    assert lims0.tolist() == [0] and ids0.size == 0 and d0.size == 0
    with pytest.raises(ValueError):
        range_csr(counts, ids, dists, cap + 1)
    with pytest.raises(ValueError):
        range_csr(counts[:3], ids, dists, cap)
