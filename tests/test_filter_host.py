"""The filtered graph search's restatement (tests/filter_common.py) and the inputs of test_filter_gpu.py,
without a GPU.

The restatement is what the device must equal, so it is pinned first: with an all-ones mask it is the
oracle's own search (ids, distance bits, counters), and its output is the first k of the allowed
computed pairs under a stable sort by distance.  Then the conditions that keep the GPU cases from
being vacuous -- the result pool really holds candidates the traversal pool dropped, comes up short,
outgrows ef, and orders ties by arrival -- and utils.pack_allow."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc


def _post_filter(r, allow, k):
    """What a caller gets by filtering the ef ids a search returns."""
    return [v for v, _ in r["pool"] if allow[v]][:k]


@pytest.mark.parametrize("dim,metric", [(64, 0), (128, 0), (64, 1), (128, 1)])
def test_all_ones_mask_is_the_plain_search(orc, dim, metric):
    base, queries, arrays = fc.graph(orc, dim, metric)
    view = dc.view_of(orc, base, arrays, metric)
    for i, r in enumerate(fc.replays(orc, dim, metric, "gist", 10, 40, 1.0)):
        ids, d, cnt = view.search(queries[i], 10, 40, with_counters=True)
        assert np.array_equal(r["ids"], ids), (i, r["ids"], ids)
        assert np.array_equal(r["dists"].view(np.uint32), d.view(np.uint32)), i
        assert tuple(r["counters"]) == tuple(cnt), (i, r["counters"], cnt)


@pytest.mark.parametrize("dim,metric,kind,k,ef,share", [
    (64, 0, "gist", 10, 40, 0.1), (64, 1, "gist", 10, 40, 0.02), (128, 0, "gist", 65, 10, 0.5),
    (16, 0, "tie", 10, 20, 0.3), (128, 0, "tie", 10, 20, 0.3)])
def test_equals_the_stable_sort_statement(orc, dim, metric, kind, k, ef, share):
    for i, r in enumerate(fc.replays(orc, dim, metric, kind, k, ef, share)):
        ids, d = fc.stable_first_k(r["pairs"], k)
        assert np.array_equal(r["ids"], ids), (i, r["ids"], ids)
        assert np.array_equal(r["dists"].view(np.uint32), d.view(np.uint32)), i


@pytest.mark.parametrize("dim", [64, 100, 128, 960])
@pytest.mark.parametrize("share", [0.1, 0.02])
def test_result_pool_differs_from_post_filtering(orc, dim, share):
    """k = 10, ef = 40: at least 11 of 12 queries return something other than the post-filtered pool."""
    allow = fc.mask(fc.N, share)
    differ = 0
    for r in fc.replays(orc, dim, 0, "gist", 10, 40, share):
        got = [int(v) for v in r["ids"] if v != fc.EMPTY]
        differ += got != _post_filter(r, allow, 10)
    print(dim, share, "queries that differ from the post-filter:", differ)
    assert differ >= 11, (dim, share, differ)


@pytest.mark.parametrize("dim", [64, 100, 128])
def test_some_query_comes_up_short(orc, dim):
    short = sum(int((r["ids"] == fc.EMPTY).any()) for r in fc.replays(orc, dim, 0, "gist", 10, 40, 0.02))
    print(dim, "queries short of k:", short)
    assert short >= 1, (dim, short)


@pytest.mark.parametrize("dim", [64, 100, 128, 960])
def test_result_pool_outgrows_ef(orc, dim):
    """k = 65, ef = 10 at share 0.5 and k = 5, ef = 1 with all ones: every query returns more than ef
    entries; k = 224, ef = 10 with all ones: at least 5 of 12 come up short."""
    for k, ef, share in ((65, 10, 0.5), (5, 1, 1.0)):
        for i, r in enumerate(fc.replays(orc, dim, 0, "gist", k, ef, share)):
            assert int((r["ids"] != fc.EMPTY).sum()) > ef, (dim, k, ef, i)
    short = sum(int((r["ids"] == fc.EMPTY).any()) for r in fc.replays(orc, dim, 0, "gist", 224, 10, 1.0))
    print(dim, "queries short of 224:", short)
    assert short >= 5, (dim, short)


@pytest.mark.parametrize("dim", [8, 16, 128])
def test_tie_rows_order_by_arrival(orc, dim):
    """Share 0.3, k = 10, ef = 20: for at least 9 of 12 queries the output is not the (distance, id)
    order of the allowed pairs, and for some query a tie straddles slot k."""
    k = 10
    differ = straddle = 0
    for r in fc.replays(orc, dim, 0, "tie", k, 20, 0.3):
        by_id = sorted(r["pairs"], key=lambda p: (float(p[1]), p[0]))[:k]
        differ += [int(v) for v in r["ids"] if v != fc.EMPTY] != [v for v, _ in by_id]
        ds = sorted(float(d) for _, d in r["pairs"])
        straddle += len(ds) > k and ds[k - 1] == ds[k]
    print(dim, "queries whose arrival order is not the id order:", differ, "ties across slot k:", straddle)
    assert differ >= 9 and straddle >= 1, (dim, differ, straddle)


# ---- utils.pack_allow ------------------------------------------------------------------------------
def test_pack_allow_bit_layout():
    from alayalite_amd.utils import pack_allow

    n = 70
    allow = np.zeros(n, bool)
    allow[[0, 1, 31, 32, 69]] = True
    w = pack_allow(allow, n)
    assert w.dtype == np.uint32 and w.shape == (1, 3) and w.flags.c_contiguous
    assert w[0].tolist() == [(1 << 0) | (1 << 1) | (1 << 31), 1 << 0, 1 << 5]
    for i in range(n):
        assert bool((w[0, i >> 5] >> (i & 31)) & 1) == bool(allow[i])


def test_pack_allow_padding_shape_and_dtypes():
    from alayalite_amd.utils import pack_allow

    rng = np.random.default_rng(7)
    for n in (1, 31, 32, 33, 64, 2000):
        a = rng.random((3, n)) < 0.5
        w = pack_allow(a, n)
        assert w.shape == (3, (n + 31) // 32) and w.dtype == np.uint32
        bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")
        assert np.array_equal(bits[:, :n].astype(bool), a)
        assert not bits[:, n:].any()  # padding bits zero
        for other in (a.astype(np.uint8), a.astype(np.int64), a.astype(np.float32)):
            assert np.array_equal(pack_allow(other, n), w)
    ones = pack_allow(np.ones(33, bool), 33)
    assert ones.tolist() == [[0xFFFFFFFF, 1]]
    assert pack_allow(np.zeros(0, bool), 0).shape == (1, 0)


def test_pack_allow_range_errors():
    from alayalite_amd.utils import pack_allow

    with pytest.raises(ValueError):
        pack_allow(np.ones(10, bool), 11)
    with pytest.raises(ValueError):
        pack_allow(np.ones((2, 12), bool), 11)
    with pytest.raises(ValueError):
        pack_allow(np.ones((2, 3, 4), bool), 4)
    with pytest.raises(ValueError):
        pack_allow(np.ones((0, 4), bool), 4)
    with pytest.raises(ValueError):
        pack_allow(np.ones(4, bool), -1)
