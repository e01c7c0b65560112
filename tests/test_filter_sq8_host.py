"""The filtered SQ8 search's restatement (tests/filter_sq8_common.py), the inputs of test_filter_sq8_gpu.py
and sharded.shard_allow_words, without a GPU.

The restatement is what the device must equal, so it is pinned first: with an all-ones mask its traversal is
the oracle's own SQ8 search (pool ids, distance bits, counters), and its candidate pool is the stable first m,
by code distance, of the allowed valid pairs in arrival order.  Then the conditions that keep the GPU cases
from being vacuous: the rerank changes the answer's set and order, m > k buys candidates, ties order by id
where the pool ordered them by arrival, and some queries come up short."""

import numpy as np
import pytest

import filter_common as fc
import filter_sq8_common as sc


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("dim,metric", [(64, 0), (100, 0), (128, 1), (768, 1), (960, 0)])
def test_all_ones_mask_is_the_sq8_search(orc, dim, metric, order):
    base, queries, arrays, quant = sc.inputs(orc, dim, metric)
    view = sc.view_of(orc, base, arrays, metric, quant, order)
    ef = 40
    for i, r in enumerate(sc.replays(orc, dim, metric, "gist", order, 10, ef, ef, 1.0)):
        ids, d, cnt = view.search(queries[i], ef, ef, with_counters=True)
        size = len(r["pool"])
        assert np.array_equal(np.array([v for v, _ in r["pool"]], np.uint32), ids[:size]), (i, r["pool"], ids)
        assert np.array_equal(np.array([x for _, x in r["pool"]], np.float32).view(np.uint32), d[:size].view(np.uint32)), i
        assert tuple(r["counters"]) == tuple(cnt), (i, r["counters"], cnt)
        assert r["cand"] == r["pool"]  # m = ef and every row allowed: the two pools are one


@pytest.mark.parametrize("dim,metric,kind,k,ef,m,share", [
    (64, 0, "coarse", 10, 40, 40, 0.1), (64, 0, "coarse", 10, 40, 224, 0.5), (128, 1, "gist", 65, 10, 224, 0.5),
    (16, 0, "tie", 10, 20, 40, 0.3), (128, 0, "tie", 10, 20, 40, 0.3)])
def test_candidate_pool_is_the_stable_first_m(orc, dim, metric, kind, k, ef, m, share):
    for i, r in enumerate(sc.replays(orc, dim, metric, kind, 2, k, ef, m, share)):
        ids, d = fc.stable_first_k(r["pairs"], m)
        size = len(r["cand"])
        assert size == min(m, len(r["pairs"]))
        assert [v for v, _ in r["cand"]] == [int(v) for v in ids[:size]], i
        assert np.array_equal(np.array([x for _, x in r["cand"]], np.float32).view(np.uint32), d[:size].view(np.uint32)), i


def _set_and_order(rs, k):
    """Queries whose reranked ids differ from the candidate pool's first k: as a set, and in order."""
    in_set = in_order = 0
    for r in rs:
        got = [int(v) for v in r["ids"] if v != sc.EMPTY]
        head = [v for v, _ in r["cand"]][:k]
        in_set += set(got) != set(head)
        in_order += got != head
    return in_set, in_order


def test_coarse_codes_make_the_rerank_matter(orc):
    """coarse, d 64 L2.  (k, ef, m, share) = (10, 40, 40, 0.1): 5 of 12 queries measured with another id set
    than the pool's first k and 12 with another order; m = 10 can only reorder; (10, 40, 224, 0.5): 7 in set."""
    in_set, in_order = _set_and_order(sc.replays(orc, 64, 0, "coarse", 2, 10, 40, 40, 0.1), 10)
    print("m 40 share 0.1: set", in_set, "order", in_order)
    assert in_set >= 3 and in_order >= 8, (in_set, in_order)
    in_set10, in_order10 = _set_and_order(sc.replays(orc, 64, 0, "coarse", 2, 10, 40, 10, 0.1), 10)
    print("m 10 share 0.1: set", in_set10, "order", in_order10)
    assert in_set10 == 0, (in_set10, in_order10)  # m = k: the rerank keeps the set (no query is short here)
    in_set224, _ = _set_and_order(sc.replays(orc, 64, 0, "coarse", 2, 10, 40, 224, 0.5), 10)
    print("m 224 share 0.5: set", in_set224)
    assert in_set224 >= 3, in_set224


@pytest.mark.parametrize("dim", [16, 128])
def test_tie_rows_order_by_id_after_the_rerank(orc, dim):
    """tie, (10, 20, 40, 0.3): on at least 8 of 12 queries the (exact distance, id) order of the candidates is
    not their (exact distance, arrival) order -- the rerank's tie rule shows."""
    base = sc.inputs(orc, dim, 0, "tie")[0]
    _, queries = sc.rows(dim, "tie")
    differ = 0
    for q, r in zip(queries, sc.replays(orc, dim, 0, "tie", 2, 10, 20, 40, 0.3)):
        exact = [float(orc.dist(0, q, base[v])) for v, _ in r["cand"]]
        by_arrival = sorted(range(len(exact)), key=lambda i: (exact[i], i))[:10]
        got = [int(v) for v in r["ids"] if v != sc.EMPTY]
        differ += got != [r["cand"][i][0] for i in by_arrival]
    print(dim, "queries where (distance, id) differs from (distance, arrival):", differ)
    assert differ >= 8, (dim, differ)


def test_some_queries_come_up_short(orc):
    short = sum(int((r["ids"] == sc.EMPTY).any()) for r in sc.replays(orc, 64, 0, "gist", 2, 10, 40, 40, 0.02))
    print("queries short of k:", short)
    assert short >= 3, short


# ---- sharded.shard_allow_words -------------------------------------------------------------------------
def test_shard_allow_words_is_pack_allow_of_the_slice():
    from alayalite_amd.sharded import shard_allow_words
    from alayalite_amd.utils import pack_allow

    rng = np.random.default_rng(5)
    n = 4000
    one = rng.random(n) < 0.3
    three = rng.random((3, n)) < 0.5
    for lo, hi in ((0, n), (0, 2000), (2000, n), (37, 1001), (1, 2), (33, 97), (500, 500), (n, n)):
        for allow in (one, three):
            w = shard_allow_words(allow, lo, hi)
            assert w.dtype == np.uint32 and w.shape == (allow.shape[0] if allow.ndim == 2 else 1, (hi - lo + 31) // 32)
            assert np.array_equal(w, pack_allow(allow[..., lo:hi], hi - lo)), (lo, hi, allow.ndim)
            rows = np.atleast_2d(allow)
            for g in range(rows.shape[0]):
                for i in (0, 1, 31, 32, hi - lo - 1):
                    if 0 <= i < hi - lo:
                        assert bool((w[g, i >> 5] >> (i & 31)) & 1) == bool(rows[g, lo + i]), (lo, hi, g, i)
    for lo, hi in ((-1, 5), (5, 4), (0, n + 1)):
        with pytest.raises(ValueError):
            shard_allow_words(one, lo, hi)
