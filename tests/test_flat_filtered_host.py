"""Exact filtered k-NN without a GPU: the scan's launch plan (alaya_flat_filtered_plan, pure host
arithmetic), a check on the reference alone that the inputs of test_flat_filtered.py reach the paths
they are meant for, and the equivalence of the two ways to state the answer."""

import itertools

import numpy as np
import pytest

import flat_filtered_common as fc
from flat_common import exact as exact_l2
from flat_ip_common import exact_ip

N_ALLOWED = [0, 1, 31, 10 ** 4, 10 ** 6, 10 ** 7]
NQ = [1, 37, 1000, 10 ** 6]
KS = [1, 10, 224]
STRIDES = [32, 128, 960]
CUS = 256
GRID = list(itertools.product(N_ALLOWED, NQ, KS, STRIDES))


def _check(plan, n_allowed, nq, k, stride):
    rows, chunks, tile, sub, part = plan
    what = (n_allowed, nq, k, stride, plan)
    assert tile in (4, 8, 16) and rows > 0 and rows % fc.PASS_ROWS == 0, what
    # coverage: the chunks cover the id list without an empty one, the launches cover the queries
    assert chunks * rows >= n_allowed and (chunks == 0 or (chunks - 1) * rows < n_allowed), what
    assert sub > 0 and sub % tile == 0, what
    launches = -(-nq // sub)
    assert launches * sub >= nq, what
    # the cap, for any nq
    assert part == chunks * min(nq, sub) * k * 8 and part <= fc.CAP, what
    # one workgroup's LDS: its queries and their lists
    assert tile * (stride * 4 + k * 8) <= 160 * 1024, what
    return rows, chunks, tile, sub


@pytest.mark.parametrize("forced", [None, 32, 100, 4096])
def test_plan_conditions(native, monkeypatch, forced):
    """Coverage, the 256 MiB cap, the chunk-count bound and forced chunk rows, on the grid."""
    if forced is None:
        monkeypatch.delenv("ALAYA_FLAT_FILTER_CHUNK_ROWS", raising=False)
    else:
        monkeypatch.setenv("ALAYA_FLAT_FILTER_CHUNK_ROWS", str(forced))
    split = 0
    for n_allowed, nq, k, stride in GRID:
        plan = native.flat_filtered_plan(n_allowed, nq, k, stride, CUS)
        rows, chunks, tile, sub = _check(plan, n_allowed, nq, k, stride)
        split += sub < nq
        if forced is None:
            # no more chunks than fill the CUs twice over at this tile
            q_tiles = -(-nq // tile)
            assert chunks <= max(1, -(-2 * CUS // q_tiles)), (n_allowed, nq, k, stride, plan)
        else:
            want = -(-forced // fc.PASS_ROWS) * fc.PASS_ROWS
            # honoured wherever one query tile's lists stay under the cap at that chunk size
            if -(-n_allowed // want) * tile * k * 8 <= fc.CAP:
                assert rows == want, (n_allowed, nq, k, stride, plan)
            else:
                assert rows > want
    assert split > 0  # the grid reaches batches that have to be split


def test_plan_rejects_bad_arguments(native, monkeypatch):
    monkeypatch.delenv("ALAYA_FLAT_FILTER_CHUNK_ROWS", raising=False)
    for k in (0, 225):
        with pytest.raises(Exception):
            native.flat_filtered_plan(100, 10, k, 128, CUS)
    with pytest.raises(Exception):  # four queries of such rows do not fit a CU's LDS
        native.flat_filtered_plan(100, 10, 10, 1 << 14, CUS)
    # wide rows take a smaller tile instead
    assert native.flat_filtered_plan(100, 100, 10, 2048, CUS)[2] == 8
    assert native.flat_filtered_plan(100, 100, 10, 960, CUS)[2] == 16
    assert native.flat_filtered_plan(100, 3, 10, 960, CUS)[2] == 4


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", fc.TIE_KINDS)
def test_tie_inputs_tie_across_chunks_and_across_the_mask(orc, kind, metric):
    """With chunks of one wave pass (32 id-list entries) the tie inputs put equal distances on both
    sides of a chunk boundary inside the answer, and on allowed and disallowed rows."""
    base, q, allow = fc.tie_input(kind)
    rows = np.nonzero(allow)[0]
    dist = fc.cached(("tie-dist", kind, metric), lambda: fc.distances(orc, metric, base, q, np.arange(len(base))))
    across_chunks = across_mask = 0
    for a in range(len(q)):
        d = dist[a][rows]
        o = np.lexsort((rows, d))[:fc.TIE_K]
        for v in np.unique(d[o]):
            pos = np.nonzero(d == v)[0]  # positions in the id list
            across_chunks += len(np.unique(pos // fc.PASS_ROWS)) > 1
            across_mask += ((dist[a] == v) & ~allow).any()
    assert across_chunks > 0 and across_mask > 0, (across_chunks, across_mask)


def test_short_and_padding_inputs():
    base, q, allow = fc.short_input()
    assert allow.sum() == 9 < 10
    n = 2001
    words = fc.padding_words(n, np.zeros(n, bool))
    assert words.shape == (1, 63) and words[0, -1] == 0xFFFFFFFF << (n % 32) & 0xFFFFFFFF and words[0, -1] != 0
    assert (words[0, :-1] == 0).all()


@pytest.mark.parametrize("metric", [0, 1])
def test_reference_equals_the_unmasked_reference_over_the_sub_base(orc, metric):
    """The reference over (base, allow) is flat_common.exact / flat_ip_common.exact_ip over base[rows]
    with ids mapped through rows."""
    base, q = fc.gist_rows(600, 5, 40)
    allow = fc.random_mask(len(base), 0.3, 21)
    rows = np.nonzero(allow)[0]
    k = 10
    ref_i, ref_d = fc.reference(orc, metric, base, q, k, allow)
    sub = np.ascontiguousarray(base[rows])
    sub_i, sub_d = exact_l2(orc, sub, q, k) if metric == 0 else exact_ip(orc, sub, q, k)
    assert np.array_equal(ref_i, rows[sub_i].astype(np.uint32))
    assert np.array_equal(ref_d.view(np.uint32), sub_d.view(np.uint32))
    # fewer allowed rows than k: empty slots in both
    few = np.zeros(len(base), bool)
    few[[5, 17, 300]] = True
    ref_i, ref_d = fc.reference(orc, metric, base, q, k, few)
    sub = np.ascontiguousarray(base[[5, 17, 300]])
    sub_i, sub_d = exact_l2(orc, sub, q, k) if metric == 0 else exact_ip(orc, sub, q, k)
    assert (ref_i[:, 3:] == fc.EMPTY).all() and np.array_equal(ref_i[:, :3], np.array([5, 17, 300], np.uint32)[sub_i[:, :3]])
    assert np.array_equal(ref_d.view(np.uint32), sub_d.view(np.uint32))
