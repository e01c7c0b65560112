"""Index.exact_range_search: the exact range scan behind the public interface, on f32 and SQ8 indexes, after
remove and add, with both id types; against flat_range_common.reference (array_equal on counts, ids and distance
bits), against range_search (whose hits are a subset) and against exact_search (whose answer is a prefix)."""

import numpy as np
import pytest

import alayalite_amd
import flat_filtered_common as fc
import flat_range_common as rc

pytestmark = pytest.mark.gpu

N0, N1, DIM, NQ = 1000, 1200, 40, 9
CAP = 256


def _rows():
    rng = np.random.default_rng(2222)
    return rng.standard_normal((N1, DIM)).astype(np.float32), rng.standard_normal((NQ, DIM)).astype(np.float32)


def _check(orc, index, m, stored, qn, queries, valid, id_type, radius_m, allow=None, groups=None, cap=CAP, chunk=None):
    """Index.exact_range_search at each query's radius_m-th eligible distance against the reference over `stored`
    (the rows as the index holds them) and `qn` (the queries as it prepares them)."""
    n = len(stored)
    every = fc.distances(orc, min(m, 1), stored, qn, np.arange(n))
    masks = np.ones((1, n), bool) if allow is None else np.atleast_2d(allow)
    g = np.zeros(NQ, np.int64) if groups is None else groups
    radii = np.array([np.sort(every[a][masks[g[a]] & valid])[radius_m - 1] for a in range(NQ)], np.float32)
    ref_c, ref_i, ref_d = rc.reference(orc, min(m, 1), stored, qn, radii, cap, allow, valid, groups)
    lims, ids, dists, counts = index.exact_range_search(queries.copy(), radii, cap, allow=allow, groups=groups, _chunk=chunk)
    assert ids.dtype == id_type and dists.dtype == np.float32 and counts.dtype == np.uint32 and lims.dtype == np.int64
    ref_lims, csr_i, csr_d = rc.csr_of(ref_c, ref_i, ref_d, cap)
    assert np.array_equal(counts, ref_c) and (counts >= radius_m).all()
    assert np.array_equal(lims, ref_lims)
    assert np.array_equal(ids, csr_i.astype(id_type))
    assert np.array_equal(dists.view(np.uint32), csr_d.view(np.uint32))
    return radii


@pytest.mark.parametrize("metric,id_type,quant", [("l2", np.uint32, "none"), ("ip", np.uint64, "none"),
                                                  ("cosine", np.uint32, "none"), ("l2", np.uint64, "sq8")])
def test_index_exact_range_search(orc, metric, id_type, quant):
    """After fit, after remove (f32 indexes: an SQ8 index refuses remove) and after add; with one mask, with groups,
    and with the queries chunked."""
    base, queries = _rows()
    m = {"l2": 0, "ip": 1, "cosine": 2}[metric]
    stored = np.stack([orc.normalize(r) for r in base]) if m == 2 else base
    qn = np.stack([orc.normalize(r) for r in queries]) if m == 2 else queries
    client = alayalite_amd.Client()
    index = client.create_index(f"xr_{metric}_{quant}", capacity=N1, metric=metric, id_type=id_type,
                                quantization_type=quant)
    index.fit(base[:N0].copy(), ef_construction=60)
    valid = np.ones(N0, bool)
    _check(orc, index, m, stored[:N0], qn, queries, valid, id_type, 30)
    allow = fc.random_mask(N0, 0.5, 3)
    _check(orc, index, m, stored[:N0], qn, queries, valid, id_type, 30, allow)
    # a scalar radius, and truncation: counts stay exact, the list holds the smallest ids
    lims, ids, dists, counts = index.exact_range_search(queries.copy(), np.inf, 7)
    assert (counts == N0).all() and np.array_equal(np.diff(lims), np.full(NQ, 7))
    assert np.array_equal(np.sort(ids.reshape(NQ, 7), axis=1), np.tile(np.arange(7, dtype=id_type), (NQ, 1)))
    # removed rows, some of them hits of the first query
    lims, ids, _, _ = index.exact_range_search(queries.copy(), _check(orc, index, m, stored[:N0], qn, queries, valid,
                                                                      id_type, 30), CAP)
    gone = [] if quant == "sq8" else [int(v) for v in ids[:3]] + [0, 999]  # (an SQ8 index has no remove)
    for v in gone:
        index.remove(v)
    valid[gone] = False
    _check(orc, index, m, stored[:N0], qn, queries, valid, id_type, 30)
    lims, ids, _, counts = index.exact_range_search(queries.copy(), np.inf, 4096)
    assert (counts == valid.sum()).all() and not np.isin(ids, gone).any()
    # rows added in bulk
    new_ids = index.add(base[N0:].copy())
    assert len(new_ids) == N1 - N0
    valid = np.concatenate([valid, np.ones(N1 - N0, bool)])
    _check(orc, index, m, stored, qn, queries, valid, id_type, 30)
    allow = np.stack([fc.random_mask(N1, 0.5, 4), fc.random_mask(N1, 0.2, 5), np.ones(N1, bool)])
    groups = np.arange(NQ) % 3
    _check(orc, index, m, stored, qn, queries, valid, id_type, 30, allow, groups, chunk=4)
    with pytest.raises(ValueError, match="groups needs allow"):
        index.exact_range_search(queries.copy(), 1.0, groups=groups)
    with pytest.raises(ValueError, match="max_results"):
        index.exact_range_search(queries.copy(), 1.0, 4097)
    with pytest.raises(ValueError, match="NaN"):
        index.exact_range_search(queries.copy(), np.nan)


def _f32_index():
    def make():
        base, queries = _rows()
        index = alayalite_amd.Client().create_index("xr_subset", capacity=N1)
        index.fit(base.copy(), ef_construction=60)
        return index
    return fc.cached(("xr-subset-index",), make)


@pytest.mark.parametrize("expand", ["fixed", "radius"])
def test_graph_range_hits_are_a_subset(expand):
    """Without truncation the hits of range_search at the same radius are among the exact hits, with equal
    distance bits per id."""
    base, queries = _rows()
    index = _f32_index()
    _, d10 = index.exact_search(queries.copy(), 50)
    radii = d10[:, -1].copy()
    lims, ids, dists, counts = index.exact_range_search(queries.copy(), radii, 1024)
    g_lims, g_ids, g_dists, g_counts = index.range_search(queries.copy(), radii, 64, 1024, expand=expand)
    assert (counts <= 1024).all() and (g_counts <= counts).all() and g_counts.sum() > 0
    for a in range(NQ):
        exact = dict(zip(ids[lims[a]:lims[a + 1]].tolist(), dists[lims[a]:lims[a + 1]].view(np.uint32).tolist()))
        got = dict(zip(g_ids[g_lims[a]:g_lims[a + 1]].tolist(), g_dists[g_lims[a]:g_lims[a + 1]].view(np.uint32).tolist()))
        assert set(got) <= set(exact) and all(exact[i] == b for i, b in got.items()), a


@pytest.mark.parametrize("metric", ["l2", "ip", "cos"])
def test_calc_range_gt_device(orc, metric):
    """The same call on raw arrays, with a mask: int32 ids, range_search's form."""
    from alayalite_amd.utils import calc_range_gt_device

    base, queries = _rows()
    m = {"l2": 0, "ip": 1, "cos": 2}[metric]
    stored = np.stack([orc.normalize(r) for r in base]) if m == 2 else base
    qn = np.stack([orc.normalize(r) for r in queries]) if m == 2 else queries
    allow = fc.random_mask(N1, 0.4, 8)
    rows = np.nonzero(allow)[0]
    dist = fc.distances(orc, min(m, 1), stored, qn, rows)
    radii = np.sort(dist, axis=1)[:, 39].copy()
    ref_c, ref_i, ref_d = rc.from_distances(rows, dist, radii, 32)  # 40 hits under a cap of 32: truncated
    ref_lims, csr_i, csr_d = rc.csr_of(ref_c, ref_i, ref_d, 32)
    lims, ids, dists, counts = calc_range_gt_device(base, queries, radii, 32, metric=metric, allow=allow)
    assert ids.dtype == np.int32 and (counts >= 40).all()
    assert np.array_equal(counts, ref_c) and np.array_equal(lims, ref_lims) and np.array_equal(ids, csr_i.astype(np.int32))
    assert np.array_equal(dists.view(np.uint32), csr_d.view(np.uint32))


def test_exact_search_is_a_prefix():
    """With the radius at exact_search's k-th distance the first k of each list are exact_search's answer
    wherever that distance is not tied."""
    base, queries = _rows()
    index = _f32_index()
    k = 10
    e_ids, e_d = index.exact_search(queries.copy(), k + 1)
    lims, ids, dists, counts = index.exact_range_search(queries.copy(), e_d[:, k - 1].copy(), 64)
    untied = e_d[:, k - 1] != e_d[:, k]
    assert untied.any() and (counts >= k).all()
    for a in np.nonzero(untied)[0]:
        assert counts[a] == k
        assert np.array_equal(ids[lims[a]:lims[a] + k], e_ids[a, :k])
        assert np.array_equal(dists[lims[a]:lims[a] + k].view(np.uint32), e_d[a, :k].view(np.uint32))
