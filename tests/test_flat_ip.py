"""Flat exact k-NN for the IP and COS metrics, calc_gt_device(metric=...) and Index.exact_search.
Contract: the k smallest rows by the reference's inner-product distance -(q.b) (the ip_sqr_avx2
order, bit-identical to the oracle's orc_ip_f32) with ties broken by id; COS is IP on rows and
queries the caller normalised."""

import numpy as np
import pytest

from flat_common import FLAT_MODES, apply_flat_mode, assert_exact, contraction_of, device_search
from flat_common import exact as exact_l2
from flat_ip_common import exact_ip

pytestmark = pytest.mark.gpu
L2, IP, COS = 0, 1, 2


@pytest.fixture(params=FLAT_MODES)
def flat_mode(request, monkeypatch):
    """Every shortlist contraction and scan (flat_common.apply_flat_mode)."""
    return apply_flat_mode(monkeypatch, request.param)


_cache = {}


def _cached(key, make):
    """Inputs and references are computed once and shared by the modes (never modified)."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _input(orc, n, d, nq, k, kind):
    def make():
        rng = np.random.default_rng(n + d + (0 if kind == "uniform" else 1))
        if kind == "uniform":
            base, q = rng.random((n, d), dtype=np.float32), rng.random((nq, d), dtype=np.float32)
        else:  # centred: inner products of both signs, cutoffs and thresholds straddle zero
            base, q = rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((nq, d), dtype=np.float32)
        base, q = np.ascontiguousarray(base), np.ascontiguousarray(q)
        return (base, q) + exact_ip(orc, base, q, k)

    return _cached((n, d, nq, k, kind), make)


def _check(native, orc, mode, n, d, nq, k, kind, no_flags):
    base, q, ref_i, ref_d = _input(orc, n, d, nq, k, kind)
    dev = native.DeviceIndex(0)
    dev.set_base(base, IP)
    ids, dists, redo = dev.flat_search(q, k)
    ids_d, dists_d, flags = device_search(dev, q, k)
    print(f"flat ip: mode={mode} shape={(n, d, nq, k)} {kind} device_flagged={int(flags.sum())}/{nq} redo={redo}")
    assert_exact(ids, dists, ref_i, ref_d, what="flat_search")
    assert_exact(ids_d, dists_d, ref_i, ref_d, rows=flags == 0, what="flat_search_device, unflagged")
    if no_flags:
        assert int(flags.sum()) == 0 and redo == 0
    return dev


@pytest.mark.parametrize("kind", ["uniform", "gauss"])
@pytest.mark.parametrize("n,d,nq", [(5000, 128, 37), (3000, 32, 130), (2500, 100, 9), (4000, 200, 64)])
def test_flat_ip_exact(native, orc, flat_mode, n, d, nq, kind):
    """Narrow rows in all eight modes: flat_search is exact, the device entry is exact on every
    unflagged query, and on the centred Gaussian input nothing is flagged."""
    dev = _check(native, orc, flat_mode, n, d, nq, 10, kind, no_flags=kind == "gauss")
    if kind == "gauss":  # no rerun: the contraction is the mode's
        assert dev.flat_contraction() == contraction_of(flat_mode, d)


@pytest.mark.parametrize("mode", ["f16", "f32"])
@pytest.mark.parametrize("n,d,nq", [(3000, 256, 20), (2500, 300, 17), (3000, 768, 12), (2000, 960, 10)])
def test_flat_ip_exact_wide_rows(native, orc, monkeypatch, mode, n, d, nq):
    """The slabbed wide scan (default mode: the split; and the f32 form)."""
    apply_flat_mode(monkeypatch, mode)
    _check(native, orc, mode, n, d, nq, 10, "gauss", no_flags=False)


@pytest.mark.parametrize("n,d,nq,k", [(6000, 128, 20, 50), (6000, 128, 9, 100), (5000, 64, 7, 224)])
def test_flat_ip_exact_large_k(native, orc, monkeypatch, n, d, nq, k):
    """The big merge (128- and 256-entry lists), default mode."""
    apply_flat_mode(monkeypatch, "f16")
    _check(native, orc, "f16", n, d, nq, k, "gauss", no_flags=False)


def test_flat_ip_ties_and_fallback(native, monkeypatch):
    """Identical rows: every distance ties, so the shortlist bound cannot be proven -- the host
    recomputes exhaustively and the answer is ids 0..k-1 (ties by id)."""
    apply_flat_mode(monkeypatch, "f16")
    rng = np.random.default_rng(1)
    base = np.tile(rng.random(64, dtype=np.float32), (600, 1))
    q = rng.random((3, 64), dtype=np.float32)
    dev = native.DeviceIndex(0)
    dev.set_base(base, IP)
    ids, dists, redo = dev.flat_search(q, 10)
    assert redo == 3
    assert (ids == np.arange(10, dtype=np.uint32)).all()


def test_flat_metric_change_rebuilds_tile_records(native, orc, monkeypatch):
    """One DeviceIndex, the same rows set as L2, then IP, then L2 again: the cached f16 tile records
    carry the metric's bias, and each search is exact for the metric it runs under."""
    apply_flat_mode(monkeypatch, "f16")
    base, q, ip_i, ip_d = _input(orc, 3000, 32, 130, 10, "uniform")
    l2_i, l2_d = _cached("metric-change-l2", lambda: exact_l2(orc, base, q, 10))
    dev = native.DeviceIndex(0)
    for metric in (L2, IP, L2, IP):
        dev.set_base(base, metric)
        ids, dists, _ = dev.flat_search(q, 10)
        ref = (l2_i, l2_d) if metric == L2 else (ip_i, ip_d)
        assert_exact(ids, dists, *ref, what=f"metric {metric}")


# ---- COS and the public ground-truth helper ----------------------------------------------------
def _cos_input(orc):
    def make():
        rng = np.random.default_rng(21)
        base = rng.standard_normal((3000, 100), dtype=np.float32) * np.float32(3.0)
        q = rng.standard_normal((40, 100), dtype=np.float32)
        nb = np.stack([orc.normalize(r) for r in base])
        nq = np.stack([orc.normalize(r) for r in q])
        return (base, q, nb, nq) + exact_ip(orc, nb, nq, 10)

    return _cached("cos", make)


def test_flat_cos_is_ip_on_normalised_rows(native, orc, flat_mode):
    base, q, nb, nq, ref_i, ref_d = _cos_input(orc)
    dev = native.DeviceIndex(0)
    dev.set_base(nb, COS)
    ids2, d2, _ = dev.flat_search(nq, 10)
    dev.set_base(nb, IP)
    ids1, d1, _ = dev.flat_search(nq, 10)
    assert_exact(ids2, d2, ref_i, ref_d, what="cos")
    assert_exact(ids1, d1, ref_i, ref_d, what="ip")


def test_normalize_rows_is_the_reference_normalisation(native, orc):
    base, q, nb, nq, _, _ = _cos_input(orc)
    got = native.normalize_rows(base)
    assert got.dtype == np.float32 and got is not base
    assert np.array_equal(got.view(np.uint32), nb.view(np.uint32))


def test_calc_gt_device_metrics(native, orc):
    import alayalite_amd
    from alayalite_amd.utils import calc_gt

    base, q, nb, nq, ref_i, ref_d = _cos_input(orc)
    keep = base.copy()
    ids, dists = alayalite_amd.utils.calc_gt_device(base, q, 10, metric="cos")
    assert np.array_equal(base, keep)  # normalises copies
    assert ids.dtype == np.int32 and np.array_equal(ids, ref_i.astype(np.int32))
    assert np.array_equal(dists.view(np.uint32), ref_d.view(np.uint32))
    ip_i, ip_d = exact_ip(orc, base, q, 10)
    ids, dists = alayalite_amd.utils.calc_gt_device(base, q, 10, metric="ip")
    assert np.array_equal(ids, ip_i.astype(np.int32))
    assert np.array_equal(dists.view(np.uint32), ip_d.view(np.uint32))
    # the L2 default is unchanged (test_flat.py::test_calc_gt_device_matches_calc_gt's expectations)
    rng = np.random.default_rng(7)
    b2 = rng.random((3000, 100), dtype=np.float32)
    q2 = rng.random((20, 100), dtype=np.float32)
    ids, dists = alayalite_amd.utils.calc_gt_device(b2, q2, 10)
    assert ids.dtype == np.int32 and dists.dtype == np.float32
    assert np.array_equal(ids, calc_gt(b2, q2, 10))
    ids_l2, d_l2 = alayalite_amd.utils.calc_gt_device(b2, q2, 10, metric="l2")
    assert np.array_equal(ids, ids_l2) and np.array_equal(dists.view(np.uint32), d_l2.view(np.uint32))


# ---- Index.exact_search ------------------------------------------------------------------------
_N, _D, _NQ = 2000, 64, 24


def _index_data():
    rng = np.random.default_rng(64)
    return (np.ascontiguousarray(rng.standard_normal((_N, _D), dtype=np.float32)),
            np.ascontiguousarray(rng.standard_normal((_NQ, _D), dtype=np.float32)))


def _reference(orc, metric, rows, q, k, valid=None):
    """The reference over `rows` as the index stores them (COS: normalised rows and queries)."""
    if metric == "cos":
        rows = np.stack([orc.normalize(r) for r in rows])
        q = np.stack([orc.normalize(r) for r in q])
    if metric == "l2":
        live = np.arange(len(rows)) if valid is None else np.nonzero(valid)[0]
        ri, rd = exact_l2(orc, rows[live], q, k)
        return live[ri].astype(np.uint32), rd
    return exact_ip(orc, rows, q, k, valid=valid)


@pytest.mark.parametrize("metric", ["l2", "ip", "cos"])
def test_index_exact_search(orc, metric, tmp_path):
    """After fit it equals the reference and measures batch_search's recall; after remove the removed
    id is gone and the result is the reference over the remaining rows; an inserted row can be
    returned; save and load keep the result."""
    import alayalite_amd
    from alayalite_amd.utils import calc_recall

    base, q = _index_data()
    client = alayalite_amd.Client(str(tmp_path))
    index = client.create_index(f"ex_{metric}", metric=metric, capacity=_N + 10)
    with pytest.raises(ValueError, match="not init"):  # as batch_search
        index.exact_search(q.copy(), 10)
    index.fit(base.copy(), ef_construction=100, num_threads=1)
    ids, dists = index.exact_search(q.copy(), 10)
    assert ids.dtype == np.uint32 and ids.shape == (_NQ, 10) and dists.dtype == np.float32
    ref_i, ref_d = _reference(orc, metric, base, q, 10)
    assert_exact(ids, dists, ref_i, ref_d, what="after fit")
    recall = calc_recall(index.batch_search(q.copy(), 10, 200), ids)
    print(f"exact_search: metric={metric} recall@10 of batch_search(ef=200) = {recall:.4f}")
    assert 0.9 < recall <= 1.0
    with pytest.raises(ValueError):
        index.exact_search(q[:, :32].copy(), 10)
    # remove a top-1
    gone = int(ids[0, 0])
    index.remove(gone)
    valid = np.ones(_N, np.uint8)
    valid[gone] = 0
    ids, dists = index.exact_search(q.copy(), 10)
    assert not (ids == gone).any()
    assert_exact(ids, dists, *_reference(orc, metric, base, q, 10, valid=valid), what="after remove")
    # insert a copy of query 3 (scaled up: the best inner product too): it is query 3's top-1
    row = (q[3] * np.float32(4.0 if metric == "ip" else 1.0)).copy()
    new_id = index.insert(row.copy())
    # COS: insert normalises the vector for its search and again when it stores it; the reference
    # below normalises every row once more
    rows2 = np.vstack([base, (orc.normalize(row) if metric == "cos" else row)[None]])
    valid2 = np.append(valid, 1).astype(np.uint8)
    ids, dists = index.exact_search(q.copy(), 10)
    assert ids[3, 0] == new_id
    assert_exact(ids, dists, *_reference(orc, metric, rows2, q, 10, valid=valid2), what="after insert")
    # save / load
    client.save_index(f"ex_{metric}")
    again = alayalite_amd.Client(str(tmp_path)).get_index(f"ex_{metric}")
    ids2, dists2 = again.exact_search(q.copy(), 10)
    assert np.array_equal(ids, ids2) and np.array_equal(dists.view(np.uint32), dists2.view(np.uint32))


@pytest.mark.parametrize("metric", ["l2", "ip", "cos"])
def test_index_exact_search_sq8_and_uint64(orc, metric):
    """On an SQ8 index the exact search runs on the f32 rerank rows; a uint64 id type returns uint64
    ids (empty slots would hold its maximum)."""
    import alayalite_amd

    base, q = _index_data()
    ref_i, ref_d = _cached(("index-ref", metric), lambda: _reference(orc, metric, base, q, 10))
    client = alayalite_amd.Client()
    sq = client.create_index(f"exsq_{metric}", metric=metric, capacity=_N, quantization_type="sq8")
    sq.fit(base.copy(), ef_construction=100, num_threads=1)
    ids, dists = sq.exact_search(q.copy(), 10)
    assert_exact(ids, dists, ref_i, ref_d, what="sq8")
    u64 = client.create_index(f"exu64_{metric}", metric=metric, capacity=_N, id_type=np.uint64)
    u64.fit(base.copy(), ef_construction=100, num_threads=1)
    ids, dists = u64.exact_search(q.copy(), 10)
    assert ids.dtype == np.uint64
    assert_exact(ids.astype(np.uint32), dists, ref_i, ref_d, what="uint64")


def test_index_exact_search_tiny_index_pads_with_id_maximum():
    import alayalite_amd

    rng = np.random.default_rng(5)
    base = rng.random((6, 32), dtype=np.float32)
    for id_type, top in ((np.uint32, 0xFFFFFFFF), (np.uint64, 0xFFFFFFFFFFFFFFFF)):
        index = alayalite_amd.Client().create_index("tiny", metric="ip", capacity=8, id_type=id_type)
        index.fit(base.copy(), ef_construction=20, num_threads=1)
        ids, dists = index.exact_search(base[:2].copy(), 10)
        assert (ids[:, 6:] == top).all() and (dists[:, 6:] == np.finfo(np.float32).max).all()
        assert sorted(ids[0, :6].tolist()) == list(range(6))


def test_index_exact_search_rejects_non_float32():
    import alayalite_amd

    rng = np.random.default_rng(6)
    base = rng.integers(-100, 100, (500, 32)).astype(np.int8)
    index = alayalite_amd.Client().create_index("i8", capacity=500, data_type=np.int8)
    index.fit(base, ef_construction=50, num_threads=1)
    with pytest.raises(ValueError, match="float32"):
        index.exact_search(base[:4].copy(), 5)
