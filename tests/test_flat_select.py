"""Exact k-NN above k = 224: the histogram-select MFMA scan (flat_select_kernels.hip) behind
DeviceIndex.flat_select_search, calc_gt_device and Index.exact_search.  Contract: flat_search's -- the k smallest
valid rows by the reference's f32 distance, ties by id, empty slots (id max, FLT_MAX) -- with ids and distance
bits equal to the oracle's; there is no tolerance."""

import numpy as np
import pytest

import alayalite_amd
from alayalite_amd.utils import calc_gt_device
from flat_common import FLT_MAX, assert_exact
from flat_common import exact as exact_l2
from flat_ip_common import exact_ip

pytestmark = pytest.mark.gpu
KMAX = 2048
# n off the 32-row tile and the 128-row super-tile; a partial slab (24, 100), 2 and 15 slabs; nq across the
# 32-query wave and the 128-query workgroup; the last shape is the smallest whose span and first window come from
# a strided sample (every second super-tile from 131072 rows on)
SHAPES = [(4133, 24, 1), (4133, 100, 33), (9000, 128, 130), (3000, 960, 5), (131333, 16, 2)]
_cache = {}


def _input(orc, n, d, nq, metric="l2"):
    """Rows, queries and the reference at KMAX, computed once per shape and never modified."""
    key = (n, d, nq, metric)
    if key not in _cache:
        rng = np.random.default_rng(n + d + nq)
        base = np.ascontiguousarray(rng.standard_normal((n, d), dtype=np.float32))
        q = np.ascontiguousarray(rng.standard_normal((nq, d), dtype=np.float32))
        if metric == "cos":
            rb, rq = np.stack([orc.normalize(r) for r in base]), np.stack([orc.normalize(r) for r in q])
            ref = exact_ip(orc, rb, rq, KMAX)
        else:
            ref = exact_ip(orc, base, q, KMAX) if metric == "ip" else exact_l2(orc, base, q, KMAX)
        _cache[key] = (base, q) + ref
    return _cache[key]


@pytest.mark.parametrize("k", [225, 1000, 2048])
@pytest.mark.parametrize("n,d,nq", SHAPES)
def test_select_exact(native, orc, n, d, nq, k):
    base, q, ref_i, ref_d = _input(orc, n, d, nq)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0)
    ids, dists, redo = dev.flat_select_search(q, k)
    passes, verified, fallback = dev.flat_select_last()
    print(f"select: shape={(n, d, nq)} k={k} full passes={passes} verified pairs/query={verified / nq:.0f} redo={redo}")
    assert_exact(ids, dists, ref_i[:, :k], ref_d[:, :k])
    assert redo == 0 and fallback == 0 and 1 <= passes <= 4


@pytest.mark.parametrize("metric,n,d,nq", [("ip", 4133, 100, 33), ("cos", 3000, 960, 5)])
def test_select_metrics(native, orc, metric, n, d, nq):
    base, q, ref_i, ref_d = _input(orc, n, d, nq, metric)
    ids, dists = calc_gt_device(base, q, 1000, metric=metric)
    assert_exact(ids.view(np.uint32), dists, ref_i[:, :1000], ref_d[:, :1000])


def test_select_device_entry(native, orc):
    import torch

    base, q, ref_i, ref_d = _input(orc, 4133, 100, 33)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0)
    d0 = torch.device("cuda", 0)
    qd = torch.from_numpy(q).to(d0)
    ids = torch.zeros((len(q), 1000), dtype=torch.int32, device=d0)
    dists = torch.zeros((len(q), 1000), dtype=torch.float32, device=d0)
    redo = dev.flat_select_search_device(qd.data_ptr(), len(q), 1000, ids.data_ptr(), dists.data_ptr(),
                                         torch.cuda.current_stream(d0).cuda_stream)
    torch.cuda.synchronize()
    assert redo == 0
    assert_exact(ids.cpu().numpy().view(np.uint32), dists.cpu().numpy(), ref_i[:, :1000], ref_d[:, :1000])


def test_select_short_base(native, orc):
    """Fewer rows than k: every row in order, then (id max, FLT_MAX)."""
    base, q, _, _ = _input(orc, 4133, 24, 1)
    ref_i, ref_d = exact_l2(orc, base[:300], q, 512)
    ids, dists = calc_gt_device(base[:300], q, 512)
    assert_exact(ids.view(np.uint32), dists, ref_i, ref_d)
    assert (ids[:, 300:] == -1).all() and (dists[:, 300:] == FLT_MAX).all()


def test_select_removed_rows(orc):
    """Index.exact_search after remove of rows among the true neighbours: they are absent, the rest moves up."""
    base, q, ref_i, ref_d = _input(orc, 4133, 100, 33)
    index = alayalite_amd.Client().create_index("select_removed", capacity=len(base), metric="l2", id_type=np.uint32)
    index.fit(base.copy(), ef_construction=40)
    gone = [int(v) for v in ref_i[0, [0, 5, 224, 299]]] + [int(ref_i[7, 100])]
    for v in gone:
        index.remove(v)
    ids, dists = index.exact_search(q.copy(), 300)
    for a in range(len(q)):
        keep = ~np.isin(ref_i[a], gone)
        assert np.array_equal(ids[a], ref_i[a][keep][:300])
        assert np.array_equal(dists[a].view(np.uint32), ref_d[a][keep][:300].view(np.uint32))


def test_select_ties_across_the_cut(native, orc):
    """40 copies of one row straddle rank k: the ids decide which copies are kept."""
    base, q, ref_i, _ = _input(orc, 4133, 24, 1)
    base = base.copy()
    k = 300
    copies = np.random.default_rng(3).choice(len(base), 40, replace=False)
    base[copies] = base[ref_i[0, k - 20]]
    ref_i, ref_d = exact_l2(orc, base, q, k)
    assert np.isin(ref_i[0], copies).sum() < 40  # some copies fall past the cut
    ids, dists = calc_gt_device(base, q, k)
    assert_exact(ids.view(np.uint32), dists, ref_i, ref_d)


def test_select_mass_tie_takes_the_fallback(native):
    """6000 identical rows: every pair ties, more than the 4096 a list holds, so the exhaustive recompute answers
    (the oracle's tie rule is by id: ids 0..299)."""
    rng = np.random.default_rng(1)
    base = np.tile(rng.random(64, dtype=np.float32), (6000, 1))
    q = rng.random((3, 64), dtype=np.float32)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0)
    ids, dists, redo = dev.flat_select_search(q, 300)
    assert redo == 3 and dev.flat_select_last()[2] == 3
    assert (ids == np.arange(300, dtype=np.uint32)).all() and (dists == dists[:, :1]).all()


def test_select_mixed_scales(native, orc):
    """Tiny queries beside ordinary ones and rows of two magnitudes: windows and bin widths are per query."""
    rng = np.random.default_rng(17)
    base = np.ascontiguousarray(rng.random((4000, 64), dtype=np.float32))
    q = np.ascontiguousarray(rng.random((20, 64), dtype=np.float32))
    q[::4] *= np.float32(1e-30)
    base[::5] *= np.float32(1e3)
    ref_i, ref_d = exact_l2(orc, base, q, 225)
    ids, dists = calc_gt_device(base, q, 225)
    assert_exact(ids.view(np.uint32), dists, ref_i, ref_d)


def test_select_equals_flat_search_at_224(native, orc, monkeypatch):
    base, q, _, _ = _input(orc, 4133, 100, 33)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0)
    ids, dists, _ = dev.flat_search(q, 224)
    monkeypatch.setenv("ALAYA_FLAT_SELECT", "1")
    ids_s, dists_s, redo = dev.flat_select_search(q, 224)
    assert dev.flat_select_last()[0] >= 1  # the selection ran
    assert_exact(ids_s, dists_s, ids, dists)


def test_select_refusals(native):
    base = np.zeros((400, 16), np.float32)
    index = alayalite_amd.Client().create_index("select_refusals", capacity=400, metric="l2", id_type=np.uint32)
    index.fit(base + np.arange(400, dtype=np.float32)[:, None], ef_construction=40)
    with pytest.raises(ValueError, match="2048"):
        index.exact_search(base[:2], 2049)
    with pytest.raises(ValueError, match="224"):
        index.exact_search(base[:2], 225, allow=np.ones(400, bool))
