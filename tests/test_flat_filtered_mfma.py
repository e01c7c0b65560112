"""Exact filtered k-NN on the MFMA scan (ALAYA_FLAT_FILTER_MFMA=1: flat_filtered_mfma_kernels.hip, thresholds
from flat_range_bound.h at each list's worst distance): ids and distance bits against flat_filtered_common's
reference over the oracle's distances, as test_flat_filtered.py holds the f32 scan to."""

import numpy as np
import pytest

import flat_filtered_common as fc
from alayalite_amd.utils import pack_allow
from test_flat_filtered import _dev, _device_entry, _host

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _mfma(monkeypatch):
    monkeypatch.delenv("ALAYA_FLAT_FILTER_CHUNK_ROWS", raising=False)
    monkeypatch.setenv("ALAYA_FLAT_FILTER_MFMA", "1")


def _search(dev, q, k, allow, groups=None):
    allow = np.asarray(allow)
    got = dev.flat_search_filtered(np.ascontiguousarray(q), k, pack_allow(allow, allow.shape[-1]),
                                   None if groups is None else np.asarray(groups, np.uint32))
    path = dev.flat_filtered_path()
    assert path[0] == 1 and path[2] <= path[1] <= path[3], path
    return got, path


def _top(rows, dist, k):
    """The first k of `rows` by (distance, id) per query, the rest empty."""
    out_i = np.full((len(dist), k), fc.EMPTY, np.uint32)
    out_d = np.full((len(dist), k), fc.FLT_MAX, np.float32)
    for a in range(len(dist)):
        o = np.lexsort((rows, dist[a]))[:k]
        out_i[a, :len(o)], out_d[a, :len(o)] = rows[o], dist[a][o]
    return out_i, out_d


@pytest.mark.parametrize("d", [1, 33, 100, 128, 200, 960, 1000])
@pytest.mark.parametrize("metric", [0, 1])
def test_widths(native, orc, metric, d):
    """Every slab count and tail; n and nq are no multiples of 32."""
    rng = np.random.default_rng(200 + d)
    n, nq = 1999, 37
    base = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    allow = fc.random_mask(n, 0.5, d)
    dev = _dev(native, base, metric)
    (ids, dists), _ = _search(dev, q, 20, allow)
    fc.assert_same(ids, dists, *fc.reference(orc, metric, base, q, 20, allow), what=(metric, d))
    assert dev.flat_filtered_last()[0] == allow.sum() and dev.flat_filtered_last()[2] == 128


def _scaled_input(scale):
    rng = np.random.default_rng(5)
    base = (rng.standard_normal((600, 40)) * scale).astype(np.float32)
    q = (rng.standard_normal((9, 40)) * scale).astype(np.float32)
    return base, q, fc.random_mask(600, 0.7, 3)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", fc.TIE_KINDS + [1e3, 1e-3])
def test_ties_and_scales(native, orc, kind, metric):
    """Rows that tie at the k-th distance, and signed rows at two scales: a threshold one step too tight drops a
    row that belongs in the list, and the answer shows another id."""
    base, q, allow = fc.tie_input(kind) if isinstance(kind, str) else _scaled_input(kind)
    ref = fc.cached(("filtered-mfma-tie", kind, metric), lambda: fc.reference(orc, metric, base, q, fc.TIE_K, allow))
    (ids, dists), _ = _search(_dev(native, base, metric), q, fc.TIE_K, allow)
    fc.assert_same(ids, dists, *ref, what=(kind, metric))


@pytest.mark.parametrize("k", [1, 64, 65, 224])
@pytest.mark.parametrize("nq", [1, 17])
def test_list_sizes(native, orc, nq, k):
    """Lists of one entry, of one and of more than one entry per lane, and the longest, over 5000 x 16 rows with
    removed rows among the first ids: a 0.9 mask, then a 0.01 mask whose ~50 eligible rows leave empty slots
    from k = 64.  At k = 1 most pairs are proven out: a chunk is at least 1024 rows, and a list verifies a
    32-row tile while it has no threshold and about k (1 + ln(rows / k)) rows in all when rows come in random
    order -- far under half of the ~920 eligible rows of a chunk."""
    rng = np.random.default_rng(16)
    base = rng.standard_normal((5000, 16), dtype=np.float32)
    q = rng.standard_normal((17, 16), dtype=np.float32)[:nq]
    dist = fc.cached(("filtered-mfma-lists", nq), lambda: fc.distances(orc, 0, base, q, np.arange(5000)))
    valid = np.ones(5000, bool)
    valid[[0, 1, 5, 31, 32, 33, 100]] = False
    dev = _dev(native, base, 0, valid)
    for share in (0.9, 0.01):
        allow = fc.random_mask(5000, share, 9)
        rows = np.nonzero(valid & allow)[0]
        (ids, dists), path = _search(dev, q, k, allow)
        fc.assert_same(ids, dists, *_top(rows, dist[:, rows], k), what=(nq, k, share))
        assert path[3] == len(rows) * nq and dev.flat_filtered_last()[0] == len(rows)
        if share == 0.01 and k >= 64:
            assert len(rows) < k and (ids[:, len(rows):] == fc.EMPTY).all() and (dists[:, len(rows):] == fc.FLT_MAX).all()
        if share == 0.9 and k == 1:
            assert path[2] <= path[1] <= path[3] // 2, path


@pytest.mark.parametrize("metric", [0, 1])
def test_no_bound(native, orc, monkeypatch, metric):
    """A query with an inf element, and a base whose largest row norm is past 1e18: no threshold exists, every
    eligible pair is verified, and the answer is still the reference's and the f32 scan's.  Under L2 every distance
    of the inf query is +inf; the entry's contract does not cover such rows (both scans leave the slots empty, the
    reference lists them), so that query is held to the f32 scan alone."""
    rng = np.random.default_rng(77)
    base = rng.standard_normal((700, 16), dtype=np.float32)
    q = rng.standard_normal((5, 16), dtype=np.float32)
    allow = fc.random_mask(700, 0.9, 4)
    m = int(allow.sum())
    q_inf = q.copy()
    q_inf[2, 3] = np.inf
    big = base.copy()
    big[123] *= np.float32(1e18)
    with np.errstate(all="ignore"):
        for b, qq, verified in ((base, q_inf, m), (big, q, 5 * m)):
            dev = _dev(native, b, metric)
            monkeypatch.setenv("ALAYA_FLAT_FILTER_MFMA", "1")
            (ids, dists), path = _search(dev, qq, 30, allow)
            assert path[1] >= verified and path[3] == 5 * m, path
            ref_i, ref_d = fc.reference(orc, metric, b, qq, 30, allow)
            covered = ~np.isposinf(ref_d).any(1)
            assert covered.sum() >= 4
            fc.assert_same(ids[covered], dists[covered], ref_i[covered], ref_d[covered], what=(metric, verified))
            monkeypatch.setenv("ALAYA_FLAT_FILTER_MFMA", "0")
            fc.assert_same(ids, dists, *_search_f32(dev, qq, 30, allow), what=(metric, verified, "f32 scan"))


def _search_f32(dev, q, k, allow, groups=None):
    allow = np.asarray(allow)
    got = dev.flat_search_filtered(np.ascontiguousarray(q), k, pack_allow(allow, allow.shape[-1]),
                                   None if groups is None else np.asarray(groups, np.uint32))
    assert dev.flat_filtered_path() == (0, 0, 0, 0)
    return got


@pytest.mark.parametrize("metric", [0, 1])
def test_masks(native, orc, monkeypatch, metric):
    """Three interleaved masks with per-query indices: the MFMA scan's answer is the reference's and the f32
    scan's, through the host entry and through the device entry on a torch stream with prefilled outputs."""
    import torch

    base, q = fc.gist_rows(2000, 12, 128)
    n = len(base)
    allow = np.stack([fc.random_mask(n, s, 40 + i) for i, s in enumerate((0.5, 0.05, 0.9))])
    groups = np.arange(len(q)) % 3
    ref = fc.cached(("filtered-mfma-masks", metric), lambda: fc.reference(orc, metric, base, q, 10, allow, None, groups))
    dev = _dev(native, base, metric)
    (ids, dists), path = _search(dev, q, 10, allow, groups)
    assert dev.flat_filtered_last()[0] == allow.sum() and path[3] == 4 * allow.sum()
    fc.assert_same(ids, dists, *ref, what=metric)
    with torch.cuda.stream(torch.cuda.Stream()):
        di, dd, _keep = _device_entry(dev, q, 10, pack_allow(allow, n), groups)
        assert dev.flat_filtered_path()[0] == 1
        fc.assert_same(_host(di), _host(dd), *ref, what=(metric, "device entry"))
    monkeypatch.setenv("ALAYA_FLAT_FILTER_MFMA", "0")
    fc.assert_same(ids, dists, *_search_f32(dev, q, 10, allow, groups), what=(metric, "f32 scan"))
