"""Exact range search on the MFMA scan (ALAYA_FLAT_RANGE_MFMA=1: flat_range_mfma_kernels.hip, the thresholds of
flat_range_bound.h): counts, ids and distance bits against flat_range_common's reference over the oracle's
distances, as test_flat_range.py holds the f32 scan to."""

import numpy as np
import pytest

import flat_filtered_common as fc
import flat_range_common as rc
from alayalite_amd.utils import pack_allow

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _mfma(monkeypatch):
    monkeypatch.delenv(rc.CHUNK_ENV, raising=False)
    monkeypatch.delenv(rc.STAGING_ENV, raising=False)
    monkeypatch.delenv("ALAYA_FLAT_RANGE_STAGES", raising=False)
    monkeypatch.setenv("ALAYA_FLAT_RANGE_MFMA", "1")


def _dev(native, base, metric=0, valid=None):
    dev = native.DeviceIndex(0)
    dev.set_base(np.ascontiguousarray(base, np.float32), metric, None if valid is None else fc.valid_bytes(valid))
    return dev


def _search(dev, q, radii, cap, allow=None, groups=None):
    words = None if allow is None else pack_allow(np.asarray(allow), np.asarray(allow).shape[-1])
    radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float32), (len(q),)))
    got = dev.flat_range_search(np.ascontiguousarray(q), radii, cap, words,
                                None if groups is None else np.asarray(groups, np.uint32))
    path = dev.flat_range_path()
    assert path[0] == 1 and path[2] <= path[1], path
    return got, path


def _kth(dist, k):
    return np.sort(dist, axis=1)[:, k - 1].copy()


@pytest.mark.parametrize("d", [1, 33, 100, 128, 200, 960, 1000])
@pytest.mark.parametrize("metric", [0, 1])
def test_widths_and_the_boundary(native, orc, metric, d):
    """Every slab count and tail; n and nq are no multiples of 32.  The radius is each query's reference 20th
    distance: that row is in the band, verified and returned; one ulp below, the rows that tie with it leave."""
    rng = np.random.default_rng(200 + d)
    n, nq = 1999, 37
    base = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    allow = fc.random_mask(n, 0.5, d)
    rows = np.nonzero(allow)[0]
    dist = fc.distances(orc, metric, base, q, rows)
    radii = _kth(dist, 20)
    dev = _dev(native, base, metric)
    got, path = _search(dev, q, radii, 64, allow)
    ref = rc.from_distances(rows, dist, radii, 64)
    assert (ref[0] >= 20).all() and (ref[2][np.arange(nq), ref[0] - 1] == radii).all()
    rc.assert_same(got, ref, what=(metric, d))
    assert path[2] >= nq, path
    assert dev.flat_range_last()[0] == len(rows) and dev.flat_range_last()[2] == 128
    below = np.nextafter(radii, np.float32(-np.inf))
    rc.assert_same(_search(dev, q, below, 64, allow)[0], rc.from_distances(rows, dist, below, 64), what=(metric, d, "below"))


def _scaled_input(scale):
    rng = np.random.default_rng(5)
    base = (rng.standard_normal((600, 40)) * scale).astype(np.float32)
    q = (rng.standard_normal((9, 40)) * scale).astype(np.float32)
    return base, q, fc.random_mask(600, 0.7, 3)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", fc.TIE_KINDS + [1e3, 1e-3])
def test_ties_and_scales(native, orc, kind, metric):
    """Rows that tie at the radius, and signed rows at two scales: the radius is a row's own distance, then one
    ulp below it.  A threshold that is too tight drops or admits a row here."""
    base, q, allow = fc.tie_input(kind) if isinstance(kind, str) else _scaled_input(kind)
    rows = np.nonzero(allow)[0]
    dist = fc.cached(("range-mfma-tie", kind, metric), lambda: fc.distances(orc, metric, base, q, rows))
    radii = _kth(dist, fc.TIE_K)
    dev = _dev(native, base, metric)
    for r in (radii, np.nextafter(radii, np.float32(-np.inf))):
        rc.assert_same(_search(dev, q, r, 2048, allow)[0], rc.from_distances(rows, dist, r, 2048), what=(kind, metric))


@pytest.mark.parametrize("cap", [1, 7, 4096])
@pytest.mark.parametrize("nq", [1, 17])
def test_proven_hits_are_not_measured(native, orc, nq, cap):
    """Radius +inf and FLT_MAX over 5000 rows: every count is 5000, the list is the cap smallest ids by
    (distance, id), and only the stored hits of each (chunk, query) pair -- at most slots + 31 -- had a distance
    computed.  Then with removed rows among the first ids and a 0.9 mask."""
    import torch

    rng = np.random.default_rng(16)
    base = rng.standard_normal((5000, 16), dtype=np.float32)
    q = rng.standard_normal((17, 16), dtype=np.float32)[:nq]
    dist = fc.cached(("range-mfma-trunc", nq), lambda: fc.distances(orc, 0, base, q, np.arange(5000)))
    valid = np.ones(5000, bool)
    valid[[0, 1, 5, 31, 32, 33, 100]] = False
    allow = fc.random_mask(5000, 0.9, 9)
    plan = native.flat_range_mfma_plan(5000, nq, cap, torch.cuda.get_device_properties(0).multi_processor_count)
    for radius in (np.inf, fc.FLT_MAX):
        radii = np.full(nq, radius, np.float32)
        for dev, a, rows in ((_dev(native, base), None, np.arange(5000)),
                             (_dev(native, base, 0, valid), allow, np.nonzero(valid & allow)[0])):
            got, path = _search(dev, q, radii, cap, a)
            assert (got[0] == len(rows)).all()
            rc.assert_same(got, rc.from_distances(rows, dist[:, rows], radii, cap), what=(nq, cap, radius, a is None))
            chunks = dev.flat_range_last()[1]
            assert chunks == plan[1] and path[1] <= nq * chunks * (plan[4] + 31) and path[3] > 0, (path, plan)


@pytest.mark.parametrize("metric", [0, 1])
def test_no_bound(native, orc, metric):
    """A query with an inf element, and a base whose largest row norm is past 1e18: no threshold exists, every
    eligible pair is verified, and the answer is still the reference's."""
    rng = np.random.default_rng(77)
    base = rng.standard_normal((700, 16), dtype=np.float32)
    q = rng.standard_normal((5, 16), dtype=np.float32)
    radii = _kth(fc.distances(orc, metric, base, q, np.arange(700)), 30)
    q_inf = q.copy()
    q_inf[2, 3] = np.inf
    big = base.copy()
    big[123] *= np.float32(1e18)
    with np.errstate(all="ignore"):
        for b, qq, verified in ((base, q_inf, 700), (big, q, 5 * 700)):
            got, path = _search(_dev(native, b, metric), qq, radii, 64)
            rc.assert_same(got, rc.reference(orc, metric, b, qq, radii, 64), what=(metric, verified))
            assert path[1] >= verified and (verified == 700 or path[3] == 0), path


@pytest.mark.parametrize("metric", [0, 1])
def test_masks(native, orc, monkeypatch, metric):
    """Three interleaved masks, radii mixing -inf, tight, wide and FLT_MAX: the MFMA scan's answer is the f32
    scan's, and the reference's."""
    base, q = fc.gist_rows(2000, 12, 128)
    n = len(base)
    allow = np.stack([fc.random_mask(n, s, 40 + i) for i, s in enumerate((0.5, 0.05, 0.9))])
    groups = np.arange(len(q)) % 3
    dist = fc.cached(("range-groups-dist", metric), lambda: fc.distances(orc, metric, base, q, np.arange(n)))
    pick = np.arange(len(q)) % 4
    radii = np.choose(pick, [np.full(len(q), -np.inf), _kth(dist, 5), _kth(dist, 900), np.full(len(q), fc.FLT_MAX)])
    radii = radii.astype(np.float32)
    dev = _dev(native, base, metric)
    got, _ = _search(dev, q, radii, 1024, allow, groups)
    assert dev.flat_range_last()[4] == allow.sum()
    rc.assert_same(got, rc.reference(orc, metric, base, q, radii, 1024, allow, None, groups), what=metric)
    monkeypatch.setenv("ALAYA_FLAT_RANGE_MFMA", "0")
    f32 = dev.flat_range_search(np.ascontiguousarray(q), radii, 1024, pack_allow(allow, n), groups.astype(np.uint32))
    assert dev.flat_range_path() == (0, 0, 0, 0)
    rc.assert_same(got, f32, what=(metric, "f32 scan"))
