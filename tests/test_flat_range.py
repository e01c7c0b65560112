"""Exact range search on the device (alaya_index_flat_range_search*): compaction of (mask AND validity), the
row-reusing f32 scan with a threshold, the gather in chunk order, the sort.  Every comparison is array_equal
on counts, on ids and on distance bits, empty slots included, against flat_range_common.reference."""

import numpy as np
import pytest

import flat_filtered_common as fc
import flat_range_common as rc
from alayalite_amd.utils import pack_allow

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_plan(monkeypatch):
    monkeypatch.delenv(rc.CHUNK_ENV, raising=False)
    monkeypatch.delenv(rc.STAGING_ENV, raising=False)
    monkeypatch.delenv("ALAYA_FLAT_RANGE_STAGES", raising=False)


def _dev(native, base, metric=0, valid=None):
    dev = native.DeviceIndex(0)
    dev.set_base(np.ascontiguousarray(base, np.float32), metric, None if valid is None else fc.valid_bytes(valid))
    return dev


def _search(dev, q, radii, cap, allow=None, groups=None):
    words = None
    if allow is not None:
        allow = np.asarray(allow)
        words = pack_allow(allow, allow.shape[-1])
    radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float32), (len(q),)))
    return dev.flat_range_search(np.ascontiguousarray(q), radii, cap, words,
                                 None if groups is None else np.asarray(groups, np.uint32))


def _kth(dist, k):
    """Each query's k-th smallest distance (k from 1)."""
    return np.sort(dist, axis=1)[:, k - 1].copy()


@pytest.mark.parametrize("d", [1, 7, 8, 31, 32, 33, 40, 100, 128, 200, 256, 960, 1000])
@pytest.mark.parametrize("metric", [0, 1])
def test_every_tail_of_the_sum(native, orc, metric, d):
    """Whole 32-element blocks, the 8-element blocks on lanes 0-1 and the scalar tail, in every mix.  The radius
    of each query is its reference 20th distance: that row sits exactly on the boundary and is returned."""
    rng = np.random.default_rng(100 + d)
    base = rng.standard_normal((600, d), dtype=np.float32)
    q = rng.standard_normal((5, d), dtype=np.float32)
    allow = fc.random_mask(600, 0.5, d)
    rows = np.nonzero(allow)[0]
    dist = fc.distances(orc, metric, base, q, rows)
    radii = _kth(dist, 20)
    ref = rc.from_distances(rows, dist, radii, 64)
    assert (ref[0] >= 20).all() and (ref[2][np.arange(5), ref[0] - 1] == radii).all()  # the boundary row is in
    rc.assert_same(_search(_dev(native, base, metric), q, radii, 64, allow), ref, what=(metric, d))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", fc.TIE_KINDS)
def test_boundary_and_ties(native, orc, monkeypatch, kind, metric):
    """The radius is a row's own distance: the row, and every row that ties with it, is in; one ulp below, they
    are out.  Chunks of one wave pass: equal distances order by id across chunk boundaries."""
    base, q, allow = fc.tie_input(kind)
    rows = np.nonzero(allow)[0]
    dist = fc.cached(("range-tie-dist", kind, metric), lambda: fc.distances(orc, metric, base, q, rows))
    radii = _kth(dist, fc.TIE_K)
    below = np.nextafter(radii, np.float32(-np.inf))
    cap = 2048
    ref_in = rc.from_distances(rows, dist, radii, cap)
    ref_out = rc.from_distances(rows, dist, below, cap)
    at = (dist == radii[:, None]).sum(1)
    assert (at >= 1).all() and np.array_equal(ref_in[0] - ref_out[0], at)
    monkeypatch.setenv(rc.CHUNK_ENV, str(rc.PASS_ROWS))
    dev = _dev(native, base, metric)
    rc.assert_same(_search(dev, q, radii, cap, allow), ref_in, what=(kind, metric, "in"))
    assert dev.flat_range_last()[1] == -(-len(rows) // rc.PASS_ROWS)
    rc.assert_same(_search(dev, q, below, cap, allow), ref_out, what=(kind, metric, "out"))


def _share_mask(share, n):
    if share == "none":
        return np.zeros(n, bool)
    if share == "one":
        a = np.zeros(n, bool)
        a[1234] = True
        return a
    return fc.random_mask(n, share, 31) if share < 1 else np.ones(n, bool)


def _shares_input(orc):
    base, q = fc.gist_rows(2000, 12, 128)
    dist = fc.cached(("range-shares-dist",), lambda: fc.distances(orc, 0, base, q, np.arange(len(base))))
    return base, q, dist


@pytest.mark.parametrize("share", ["none", "one", 0.01, 0.5, 1, "no mask"])
def test_shares(native, orc, share):
    """From nothing allowed over one row to everything allowed; no mask at all equals the all-ones mask."""
    base, q, dist = _shares_input(orc)
    n = len(base)
    allow = None if share == "no mask" else _share_mask(share, n)
    rows = np.arange(n) if allow is None else np.nonzero(allow)[0]
    radii = _kth(dist, 300)  # 300 of all rows: some, not all, of every mask's
    radii[0] = np.inf
    ref = rc.from_distances(rows, dist[:, rows], radii, 512)
    dev = fc.cached(("range-shares-dev",), lambda: _dev(native, base))
    got = _search(dev, q, radii, 512, allow)
    rc.assert_same(got, ref, what=share)
    assert got[0][0] == len(rows)
    assert dev.flat_range_last()[0] == len(rows)
    if share == "no mask":
        rc.assert_same(got, _search(dev, q, radii, 512, np.ones(n, bool)), what="all-ones mask")
        # bits past n are ignored
        n2 = 1999
        dev2 = _dev(native, base[:n2])
        words = fc.padding_words(n2, np.ones(n2, bool))
        got2 = dev2.flat_range_search(np.ascontiguousarray(q), radii, 512, words, None)
        rc.assert_same(got2, rc.from_distances(np.arange(n2), dist[:, :n2], radii, 512), what="padding bits")


def test_removed_rows(native, orc):
    """A removed row is never returned or counted, whatever the radius, +inf included, with and without a mask."""
    base, q, dist = _shares_input(orc)
    n = len(base)
    valid = fc.random_mask(n, 0.7, 77)
    valid[:40] = False
    allow = fc.random_mask(n, 0.5, 31)
    dev = _dev(native, base, 0, valid)
    for radii in (_kth(dist, 300), np.full(len(q), np.inf, np.float32), np.full(len(q), fc.FLT_MAX, np.float32)):
        for a in (None, allow):
            rows = np.nonzero(valid if a is None else valid & a)[0]
            ref = rc.from_distances(rows, dist[:, rows], radii, 4096)
            got = _search(dev, q, radii, 4096, a)
            rc.assert_same(got, ref, what=(float(radii[0]), a is None))
            assert not np.isin(got[1], np.nonzero(~valid)[0]).any()
    assert (got[0] == (valid & allow).sum()).all()


def _trunc_input(orc):
    rng = np.random.default_rng(16)
    base = rng.standard_normal((5000, 16), dtype=np.float32)
    q = rng.standard_normal((17, 16), dtype=np.float32)
    dist = fc.cached(("range-trunc-dist",), lambda: fc.distances(orc, 0, base, q, np.arange(5000)))
    return base, q, dist


@pytest.mark.parametrize("forced", [None, 32])
@pytest.mark.parametrize("cap", [1, 7, 4096])
@pytest.mark.parametrize("nq", [1, 5, 17])
def test_truncation(native, orc, monkeypatch, nq, cap, forced):
    """Radius +inf over 5000 rows: counts == 5000 and the list is the C smallest eligible ids by (distance, id).
    C = 1 and 7 cut inside a pass, C = 4096 inside a chunk after many full ones.  Then with a mask and removed
    rows among the first ids."""
    base, q, dist = _trunc_input(orc)
    q, dist = q[:nq], dist[:nq]
    if forced:
        monkeypatch.setenv(rc.CHUNK_ENV, str(forced))
    radii = np.full(nq, np.inf, np.float32)
    dev = fc.cached(("range-trunc-dev",), lambda: _dev(native, base))
    got = _search(dev, q, radii, cap)
    assert (got[0] == 5000).all()
    assert np.array_equal(np.sort(got[1], axis=1), np.tile(np.arange(cap, dtype=np.uint32), (nq, 1)))
    rc.assert_same(got, rc.from_distances(np.arange(5000), dist, radii, cap), what=(nq, cap, forced))
    if forced:
        assert dev.flat_range_last()[:2] == (5000, -(-5000 // 32))
    valid = np.ones(5000, bool)
    valid[[0, 1, 5, 31, 32, 33, 100]] = False
    allow = fc.random_mask(5000, 0.9, 9)
    rows = np.nonzero(valid & allow)[0]
    dev2 = fc.cached(("range-trunc-dev2",), lambda: _dev(native, base, 0, valid))
    got = _search(dev2, q, radii, cap, allow)
    assert (got[0] == len(rows)).all()
    rc.assert_same(got, rc.from_distances(rows, dist[:, rows], radii, cap), what=(nq, cap, forced, "masked"))


def test_more_than_one_scan_launch_per_mask(native, orc, monkeypatch):
    """The staging knob splits a mask's queries over scan launches: the result is that of one launch."""
    base, q, dist = _trunc_input(orc)
    radii = _kth(dist, 700)
    radii[3] = np.inf
    cap = 256
    dev = fc.cached(("range-trunc-dev",), lambda: _dev(native, base))
    one = _search(dev, q, radii, cap)
    assert dev.flat_range_last()[3] == 1
    rc.assert_same(one, rc.from_distances(np.arange(5000), dist, radii, cap), what="one launch")
    monkeypatch.setenv(rc.CHUNK_ENV, "64")
    chunks = -(-5000 // 64)
    monkeypatch.setenv(rc.STAGING_ENV, str(chunks * 16 * (64 * 8 + 4)))  # one query tile per launch
    split = _search(dev, q, radii, cap)
    last = dev.flat_range_last()
    assert last[1] == chunks and last[2] == 16 and last[3] == 2, last
    rc.assert_same(split, one, what="two launches")


def test_groups_and_radii(native, orc):
    """Three interleaved masks; per-query radii mix -inf, a tight one, a wide one and FLT_MAX; IP radii are
    negative."""
    base, q = fc.gist_rows(2000, 12, 128)
    n = len(base)
    allow = np.stack([fc.random_mask(n, s, 40 + i) for i, s in enumerate((0.5, 0.05, 0.9))])
    groups = np.arange(len(q)) % 3
    for metric in (0, 1):
        dist = fc.cached(("range-groups-dist", metric), lambda: fc.distances(orc, metric, base, q, np.arange(n)))
        tight, wide = _kth(dist, 5), _kth(dist, 900)
        radii = np.where(np.arange(len(q)) % 4 == 0, -np.inf,
                         np.where(np.arange(len(q)) % 4 == 1, tight,
                                  np.where(np.arange(len(q)) % 4 == 2, wide, fc.FLT_MAX))).astype(np.float32)
        if metric == 1:
            assert (tight < 0).all()
        ref = rc.reference(orc, metric, base, q, radii, 1024, allow, None, groups)
        assert (ref[0][radii == -np.inf] == 0).all() and (ref[0][radii == fc.FLT_MAX] > 0).all()
        dev = _dev(native, base, metric)
        rc.assert_same(_search(dev, q, radii, 1024, allow, groups), ref, what=metric)
        assert dev.flat_range_last()[4] == allow.sum()


def test_device_entry(native, orc):
    """alaya_index_flat_range_search_device on a torch stream, outputs prefilled with 7: every slot of every
    query is written.  A NaN radius matches nothing there."""
    import torch

    base, q, dist = _shares_input(orc)
    n = len(base)
    allow = np.stack([fc.random_mask(n, 0.5, 31), np.zeros(n, bool)])
    groups = (np.arange(len(q)) % 2).astype(np.uint32)
    radii = _kth(dist, 300)
    radii[2] = np.nan
    cap = 100
    ref = rc.reference(orc, 0, base, q, np.where(np.isnan(radii), -np.inf, radii), cap, allow, None, groups)
    dev = fc.cached(("range-shares-dev",), lambda: _dev(native, base))
    d0 = torch.device("cuda", 0)
    nq = len(q)
    words = pack_allow(allow, n)
    side = torch.cuda.Stream(d0)
    with torch.cuda.stream(side):
        qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(d0)
        rd = torch.from_numpy(radii).to(d0)
        wd = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(d0)
        gd = torch.from_numpy(groups.view(np.int32)).to(d0)
        cnt = torch.full((nq,), 7, dtype=torch.int32, device=d0)
        ids = torch.full((nq, cap), 7, dtype=torch.int32, device=d0)
        dd = torch.full((nq, cap), 7.0, dtype=torch.float32, device=d0)
        dev.flat_range_search_device(qd.data_ptr(), nq, rd.data_ptr(), cap, wd.data_ptr(), 2, gd.data_ptr(), cnt.data_ptr(),
                                     ids.data_ptr(), dd.data_ptr(), side.cuda_stream)
        side.synchronize()
    got = (cnt.cpu().numpy().view(np.uint32), ids.cpu().numpy().view(np.uint32), dd.cpu().numpy())
    rc.assert_same(got, ref, what="device entry")
    assert ref[0][2] == 0 and (ref[0][1::2] == 0).all() and (ref[0][0] > 0)
    # no mask on the device entry: null words with n_masks 0
    with torch.cuda.stream(side):
        cnt.fill_(7)
        ids.fill_(7)
        dd.fill_(7.0)
        dev.flat_range_search_device(qd.data_ptr(), nq, rd.data_ptr(), cap, 0, 0, 0, cnt.data_ptr(), ids.data_ptr(),
                                     dd.data_ptr(), side.cuda_stream)
        side.synchronize()
    got = (cnt.cpu().numpy().view(np.uint32), ids.cpu().numpy().view(np.uint32), dd.cpu().numpy())
    rc.assert_same(got, rc.from_distances(np.arange(n), dist, np.where(np.isnan(radii), -np.inf, radii), cap),
                   what="device entry, no mask")


def test_host_entry_refuses_bad_arguments(native):
    base, q = fc.gist_rows(2000, 12, 128)
    dev = _dev(native, base)
    radii = np.zeros(len(q), np.float32)
    for cap in (0, 4097):
        with pytest.raises(Exception):
            dev.flat_range_search(np.ascontiguousarray(q), radii, cap, None, None)
    bad = radii.copy()
    bad[5] = np.nan
    with pytest.raises(Exception):
        dev.flat_range_search(np.ascontiguousarray(q), bad, 10, None, None)
    with pytest.raises(Exception):  # groups without masks
        dev.flat_range_search(np.ascontiguousarray(q), radii, 10, None, np.zeros(len(q), np.uint32))
