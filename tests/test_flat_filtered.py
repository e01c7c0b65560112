"""Exact filtered k-NN on the device (alaya_index_flat_search_filtered*): compaction of
(mask AND validity), the row-reusing f32 scan, the merge.  Every comparison is array_equal on ids and on
distance bits against flat_filtered_common.reference."""

import numpy as np
import pytest

import flat_filtered_common as fc
from alayalite_amd.utils import pack_allow

pytestmark = pytest.mark.gpu

CHUNK_ENV = "ALAYA_FLAT_FILTER_CHUNK_ROWS"


@pytest.fixture(autouse=True)
def _default_chunks(monkeypatch):
    monkeypatch.delenv(CHUNK_ENV, raising=False)


def _dev(native, base, metric=0, valid=None):
    dev = native.DeviceIndex(0)
    dev.set_base(np.ascontiguousarray(base, np.float32), metric, None if valid is None else fc.valid_bytes(valid))
    return dev


def _search(dev, q, k, allow, groups=None):
    allow = np.asarray(allow)
    words = pack_allow(allow, allow.shape[-1])
    return dev.flat_search_filtered(np.ascontiguousarray(q), k, words,
                                    None if groups is None else np.asarray(groups, np.uint32))


def _device_entry(dev, q, k, words, groups=None):
    """alaya_index_flat_search_filtered_device on the current torch stream; outputs prefilled with 7."""
    import torch

    d0 = torch.device("cuda", 0)
    nq = len(q)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(d0)
    wd = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).to(d0)
    gd = None if groups is None else torch.from_numpy(np.asarray(groups, np.uint32).view(np.int32)).to(d0)
    ids = torch.full((nq, k), 7, dtype=torch.int32, device=d0)
    dd = torch.full((nq, k), 7.0, dtype=torch.float32, device=d0)
    s = torch.cuda.current_stream(d0)
    dev.flat_search_filtered_device(qd.data_ptr(), nq, k, wd.data_ptr(), words.shape[0], 0 if gd is None else gd.data_ptr(),
                                    ids.data_ptr(), dd.data_ptr(), s.cuda_stream)
    return ids, dd, (qd, wd, gd)


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


@pytest.mark.parametrize("d", [1, 7, 8, 31, 32, 33, 40, 100, 128, 200, 256, 960, 1000])
@pytest.mark.parametrize("metric", [0, 1])
def test_every_tail_of_the_sum(native, orc, metric, d):
    """Whole 32-element blocks, the 8-element blocks on lanes 0-1 and the scalar tail, in every mix."""
    rng = np.random.default_rng(100 + d)
    base = rng.standard_normal((600, d), dtype=np.float32)
    q = rng.standard_normal((5, d), dtype=np.float32)
    allow = fc.random_mask(600, 0.5, d)
    ref = fc.reference(orc, metric, base, q, 10, allow)
    ids, dists = _search(_dev(native, base, metric), q, 10, allow)
    fc.assert_same(ids, dists, *ref, what=(metric, d))


def _share_mask(share, n):
    if share == "none":
        return np.zeros(n, bool)
    if share == "one":
        a = np.zeros(n, bool)
        a[1234] = True
        return a
    if share == "short":
        return fc.short_input()[2]
    return fc.random_mask(n, share, 31) if share < 1 else np.ones(n, bool)


@pytest.mark.parametrize("share", ["none", "one", "short", 0.01, 0.5, 1])
def test_shares(native, orc, share):
    """From nothing allowed (k empty slots) over short lists to everything allowed, where the result is
    also flat_search's."""
    base, q = fc.gist_rows(2000, 12, 128)
    allow = _share_mask(share, len(base))
    dev = fc.cached(("shares-dev",), lambda: _dev(native, base))
    ref_i, ref_d = fc.cached(("shares-ref", share), lambda: fc.reference(orc, 0, base, q, 10, allow))
    ids, dists = _search(dev, q, 10, allow)
    fc.assert_same(ids, dists, ref_i, ref_d, what=share)
    filled = min(10, int(allow.sum()))
    assert (ids[:, filled:] == fc.EMPTY).all() and (dists[:, filled:] == fc.FLT_MAX).all()
    assert (ids[:, :filled] != fc.EMPTY).all()
    assert dev.flat_filtered_last()[0] == allow.sum()
    if share == 1:
        fi, fd, _ = dev.flat_search(np.ascontiguousarray(q), 10)
        fc.assert_same(ids, dists, fi, fd, what="flat_search")


@pytest.mark.parametrize("k", [1, 10, 50, 224])
def test_k(native, orc, k):
    rng = np.random.default_rng(64)
    base = rng.standard_normal((3000, 64), dtype=np.float32)
    q = rng.standard_normal((8, 64), dtype=np.float32)
    allow = fc.random_mask(3000, 0.3, 5)
    dist = fc.cached(("k-dist",), lambda: fc.distances(orc, 0, base, q, np.nonzero(allow)[0]))
    rows = np.nonzero(allow)[0]
    ref_i = np.stack([rows[np.lexsort((rows, dist[a]))[:k]] for a in range(len(q))]).astype(np.uint32)
    ref_d = np.stack([dist[a][np.lexsort((rows, dist[a]))[:k]] for a in range(len(q))])
    ids, dists = _search(fc.cached(("k-dev",), lambda: _dev(native, base)), q, k, allow)
    fc.assert_same(ids, dists, ref_i, ref_d, what=k)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", fc.TIE_KINDS)
def test_ties(native, orc, monkeypatch, kind, metric):
    """Equal distances across chunk boundaries (chunks of one wave pass) and across the mask: ties go
    to the smaller id, in the scan's lists and in the merge."""
    base, q, allow = fc.tie_input(kind)
    ref = fc.reference(orc, metric, base, q, fc.TIE_K, allow)
    monkeypatch.setenv(CHUNK_ENV, str(fc.PASS_ROWS))
    dev = _dev(native, base, metric)
    ids, dists = _search(dev, q, fc.TIE_K, allow)
    fc.assert_same(ids, dists, *ref, what=(kind, metric))
    assert dev.flat_filtered_last()[1] == -(-int(allow.sum()) // fc.PASS_ROWS)


def test_chunking_changes_nothing(native, orc, monkeypatch):
    base, q = fc.gist_rows(2000, 12, 128)
    allow = fc.random_mask(len(base), 0.5, 31)
    ref_i, ref_d = fc.cached(("shares-ref", 0.5), lambda: fc.reference(orc, 0, base, q, 10, allow))
    dev = fc.cached(("shares-dev",), lambda: _dev(native, base))
    m = int(allow.sum())
    seen = set()
    for forced in (None, 32, 96, 1024):
        if forced is None:
            monkeypatch.delenv(CHUNK_ENV, raising=False)
        else:
            monkeypatch.setenv(CHUNK_ENV, str(forced))
        ids, dists = _search(dev, q, 10, allow)
        fc.assert_same(ids, dists, ref_i, ref_d, what=forced)
        last = dev.flat_filtered_last()
        if forced is not None:
            assert last[1] == -(-m // forced)
        seen.add(last[1])
    assert len(seen) >= 3


@pytest.mark.parametrize("nq", [1, 3, 15, 16, 17, 130])
def test_query_counts(native, orc, nq):
    """Around the query tile of 16 (4 per wave), and several tiles with a ragged last one."""
    rng = np.random.default_rng(9)
    base = rng.standard_normal((1000, 64), dtype=np.float32)
    q_all = rng.standard_normal((130, 64), dtype=np.float32)
    allow = fc.random_mask(1000, 0.3, 9)
    ref_i, ref_d = fc.cached(("nq-ref",), lambda: fc.reference(orc, 0, base, q_all, 10, allow))
    dev = fc.cached(("nq-dev",), lambda: _dev(native, base))
    ids, dists = _search(dev, q_all[:nq], 10, allow)
    fc.assert_same(ids, dists, ref_i[:nq], ref_d[:nq], what=nq)
    assert dev.flat_filtered_last()[2] == (4 if nq <= 4 else 16)


def test_groups(native, orc):
    """Interleaved groups over four masks, one without queries and one without rows: the caller's
    order, and the same as the per-query single-mask calls."""
    base, q = fc.gist_rows(2000, 12, 128)
    n = len(base)
    allow = np.stack([fc.random_mask(n, 0.3, 1), fc.random_mask(n, 0.05, 2), fc.random_mask(n, 0.5, 3), np.zeros(n, bool)])
    groups = np.array([0, 1, 3, 0, 1, 3, 1, 1, 0, 3, 0, 1])  # mask 2: no queries
    ref = fc.reference(orc, 0, base, q, 10, allow, groups=groups)
    dev = fc.cached(("shares-dev",), lambda: _dev(native, base))
    ids, dists = _search(dev, q, 10, allow, groups)
    fc.assert_same(ids, dists, *ref, what="groups")
    assert (ids[groups == 3] == fc.EMPTY).all()
    assert dev.flat_filtered_last()[0] == allow[0].sum() + allow[1].sum()  # the masks that had queries
    for a in range(len(q)):
        i1, d1 = _search(dev, q[a:a + 1], 10, allow[groups[a]])
        fc.assert_same(i1, d1, ids[a:a + 1], dists[a:a + 1], what=("single", a))
    with pytest.raises(Exception):  # more than one mask needs mask_of_query
        _search(dev, q, 10, allow)
    with pytest.raises(Exception):
        _search(dev, q, 10, allow, np.full(len(q), 4))


@pytest.mark.parametrize("n", [1, 31, 33, 2001])
def test_padding_and_tiny_bases(native, orc, n):
    """Raw words with every padding bit set, through the device entry: no id >= n.  An all-ones word
    sits next to a zero word."""
    import torch

    rng = np.random.default_rng(n)
    base = rng.standard_normal((n, 24), dtype=np.float32)
    q = rng.standard_normal((3, 24), dtype=np.float32)
    allow = fc.random_mask(n, 0.5, n)
    allow[0] = True
    if n > 96:
        allow[32:64] = True
        allow[64:96] = False
    words = fc.padding_words(n, allow)
    assert n % 32 == 0 or words[0, -1] >> (n % 32) != 0
    ref = fc.reference(orc, 0, base, q, 10, allow)
    dev = _dev(native, base)
    ids, dd, keep = _device_entry(dev, q, 10, words)
    torch.cuda.synchronize()
    ids, dd = _host(ids), _host(dd)
    assert ((ids < n) | (ids == fc.EMPTY)).all()
    fc.assert_same(ids, dd, *ref, what=n)
    assert dev.flat_filtered_last()[0] == allow.sum()
    hi, hd = dev.flat_search_filtered(q, 10, words)  # the host entry, same words
    fc.assert_same(hi, hd, *ref, what=(n, "host"))
    with pytest.raises(Exception):  # a mask of another length
        dev.flat_search_filtered(q, 10, np.zeros((1, (n + 31) // 32 + 1), np.uint32))


def test_validity_bitmap_keeps_rows_out(native, orc):
    base, q = fc.gist_rows(2000, 12, 128)
    n = len(base)
    allow = fc.random_mask(n, 0.3, 1)
    full = fc.reference(orc, 0, base, q, 10, allow)
    valid = np.ones(n, bool)
    valid[np.unique(full[0][:, :3])] = False  # the best three of every query: allowed, not valid
    ref = fc.reference(orc, 0, base, q, 10, allow, valid=valid)
    dev = _dev(native, base, 0, valid)
    ids, dists = _search(dev, q, 10, allow)
    fc.assert_same(ids, dists, *ref, what="valid")
    assert not np.isin(ids, np.nonzero(~valid)[0]).any()
    assert dev.flat_filtered_last()[0] == (allow & valid).sum()


# ---- Index level -----------------------------------------------------------------------------------
_N, _D, _NQ = 1000, 64, 12


def _index_data():
    rng = np.random.default_rng(64)
    return (np.ascontiguousarray(rng.standard_normal((_N, _D), dtype=np.float32)),
            np.ascontiguousarray(rng.standard_normal((_NQ, _D), dtype=np.float32)))


def _index_reference(orc, metric, rows, q, k, allow, valid=None, groups=None):
    if metric == "cos":
        rows = np.stack([orc.normalize(r) for r in rows])
        q = np.stack([orc.normalize(r) for r in q])
    return fc.reference(orc, 0 if metric == "l2" else 1, rows, q, k, allow, valid=valid, groups=groups)


@pytest.mark.parametrize("metric", ["l2", "ip", "cos"])
def test_index_exact_search_with_allow(orc, metric):
    """Index.exact_search(allow=): the three metrics, groups, filtered_search's argument checks, removed
    rows, and a mask of n + 1 bits after an insert."""
    import alayalite_amd

    base, q = _index_data()
    index = alayalite_amd.Client().create_index(f"ff_{metric}", metric=metric, capacity=_N + 10)
    index.fit(base.copy(), ef_construction=50, num_threads=1)
    allow = fc.random_mask(_N, 0.05, 3)
    ids, dists = index.exact_search(q.copy(), 10, allow=allow)
    assert ids.dtype == np.uint32 and ids.shape == (_NQ, 10) and dists.dtype == np.float32
    fc.assert_same(ids, dists, *_index_reference(orc, metric, base, q, 10, allow), what="one mask")
    # every row allowed: today's call
    ei, ed = index.exact_search(q.copy(), 10)
    ai, ad = index.exact_search(q.copy(), 10, allow=np.ones(_N, bool))
    fc.assert_same(ai, ad, ei, ed, what="all ones")
    two = np.stack([allow, fc.random_mask(_N, 0.5, 4)])
    groups = np.arange(_NQ) % 2
    ids, dists = index.exact_search(q.copy(), 10, allow=two, groups=groups)
    fc.assert_same(ids, dists, *_index_reference(orc, metric, base, q, 10, two, groups=groups), what="groups")
    for bad in (dict(allow=allow[:-1]), dict(allow=two), dict(allow=two, groups=groups[:-1]),
                dict(allow=two, groups=groups + 1), dict(allow=None, groups=groups)):
        with pytest.raises(ValueError):
            index.exact_search(q.copy(), 10, **bad)
    # removed rows are never returned even when allowed
    gone = int(ids[0, 0])
    index.remove(gone)
    valid = np.ones(_N, bool)
    valid[gone] = False
    ids, dists = index.exact_search(q.copy(), 10, allow=two, groups=groups)
    assert not (ids == gone).any()
    fc.assert_same(ids, dists, *_index_reference(orc, metric, base, q, 10, two, valid=valid, groups=groups), what="removed")
    # after an insert the mask has n + 1 bits, and the old length is refused
    row = (q[3] * np.float32(4.0 if metric == "ip" else 1.0)).copy()
    new_id = index.insert(row.copy())
    assert index.get_data_num() == _N + 1
    with pytest.raises(ValueError):
        index.exact_search(q.copy(), 10, allow=allow)
    allow2 = np.append(allow, True)
    rows2 = np.vstack([base, (orc.normalize(row) if metric == "cos" else row)[None]])
    ids, dists = index.exact_search(q.copy(), 10, allow=allow2)
    assert ids[3, 0] == new_id
    fc.assert_same(ids, dists, *_index_reference(orc, metric, rows2, q, 10, allow2, valid=np.append(valid, True)),
                   what="after insert")


def test_index_sq8_uint64_and_tiny(orc):
    """An SQ8 index is scanned on its f32 rows; a uint64 id type returns uint64 ids with its maximum in
    empty slots; the six-row index pads."""
    import alayalite_amd

    base, q = _index_data()
    allow = fc.random_mask(_N, 0.05, 3)
    ref_i, ref_d = _index_reference(orc, "ip", base, q, 10, allow)
    client = alayalite_amd.Client()
    sq = client.create_index("ffsq", metric="ip", capacity=_N, quantization_type="sq8")
    sq.fit(base.copy(), ef_construction=50, num_threads=1)
    ids, dists = sq.exact_search(q.copy(), 10, allow=allow)
    fc.assert_same(ids, dists, ref_i, ref_d, what="sq8")
    u64 = client.create_index("ffu64", metric="ip", capacity=_N, id_type=np.uint64)
    u64.fit(base.copy(), ef_construction=50, num_threads=1)
    few = np.zeros(_N, bool)
    few[[7, 70, 700]] = True
    ids, dists = u64.exact_search(q.copy(), 10, allow=few)
    assert ids.dtype == np.uint64 and (ids[:, 3:] == 0xFFFFFFFFFFFFFFFF).all() and (dists[:, 3:] == fc.FLT_MAX).all()
    fi, fd = _index_reference(orc, "ip", base, q, 10, few)
    assert np.array_equal(ids[:, :3], fi[:, :3].astype(np.uint64)) and np.array_equal(dists.view(np.uint32), fd.view(np.uint32))
    rng = np.random.default_rng(5)
    tiny = rng.random((6, 32), dtype=np.float32)
    for id_type, top in ((np.uint32, 0xFFFFFFFF), (np.uint64, 0xFFFFFFFFFFFFFFFF)):
        index = alayalite_amd.Client().create_index("tiny", metric="ip", capacity=8, id_type=id_type)
        index.fit(tiny.copy(), ef_construction=20, num_threads=1)
        ids, dists = index.exact_search(tiny[:2].copy(), 10, allow=np.array([1, 1, 0, 1, 1, 1], bool))
        assert (ids[:, 5:] == top).all() and (dists[:, 5:] == fc.FLT_MAX).all()
        assert sorted(ids[0, :5].tolist()) == [0, 1, 3, 4, 5]


def test_calc_gt_device_with_allow(orc):
    import alayalite_amd

    base, q = _index_data()
    allow = fc.random_mask(_N, 0.05, 3)
    rows = np.nonzero(allow)[0]
    for metric in ("l2", "cos"):
        ids, dists = alayalite_amd.utils.calc_gt_device(base, q, 10, metric=metric, allow=allow)
        si, sd = alayalite_amd.utils.calc_gt_device(base[rows], q, 10, metric=metric)
        assert ids.dtype == np.int32 and np.array_equal(ids, rows[si].astype(np.int32))
        assert np.array_equal(dists.view(np.uint32), sd.view(np.uint32))
    ref_i, ref_d = _index_reference(orc, "l2", base, q, 10, allow)
    ids, dists = alayalite_amd.utils.calc_gt_device(base, q, 10, allow=allow)
    fc.assert_same(ids.view(np.uint32), dists, ref_i, ref_d, what="calc_gt_device")


def test_device_entry_twice_on_one_torch_stream(native, orc):
    """Two calls with different masks (and chunk counts) back to back on one side stream, no
    synchronisation between them: the second reuses the first's scratch only after it."""
    import torch

    base, q = fc.gist_rows(2000, 12, 128)
    n = len(base)
    a1, a2 = fc.random_mask(n, 0.5, 31), fc.random_mask(n, 0.05, 2)
    two = np.stack([a1, a2])
    groups = np.arange(len(q)) % 2
    ref1 = fc.cached(("shares-ref", 0.5), lambda: fc.reference(orc, 0, base, q, 10, a1))
    ref2 = fc.reference(orc, 0, base, q, 10, a2)
    ref3 = fc.reference(orc, 0, base, q, 10, two, groups=groups)
    dev = fc.cached(("shares-dev",), lambda: _dev(native, base))
    side = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(side):
        i1, d1, k1 = _device_entry(dev, q, 10, pack_allow(a1, n))
        i2, d2, k2 = _device_entry(dev, q, 10, pack_allow(a2, n))
        i3, d3, k3 = _device_entry(dev, q, 10, pack_allow(two, n), groups)
    side.synchronize()
    fc.assert_same(_host(i1), _host(d1), *ref1, what="first")
    fc.assert_same(_host(i2), _host(d2), *ref2, what="second")
    fc.assert_same(_host(i3), _host(d3), *ref3, what="groups")
    assert dev.flat_filtered_last()[0] == a1.sum() + a2.sum()
