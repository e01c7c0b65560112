"""Exact k-NN over per-query candidate lists on the device (alaya_index_flat_search_lists*): the piece table,
the gather-and-select scan, the merge.  The expected answer is flat_filtered_common.reference with one mask per
query that allows the list's in-range ids -- the oracle's reference-order distances over the unique, valid ids,
by (distance, id), cut at k.  Every comparison is array_equal on ids and on distance bits."""

import numpy as np
import pytest

import flat_filtered_common as fc

pytestmark = pytest.mark.gpu

PIECE_ENV = "ALAYA_FLAT_LISTS_PIECE"
N, NQ, PIECE = 3000, 7, 64  # the forced piece: the longer lists take several, so the merge runs


@pytest.fixture(autouse=True)
def _forced_piece(monkeypatch):
    monkeypatch.setenv(PIECE_ENV, str(PIECE))


def _rows(dim, integer=False):
    """(base, queries); integer: values in {0, 1, 2}, so many distances are equal and the id decides."""
    def make():
        rng = np.random.default_rng(dim)
        if integer:
            return tuple(rng.integers(0, 3, (r, dim)).astype(np.float32) for r in (N, NQ))
        return tuple(rng.standard_normal((r, dim), dtype=np.float32) for r in (N, NQ))
    return fc.cached(("lists-rows", dim, integer), make)


def _lists(k, n=N):
    """One list per query: 0, 1, k - 1, k, piece + 1, 5 pieces + 3 and 100 random ids, repeats included."""
    rng = np.random.default_rng(k)
    return [rng.integers(0, n, m) for m in (0, 1, k - 1, k, PIECE + 1, 5 * PIECE + 3, 100)]


def _csr(lists, dtype=np.int64):
    lims = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return lims, np.concatenate(lists).astype(dtype)


def _reference(orc, metric, base, q, k, lists, valid=None):
    allow = np.zeros((len(lists), len(base)), bool)
    for a, ids in enumerate(lists):
        allow[a, ids[ids < len(base)]] = True
    return fc.reference(orc, metric, base, q, k, allow, valid=valid, groups=np.arange(len(lists)))


def _dev(native, base, metric=0):
    dev = native.DeviceIndex(0)
    dev.set_base(np.ascontiguousarray(base, np.float32), metric)
    return dev


@pytest.mark.parametrize("k", [1, 10, 224])
@pytest.mark.parametrize("metric", ["l2", "ip", "cos"])
@pytest.mark.parametrize("dim", [20, 128, 960])
def test_widths_metrics_and_lengths(orc, dim, metric, k):
    """calc_gt_device(candidates=): a tail below one 32-block, one flat width and the slabbed width; list lengths
    from empty over k - 1 and k to one entry past a piece and past five pieces, in one call."""
    from alayalite_amd.utils import calc_gt_device

    base, q = _rows(dim)
    unit = (base, q)
    if metric == "cos":  # the reference's rows and queries, normalised as fit normalises them
        unit = fc.cached(("lists-unit", dim), lambda: tuple(np.stack([orc.normalize(r) for r in a]) for a in (base, q)))
    lists = _lists(k)
    ref_i, ref_d = _reference(orc, 0 if metric == "l2" else 1, *unit, k, lists)
    ids, dists = calc_gt_device(base, q, k, metric=metric, candidates=_csr(lists, np.int32))
    assert ids.dtype == np.int32
    fc.assert_same(ids.view(np.uint32), dists, ref_i, ref_d, what=(dim, metric, k))
    filled = np.minimum([len(np.unique(x)) for x in lists], k)
    assert all((ids[a, f:] == -1).all() and (dists[a, f:] == fc.FLT_MAX).all() for a, f in enumerate(filled))


@pytest.mark.parametrize("metric", [0, 1])
def test_duplicates_and_ties(native, orc, metric):
    """Every id twice and one id nine times, across piece boundaries, on rows whose distances tie: a row counts
    once, in a piece and in the merge, and equal distances go to the smaller id."""
    base, q = _rows(40, integer=True)
    rng = np.random.default_rng(3)
    lists = []
    for a in range(NQ):
        some = rng.choice(N, 150, replace=False)
        lists.append(rng.permutation(np.concatenate([some, some, np.repeat(some[:1], 7)])))
    ref = _reference(orc, metric, base, q, 50, lists)
    assert any(len(np.unique(d[:50])) < 40 for d in ref[1])  # the answer holds ties
    ids, dists = _dev(native, base, metric).flat_search_lists(q, 50, *_csr(lists))
    fc.assert_same(ids, dists, *ref, what=metric)


def _index(kind):
    """A 1000 x 64 IP index: f32 with removed rows, uint64 ids, SQ8 codes."""
    import alayalite_amd

    def make():
        base, q = (a[:1000, :64].copy() for a in (_rows(128)[0], np.resize(_rows(128)[1], (12, 128))))
        extra = dict(id_type=np.uint64) if kind == "uint64" else dict(quantization_type="sq8") if kind == "sq8" else {}
        index = alayalite_amd.Client().create_index(f"lists_{kind}", metric="ip", capacity=1000, **extra)
        index.fit(base.copy(), ef_construction=50, num_threads=1)
        valid = np.ones(1000, bool)
        if kind == "removed":
            valid[::7] = False
            for i in np.nonzero(~valid)[0]:
                index.remove(int(i))
        return index, base, q, valid
    return fc.cached(("lists-index", kind), make)


@pytest.mark.parametrize("kind", ["removed", "uint64", "sq8"])
def test_index_kinds_and_batch_splitting(orc, kind):
    """Index.exact_search(candidates=): removed rows inside the lists are skipped, ids come in the index's id type,
    an SQ8 index is scanned on its f32 rows -- and five queries at a time give the same bytes."""
    index, base, q, valid = _index(kind)
    lists = (_lists(10, 1000) * 2)[:12]
    ref_i, ref_d = _reference(orc, 1, base, q, 10, lists, valid=valid)
    ids, dists = index.exact_search(q.copy(), 10, candidates=_csr(lists))
    assert ids.dtype == (np.uint64 if kind == "uint64" else np.uint32)
    top = np.iinfo(ids.dtype).max
    assert np.array_equal(ids, np.where(ref_i == fc.EMPTY, top, ref_i.astype(ids.dtype)))
    assert np.array_equal(dists.view(np.uint32), ref_d.view(np.uint32))
    si, sd = index.exact_search(q.copy(), 10, candidates=_csr(lists, np.uint16), _chunk=5)
    assert si.tobytes() == ids.tobytes() and sd.tobytes() == dists.tobytes()


def test_piece_length_changes_nothing(native, orc, monkeypatch):
    base, q = _rows(128)
    lists = _lists(10)
    ref = _reference(orc, 0, base, q, 10, lists)
    dev = _dev(native, base)
    for piece in (64, 512, None):
        if piece is None:
            monkeypatch.delenv(PIECE_ENV)
        else:
            monkeypatch.setenv(PIECE_ENV, str(piece))
        ids, dists = dev.flat_search_lists(q, 10, *_csr(lists))
        fc.assert_same(ids, dists, *ref, what=piece)
        total, got, table, launches = dev.flat_lists_last()
        assert total == sum(map(len, lists)) and got == (piece or 64) and table == total // got + NQ and launches == 1


def test_device_entry_and_ids_past_the_rows(native):
    """flat_search_lists_device on torch buffers equals the host call; ids >= n planted in the device lists are
    skipped -- the bound holds, the other slots are unchanged and the call returns."""
    import torch

    base, q = _rows(128)
    lists = _lists(10)
    dev = _dev(native, base)
    want_i, want_d = dev.flat_search_lists(q, 10, *_csr(lists))
    planted = [np.concatenate([x[:len(x) // 2], [N, N + 5, 0xFFFFFFFF], x[len(x) // 2:]]) for x in lists]
    d0 = torch.device("cuda", 0)
    qd = torch.from_numpy(q.copy()).to(d0)
    for these in (lists, planted):
        lims, cand = _csr(these, np.uint32)
        ld, cd = torch.from_numpy(lims).to(d0), torch.from_numpy(cand.view(np.int32)).to(d0)
        ids = torch.full((NQ, 10), 7, dtype=torch.int32, device=d0)
        dd = torch.full((NQ, 10), 7.0, dtype=torch.float32, device=d0)
        dev.flat_search_lists_device(qd.data_ptr(), NQ, 10, ld.data_ptr(), cd.data_ptr(), len(cand), ids.data_ptr(),
                                     dd.data_ptr(), torch.cuda.current_stream(d0).cuda_stream)
        torch.cuda.synchronize()
        fc.assert_same(ids.cpu().numpy().view(np.uint32), dd.cpu().numpy(), want_i, want_d, what=len(cand))


def test_refusals(native):
    import alayalite_amd

    index, base, q, _ = _index("sq8")
    lims, cand = _csr((_lists(10, 1000) * 2)[:12])
    down = lims.copy()
    down[3] = down[2] - 1
    for bad in (dict(candidates=(lims, cand), allow=np.ones(1000, bool)), dict(candidates=(lims, cand), topk=0),
                dict(candidates=(lims, cand), topk=225), dict(candidates=(down, cand)), dict(candidates=(lims[:-1], cand)),
                dict(candidates=(lims, np.where(cand == cand[5], 1000, cand)))):
        with pytest.raises(ValueError):
            index.exact_search(q.copy(), **{"topk": 10, **bad})
    dev = _dev(native, base)
    for args in ((q, 10, down, cand), (q, 10, lims[:-1], cand), (q, 10, lims, cand + 1000), (q, 0, lims, cand), (q, 225, lims, cand)):
        with pytest.raises(ValueError):  # the library's own checks (ALAYA_ERR_ARG)
            dev.flat_search_lists(*args)
    rows = np.random.default_rng(6).integers(-100, 100, (500, 32)).astype(np.int8)
    i8 = alayalite_amd.Client().create_index("lists_i8", capacity=500, data_type=np.int8)
    i8.fit(rows, ef_construction=50, num_threads=1)
    with pytest.raises(ValueError, match="float32"):
        i8.exact_search(rows[:4].copy(), 5, candidates=(np.arange(5) * 3, np.arange(12)))
