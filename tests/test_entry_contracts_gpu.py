"""What the search entry points share on the host side, as a table: the refusals of the filtered calls
(mask shape, mask indices, k), the agreement of every host call with its ``*_device`` twin on torch
buffers, and the widening of empty ids to a 64-bit id type.  The kernels are not under test here (the
filter and flat-filtered files compare them with their restatements): the shapes are the smallest that
carry two masks, per-query indices, a second query form for the SQ8 rerank and an empty result slot.

200 rows of 16 floats under L2, 5 queries, k = 4, ef = 8; masks of shares 0.5 and 0.1 with per-query
indices [0, 1, 0, 1, 1]; a DeviceIndex over a host-built graph of degree 8, a second one with the SQ8
codes of the same rows, and PyIndexInterface indexes (their own host-built graph, degree 32) over the
same rows."""

import numpy as np
import pytest

import filter_common as fc

pytestmark = pytest.mark.gpu

N, D, NQ, K, EF = 200, 16, 5, 4, 8
GROUPS = np.array([0, 1, 0, 1, 1], np.uint32)
EMPTY64 = 2**64 - 1
_state = {}


def _rows():
    rng = np.random.default_rng(0)
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((NQ, D)).astype(np.float32)


def _words(allow):
    from alayalite_amd.utils import pack_allow

    return pack_allow(np.asarray(allow), N)


def _two_masks():
    return _words(np.stack([fc.mask(N, 0.5), fc.mask(N, 0.1)]))


def _devices(native):
    """(f32 DeviceIndex, SQ8 DeviceIndex) over the same rows and graph."""
    if "dev" not in _state:
        base, _ = _rows()
        graph = native.Graph.build(base, 0, 8, 100, 1, 100)
        plain = native.DeviceIndex(0)
        plain.set_base(base, 0, None)
        plain.set_graph(graph)
        sq8 = native.DeviceIndex(0)
        sq8.set_base(base, 0, None)
        sq8.set_graph(graph)
        mn, mx = native.sq8_train(base)
        sq8.set_sq8(native.sq8_encode(base, mn, mx, 1), mn, mx, native.host_sq8_order())
        _state["dev"] = (plain, sq8)
    return _state["dev"]


def _index(native, sq8, id_type=np.uint32):
    key = ("index", sq8, np.dtype(id_type).name)
    if key not in _state:
        params = native.IndexParams(native.IndexType.HNSW, np.dtype(np.float32), np.dtype(id_type),
                                    native.QuantizationType.SQ8 if sq8 else native.QuantizationType.NONE,
                                    native.MetricType.L2, N)
        index = native.PyIndexInterface(params)
        index.fit(_rows()[0].copy(), 100, 1, "host")
        _state[key] = index
    return _state[key]


# ---- refusals on the host calls ---------------------------------------------------------------------
# name -> call(native, queries, k, allow_words, mask_of_query)
HOST_CALLS = {
    "DeviceIndex.filtered_search": lambda nat, q, k, w, g: _devices(nat)[0].filtered_search(q, k, EF, w, g),
    "DeviceIndex.filtered_search_hop": lambda nat, q, k, w, g: _devices(nat)[0].filtered_search_hop(q, k, EF, w, g),
    "DeviceIndex.filtered_search_sq8": lambda nat, q, k, w, g: _devices(nat)[1].filtered_search_sq8(q, k, EF, w, g),
    "DeviceIndex.flat_search_filtered": lambda nat, q, k, w, g: _devices(nat)[0].flat_search_filtered(q, k, w, g),
    "PyIndexInterface.filtered_search": lambda nat, q, k, w, g: _index(nat, False).filtered_search(q, k, EF, w, g),
    "PyIndexInterface.filtered_search[through]":
        lambda nat, q, k, w, g: _index(nat, False).filtered_search(q, k, EF, w, g, 0, True),
    "PyIndexInterface.filtered_search[sq8]": lambda nat, q, k, w, g: _index(nat, True).filtered_search(q, k, EF, w, g),
    "PyIndexInterface.exact_search_filtered":
        lambda nat, q, k, w, g: _index(nat, False).exact_search_filtered(q, k, w, g),
}

# name -> (k, allow_words, mask_of_query) of a call that must raise ValueError
REFUSED = {
    "a mask row one word short": lambda: (K, _two_masks()[:, :-1].copy(), GROUPS),
    "two masks without indices": lambda: (K, _two_masks(), None),
    "an index equal to n_masks": lambda: (K, _two_masks(), np.array([0, 1, 0, 1, 2], np.uint32)),
    "indices of length nq - 1": lambda: (K, _two_masks(), GROUPS[:NQ - 1].copy()),
    "k = 225": lambda: (225, _two_masks(), GROUPS),
    "k = 0": lambda: (0, _two_masks(), GROUPS),
}


@pytest.mark.parametrize("refused", list(REFUSED))
@pytest.mark.parametrize("call", list(HOST_CALLS))
def test_host_call_refuses(native, call, refused):
    k, words, groups = REFUSED[refused]()
    with pytest.raises(ValueError):
        HOST_CALLS[call](native, _rows()[1].copy(), k, words, groups)
    # the same call with nothing wrong goes through (the refusal above was not the index's state)
    out = HOST_CALLS[call](native, _rows()[1].copy(), K, _two_masks(), GROUPS)
    assert np.asarray(out[0]).shape == (NQ, K)


# ---- the *_device calls on torch buffers ------------------------------------------------------------
def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _device_call(native, kind, words, groups, rerank=None, n_masks=None, null_indices=False):
    """The ``*_device`` twin of ``kind`` on the current torch stream: (ids, dist bits, counters or None,
    n_through or None) as numpy arrays.  n_masks / null_indices override what is passed for the refusal cases."""
    torch, d0 = _torch()
    plain, sq8 = _devices(native)
    q = _rows()[1]
    qd = torch.from_numpy(q).to(d0)
    wd = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(d0)
    gd = None if groups is None else torch.from_numpy(np.ascontiguousarray(groups).view(np.int32)).to(d0)
    rd = None if rerank is None else torch.from_numpy(rerank).to(d0)
    ids = torch.full((NQ, K), 7, dtype=torch.int32, device=d0)
    dd = torch.full((NQ, K), 7.0, dtype=torch.float32, device=d0)
    cc = torch.full((NQ, 4), 7, dtype=torch.int32, device=d0)
    tt = torch.full((NQ,), 7, dtype=torch.int32, device=d0)
    s = torch.cuda.current_stream(d0).cuda_stream
    nm = words.shape[0] if n_masks is None else n_masks
    gp = 0 if gd is None or null_indices else gd.data_ptr()
    if kind == "plain":
        plain.filtered_search_device(qd.data_ptr(), NQ, K, EF, wd.data_ptr(), nm, gp, ids.data_ptr(), dd.data_ptr(),
                                     cc.data_ptr(), s)
    elif kind == "through":
        plain.filtered_search_hop_device(qd.data_ptr(), NQ, K, EF, wd.data_ptr(), nm, gp, ids.data_ptr(), dd.data_ptr(),
                                         cc.data_ptr(), tt.data_ptr(), s)
    elif kind == "sq8":
        sq8.filtered_search_sq8_device(qd.data_ptr(), 0 if rd is None else rd.data_ptr(), NQ, K, EF, 0, wd.data_ptr(), nm,
                                       gp, ids.data_ptr(), dd.data_ptr(), cc.data_ptr(), s)
    else:
        plain.flat_search_filtered_device(qd.data_ptr(), NQ, K, wd.data_ptr(), nm, gp, ids.data_ptr(), dd.data_ptr(), s)
    torch.cuda.synchronize(d0)
    return (_u32(ids), _u32(dd), _u32(cc) if kind != "flat" else None, _u32(tt) if kind == "through" else None)


def _host_call(native, kind, words, groups, rerank=None):
    plain, sq8 = _devices(native)
    q = _rows()[1]
    if kind == "plain":
        ids, d, c = plain.filtered_search(q, K, EF, words, groups)
        t = None
    elif kind == "through":
        ids, d, c, t = plain.filtered_search_hop(q, K, EF, words, groups)
    elif kind == "sq8":
        ids, d, c = sq8.filtered_search_sq8(q, K, EF, words, groups, 0, rerank)
        t = None
    else:
        ids, d = plain.flat_search_filtered(q, K, words, groups)
        c = t = None
    return ids, d.view(np.uint32), c, t


def _assert_same(got, want, what):
    for name, g, w in zip(("ids", "distance bits", "counters", "n_through"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            assert g.dtype == np.uint32 and w.dtype == np.uint32, (what, name, g.dtype, w.dtype)
            assert np.array_equal(g, w), (what, name, g, w)


def _rerank_queries():
    """A second query form for the SQ8 rerank: not the queries, so an upload that took the wrong array shows."""
    return (_rows()[1] + np.float32(0.25)).astype(np.float32)


KINDS = ["plain", "through", "sq8", "sq8 with rerank queries", "flat"]


def _split(kind):
    return ("sq8", _rerank_queries()) if kind == "sq8 with rerank queries" else (kind, None)


@pytest.mark.parametrize("masks", ["two masks and indices", "one mask and None"])
@pytest.mark.parametrize("kind", KINDS)
def test_host_and_device_calls_agree(native, kind, masks):
    kind, rerank = _split(kind)
    words, groups = (_two_masks(), GROUPS) if masks.startswith("two") else (_words(fc.mask(N, 0.5)), None)
    host = _host_call(native, kind, words, groups, rerank)
    dev = _device_call(native, kind, words, groups, rerank)
    _assert_same(dev, host, (kind, masks))
    assert (host[0] != fc.EMPTY).any()  # (the comparison is not one of empty slots)
    if rerank is not None:  # the second query form reached the rerank: the distances are not those of the queries
        assert not np.array_equal(host[1], _host_call(native, kind, words, groups)[1])


@pytest.mark.parametrize("refused", ["two masks, null mask_of_query", "n_masks = 0"])
@pytest.mark.parametrize("kind", ["plain", "through", "sq8", "flat"])
def test_device_call_refuses_and_recovers(native, kind, refused):
    words = _two_masks()
    before = _device_call(native, kind, words, GROUPS)
    with pytest.raises(ValueError):
        if refused == "n_masks = 0":
            _device_call(native, kind, words, GROUPS, n_masks=0)
        else:
            _device_call(native, kind, words, GROUPS, null_indices=True)
    _assert_same(_device_call(native, kind, words, GROUPS), before, (kind, refused))


# ---- id widening ------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["filtered_search", "filtered_search[sq8]", "exact_search_filtered"])
def test_empty_slots_widen_to_the_id_types_maximum(native, call):
    allow = np.zeros(N, bool)
    allow[[17, 120]] = True
    words = _words(allow)
    q = _rows()[1].copy()
    if call == "exact_search_filtered":
        ids, d = _index(native, False, np.uint64).exact_search_filtered(q, K, words, None)
    else:
        ids, d = _index(native, call.endswith("[sq8]"), np.uint64).filtered_search(q, K, EF, words, None)
    assert ids.dtype == np.uint64 and ids.shape == (NQ, K)
    assert (ids[:, K - 2:] == EMPTY64).all(), ids
    assert (d[:, K - 2:] == fc.FLT_MAX).all(), d
    assert np.isin(ids[:, :K - 2], np.array([17, 120, EMPTY64], np.uint64)).all(), ids
    if call == "exact_search_filtered":  # the scan finds both rows, whatever the graph reaches
        assert (np.sort(ids[:, :2], axis=1) == [17, 120]).all(), ids
