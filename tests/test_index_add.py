"""Index.add: rows appended in bulk through the batched device build (alaya_index_extend_graph behind
PyIndexInterface.add), on the public API.

  * fit(first n0, builder="gpu") + add(rest) at a batch boundary n0 is fit(all, builder="gpu"):
    the graph arrays and batch_search_with_distance (ids, distance bits), L2 and COS;
  * SQ8: the device-encoded codes of the new rows are oracle.sq8_encode's under the fitted range, byte
    for byte, values outside the range included; the old rows' codes stay; searches agree with an
    index that holds the host encoder's codes;
  * after insert and remove: no new row links to a removed row on any level, the removed rows' lists
    stay, searches never return them, exact_search is the brute force over the valid rows, and
    insert / remove go on working;
  * recall after removals against an index fitted in one go on the same rows;
  * save / load, the capacity limit, empty and malformed inputs, filtered_search over the new length."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF


def _client(tmp=None):
    import alayalite_amd

    return alayalite_amd.Client(str(tmp)) if tmp is not None else alayalite_amd.Client()


def _boundary(native, levels, lo):
    """The first batch end >= lo of fit(builder="gpu")'s schedule (seed 100, the default sizes)."""
    ends = native.build_batches(np.ascontiguousarray(levels, np.uint32), 1, 0, 0, 0).tolist()
    got = [e for e in ends[:-1] if e >= lo]
    assert got
    return got[0]


def _lists_of(arrays, i):
    """Every adjacency list of row i: level 0 first."""
    l0, levels, off, ue, _, upper_r = arrays[:6]
    out = [l0[i]]
    for lv in range(int(levels[i])):
        out.append(ue[int(off[i]) + lv * upper_r: int(off[i]) + (lv + 1) * upper_r])
    return out


# ---- equality at a boundary ----------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_fit_then_add_at_a_boundary_is_fit_of_all(native, metric):
    rng = np.random.default_rng(5)
    data = rng.standard_normal((2000, 32)).astype(np.float32)
    q = rng.standard_normal((30, 32)).astype(np.float32)
    c = _client()
    whole = c.create_index(f"add_whole_{metric}", metric=metric, capacity=2000)
    whole.fit(data.copy(), ef_construction=100, builder="gpu")
    ref = whole.native().graph_arrays()
    n0 = _boundary(native, ref[1], 1000)
    assert 1000 <= n0 < 1200
    part = c.create_index(f"add_part_{metric}", metric=metric, capacity=2000)
    part.fit(data[:n0].copy(), ef_construction=100, builder="gpu")
    ids = part.add(data[n0:].copy(), ef_construction=100)
    assert ids.dtype == np.uint32 and np.array_equal(ids, np.arange(n0, 2000))
    assert part.get_data_num() == 2000
    for a, b in zip(part.native().graph_arrays(), ref):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    got = part.batch_search_with_distance(q.copy(), 10, 64)
    want = whole.batch_search_with_distance(q.copy(), 10, 64)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(part.get_data_by_id(1999), whole.get_data_by_id(1999))


# ---- SQ8 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,lo", [(70, 1500, 1000), (24, 700, 300)])
def test_sq8_codes_of_added_rows(native, orc, d, n, lo):
    """d = 70 and 24 are no multiples of 64 (the code row stride) or of 4 (the kernel's store width
    covers 4 codes); the counts are no multiples of the kernel's block."""
    rng = np.random.default_rng(d)
    data = rng.random((n, d), dtype=np.float32)
    c = _client()
    probe = c.create_index(f"sq_probe_{d}", capacity=n)
    probe.fit(data.copy(), builder="gpu")
    n0 = _boundary(native, probe.native().graph_arrays()[1], lo)
    new = rng.uniform(-0.3, 1.3, (n - n0, d)).astype(np.float32)  # below and above the fitted [0, 1)
    new[0, :] = data[:n0].max(axis=0)  # exactly the fitted maximum: code 255
    new[1, :] = data[:n0].min(axis=0)  # exactly the fitted minimum: code 0
    idx = c.create_index(f"sq_add_{d}", quantization_type="sq8", capacity=n)
    idx.fit(data[:n0].copy(), builder="gpu")
    mn, mx = idx.native().sq8_range()
    assert np.array_equal(mn, data[:n0].min(axis=0)) and np.array_equal(mx, data[:n0].max(axis=0))
    old = idx.native().sq8_codes()
    assert np.array_equal(old, orc.sq8_encode(data[:n0], mn, mx))
    ids = idx.add(new.copy())
    assert np.array_equal(ids, np.arange(n0, n))
    codes = idx.native().sq8_codes()
    assert codes.shape == (n, d)
    assert np.array_equal(codes[:n0], old)
    want = orc.sq8_encode(new, mn, mx)
    assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()
    assert (want[0] == 255).all() and (want[1] == 0).all()
    assert np.array_equal(codes[n0:], want)
    # searches: the same graph and rows under the host encoder's codes
    rows = np.concatenate([data[:n0], new])
    # queries: ten in the fitted range, ten beside new rows (which lie far out in the clamped corners)
    q = np.concatenate([rng.random((10, d), dtype=np.float32),
                        new[5:15] + rng.normal(0, 0.01, (10, d)).astype(np.float32)])
    l0, levels, off, ue, ep, upper_r, _ = idx.native().graph_arrays()
    twin = native.DeviceIndex(0)
    twin.set_base(rows, 0, None)
    twin.set_graph(native.Graph.from_arrays(l0, levels, off, ue, upper_r, ep, None))
    twin.set_sq8(native.sq8_encode(rows, mn, mx, 1), mn, mx, native.host_sq8_order())
    got = idx.batch_search(q.copy(), 10, 64)
    assert np.array_equal(got, twin.search_sq8(q, 10, 64, 1, q)[0])
    assert (got >= n0).any()


# ---- after insert and remove ---------------------------------------------------------------------
def _updated_index(c, name, data, seed):
    """fit(600, host) + 3 inserts + 5 removes (one of them the row with the most in-links)."""
    idx = c.create_index(name, capacity=1100)
    idx.fit(data[:600].copy(), ef_construction=100, num_threads=1, builder="host")
    for i in range(600, 603):
        assert idx.insert(data[i].copy(), 64) == i
    l0 = idx.native().graph_arrays()[0]
    live = l0[l0 != EMPTY]
    rich = int(np.argmax(np.bincount(live, minlength=603)))
    rng = np.random.default_rng(seed)
    removed = [rich] + [int(r) for r in rng.choice([i for i in range(603) if i != rich], 4, replace=False)]
    for r in removed:
        idx.remove(r)
    return idx, removed


def test_add_after_insert_and_remove(native):
    rng = np.random.default_rng(8)
    data = rng.standard_normal((1004, 24)).astype(np.float32)
    q = rng.standard_normal((40, 24)).astype(np.float32)
    idx, removed = _updated_index(_client(), "add_upd", data, 1)
    before = idx.native().graph_arrays()
    ids = idx.add(data[603:1003].copy())
    assert np.array_equal(ids, np.arange(603, 1003)) and idx.get_data_num() == 1003
    after = idx.native().graph_arrays()
    gone = set(removed)
    for i in range(603, 1003):
        for lst in _lists_of(after, i):
            live = lst[lst != EMPTY].tolist()
            assert not gone & set(live), (i, live)
            assert i not in live and all(v < 1003 for v in live)
    for r in removed:
        for a, b in zip(_lists_of(before, r), _lists_of(after, r)):
            assert np.array_equal(a, b), r
    got = idx.batch_search(q.copy(), 10, 64)
    assert not gone & set(got.ravel().tolist())
    assert (got >= 603).any()
    valid = np.array([i for i in range(1003) if i not in gone])
    e_ids, e_d = idx.exact_search(q.copy(), 10)
    dist = ((data[valid][None, :, :].astype(np.float64) - q[:, None, :]) ** 2).sum(-1)
    want = valid[np.argsort(dist, axis=1, kind="stable")[:, :10]]
    assert np.array_equal(e_ids, want)
    assert np.allclose(e_d, np.sort(dist, axis=1)[:, :10], rtol=1e-5)
    # updates go on: the next id is n, and the new row is found
    assert idx.insert(data[1003].copy(), 64) == 1003
    assert idx.batch_search(data[1003:1004].copy(), 1, 64)[0, 0] == 1003
    idx.remove(700)
    assert 700 not in idx.batch_search(data[700:701].copy(), 10, 64)[0].tolist()


# ---- recall after removals -----------------------------------------------------------------------
# recall@10 at ef 32 against exact_search of the same index, three data seeds, measured on the MI355X
# ("Bulk growth").  The allowed shortfall of the grown index is the spread (max - min) of
# the one-go fit's recall across the seeds: what the data alone moves the figure by.  Measured
# (grown, one-go): seed 11 0.9620 / 0.9670, seed 12 0.9660 / 0.9705, seed 13 0.9630 / 0.9625.
ONE_GO_RECALL = {11: 0.9670, 12: 0.9705, 13: 0.9625}
SHORTFALL = max(ONE_GO_RECALL.values()) - min(ONE_GO_RECALL.values())  # 0.0080


def _recalls(seed):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((2000, 32)).astype(np.float32)
    q = rng.standard_normal((200, 32)).astype(np.float32)
    removed = rng.choice(1200, 100, replace=False)
    c = _client()
    grown = c.create_index(f"rec_grown_{seed}", capacity=2000)
    grown.fit(data[:1200].copy(), builder="gpu")
    for r in removed:
        grown.remove(int(r))
    grown.add(data[1200:].copy())
    keep = np.setdiff1d(np.arange(2000), removed)
    whole = c.create_index(f"rec_whole_{seed}", capacity=2000)
    whole.fit(data[keep].copy(), builder="gpu")
    out = []
    for idx in (grown, whole):
        gt = idx.exact_search(q.copy(), 10)[0]
        ids = idx.batch_search(q.copy(), 10, 32)
        out.append(float(np.mean([len(set(a.tolist()) & set(b.tolist())) / 10 for a, b in zip(ids, gt)])))
    return out


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_recall_after_removals_close_to_one_go_fit(seed):
    grown, whole = _recalls(seed)
    print(f"recall@10 ef 32 seed {seed}: grown {grown:.4f} one-go {whole:.4f}")
    assert grown >= whole - SHORTFALL, (grown, whole)


# ---- persistence and limits ----------------------------------------------------------------------
@pytest.mark.parametrize("quant", ["none", "sq8"])
def test_save_load_after_add(native, tmp_path, quant):
    rng = np.random.default_rng(21)
    data = rng.random((900, 40), dtype=np.float32)
    q = rng.random((10, 40), dtype=np.float32)
    c = _client(tmp_path)
    idx = c.create_index(f"persist_{quant}", quantization_type=quant, capacity=1000)
    idx.fit(data[:500].copy(), builder="gpu")
    if quant == "none":
        idx.remove(17)
    idx.add(data[500:].copy())
    c.save_index(f"persist_{quant}")
    again = _client(tmp_path).get_index(f"persist_{quant}")
    assert again.get_data_num() == 900
    for a, b in zip(again.native().graph_arrays(), idx.native().graph_arrays()):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert np.array_equal(again.get_data_by_id(899), data[899])
    assert np.array_equal(again.batch_search(q.copy(), 10, 64), idx.batch_search(q.copy(), 10, 64))
    assert np.array_equal(again.exact_search(q.copy(), 10)[0], idx.exact_search(q.copy(), 10)[0])
    if quant == "sq8":
        assert np.array_equal(again.native().sq8_codes(), idx.native().sq8_codes())
    else:
        assert 17 not in again.exact_search(data[17:18].copy(), 5)[0][0].tolist()  # the bitmap travelled


def test_limits_and_malformed_inputs(native):
    rng = np.random.default_rng(22)
    data = rng.random((800, 16), dtype=np.float32)
    q = rng.random((10, 16), dtype=np.float32)
    idx = _client().create_index("add_limits", capacity=700)
    idx.fit(data[:500].copy(), builder="gpu")
    before = idx.batch_search_with_distance(q.copy(), 10, 64)
    with pytest.raises(RuntimeError, match="The index is full"):
        idx.add(data[500:701].copy())
    assert idx.get_data_num() == 500
    empty = idx.add(np.zeros((0, 16), np.float32))
    assert empty.shape == (0,) and empty.dtype == np.uint32 and idx.get_data_num() == 500
    with pytest.raises(ValueError):
        idx.add(np.zeros((3, 17), np.float32))
    with pytest.raises(ValueError):
        idx.add(np.zeros(16, np.float32))
    with pytest.raises(ValueError):
        idx.add(np.zeros((3, 16), np.float64))
    after = idx.batch_search_with_distance(q.copy(), 10, 64)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    ids = idx.add(data[500:700].copy())  # exactly to capacity
    assert ids[0] == 500 and ids[-1] == 699 and idx.get_data_num() == 700
    with pytest.raises(RuntimeError):
        idx.add(data[700:701].copy())
    # filtered_search takes a mask of the new length and can return new rows
    allow = np.zeros(700, bool)
    allow[500:] = True
    f_ids, f_d = idx.filtered_search(q.copy(), 5, 64, allow=allow)
    assert ((f_ids >= 500) & (f_ids < 700)).all()
    with pytest.raises(ValueError):
        idx.filtered_search(q.copy(), 5, 64, allow=np.ones(500, bool))
