"""The candidate screen under integer dot products (``ALAYA_SEARCH_SCREEN=9``, DESIGN.md section 3,
"Round 10"): the kernels and the 8-bit records of ``test_search_screen_u8.py``, but the query is
quantised too and a candidate costs one ``v_dot4_u32_u8`` sum of the two code vectors; the record's
code sums C1, C2 (in its padding) and the query's turn it into the bound.  Ids, distance bits and all
four counters must stay those of the oracle whatever the copy holds, and ``screen_stats()`` shows the
screen is running.  The shapes, helpers and cached indexes are those of ``test_search_screen.py``.
"""

import numpy as np
import pytest

from test_search_screen import _check, _dev, _gist, _graph_view, _replay, _shape

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _int(monkeypatch):
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "9")


@pytest.mark.parametrize("ef", [32, 96])
@pytest.mark.parametrize("dim", [512, 768, 960, 1024])
def test_int_screen_parity_and_firing(native, orc, dim, ef):
    base, queries, g, view, dev = _shape(native, orc, dim)
    ids, _, cnt = _check(view, dev, queries, 10, ef)
    screened, out = dev.screen_stats()
    print(f"dim {dim} ef {ef}: screened {screened}, screened out {out}, n_dist {int(cnt[:, 0].sum())}")
    assert 0 < out <= screened <= int(cnt[:, 0].sum())
    if (dim, ef) == (960, 96):
        # how many candidates the screen may drop (exact d >= tau at the start of their expansion,
        # pool full), and that two 8-bit grids still drop nearly all of them
        tot_screened = tot_rejectable = 0
        for i, q in enumerate(queries):
            p_ids, n_dist, n_expand, s, r = _replay(orc, view, q, ef)
            assert p_ids[:10] == ids[i].tolist() and (n_dist, n_expand) == (cnt[i, 0], cnt[i, 1])
            tot_screened += s
            tot_rejectable += r
        print(f"replay: screened {tot_screened}, rejectable {tot_rejectable}, device out / rejectable "
              f"{out / tot_rejectable:.4f}")
        assert screened == tot_screened
        assert out <= tot_rejectable
        assert out >= 0.9 * tot_rejectable


@pytest.mark.parametrize("ef", [64, 200])
def test_int_screen_ties(native, orc, ef):
    """Integer rows in {0, 1, 2} tie on most distances, d == tau included: a tie is rejected by the
    reference and may be screened out, a candidate one step closer may not."""
    rng = np.random.default_rng(512 + ef)
    base = rng.integers(0, 3, (3000, 512)).astype(np.float32)
    queries = rng.integers(0, 3, (24, 512)).astype(np.float32)
    queries[:4] = base[:4]
    g, view = _graph_view(native, orc, base)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, ef)
    assert dev.screen_stats()[1] > 0


def test_int_screen_pool_never_full(native, orc):
    base, queries = _gist(200, 8, 768, centres=2)
    g, view = _graph_view(native, orc, base, threads=1)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, 300)
    assert dev.screen_stats() == (0, 0)


def test_int_screen_invalid_rows(native, orc):
    base, queries, g, _, _ = _shape(native, orc, 768)
    valid = np.full(5000 // 8, 0xFF, np.uint8)
    valid[::5] = 0xA5  # half the rows of every fifth byte: 10 % invalid
    l0, levels, off, ue, ep, upper_r, _ = g.arrays()
    view = orc.IndexView(base, l0, levels, off, ue, upper_r, ep, valid=valid)
    dev = _dev(native, base, g, valid=valid)
    _check(view, dev, queries, 10, 96)
    assert dev.screen_stats()[1] > 0


def test_int_screen_scaled_and_infinite_rows(native, orc):
    """Rows x 1e5 and x 1e-6 among ordinary ones (each record carries its row's own grid; nothing is
    asserted about how many are dropped), then rows holding inf (e_row = +inf: never screened out), and a
    query holding inf (e_q = +inf: nothing is screened out for it)."""
    base, queries = _gist(3000, 16, 512, centres=3)
    base = base.copy()
    base[::7] *= np.float32(1e5)
    base[::7, 5] = np.float32(1e5)
    base[3::11] *= np.float32(1e-6)
    g, view = _graph_view(native, orc, base)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, 64)
    assert dev.screen_stats()[0] > 0
    bad_q = queries[:4].copy()
    bad_q[:, 3] = np.float32(np.inf)
    _check(view, dev, bad_q, 10, 64)
    assert dev.screen_stats()[1] == 0
    # the same graph over rows of which some hold inf: their distance is inf for every query
    with_inf = base.copy()
    with_inf[5::13, 17] = np.float32(np.inf)
    l0, levels, off, ue, ep, upper_r, _ = g.arrays()
    view = orc.IndexView(with_inf, l0, levels, off, ue, upper_r, ep)
    dev = _dev(native, with_inf, g)
    _check(view, dev, queries, 10, 64)
    assert dev.screen_stats()[0] > 0


@pytest.mark.parametrize("dim", [768, 960])
def test_int_screen_two_waves(native, orc, monkeypatch, dim):
    monkeypatch.setenv("ALAYA_TWO_WAVES", "1")
    _, queries, _, view, dev = _shape(native, orc, dim)
    _check(view, dev, queries, 10, 96)
    assert dev.screen_stats()[1] > 0


def test_int_screen_follows_set_base(native, orc):
    """set_base three times on one index, another n and dim each time: the records are rebuilt for the new base."""
    dev = native.DeviceIndex(0)
    for n, dim in [(3000, 512), (1500, 1024), (3000, 512)]:
        base, queries = _gist(n, 12, dim, centres=3)
        base = (base * np.float32(1 + dim / 512)).astype(np.float32)
        g, view = _graph_view(native, orc, base)
        dev.set_base(base, 0, None)
        dev.set_graph(g)
        _check(view, dev, queries, 10, 64)
        assert dev.screen_stats()[1] > 0


def test_int_screen_follows_updates(native, orc):
    """Online insert / remove (the tests/test_updates.py sequence at d = 512): the patched records carry
    the written rows' codes and code sums -- a stale C1 / C2 gives a wrong bound, and a wrong bound that
    drops a candidate the reference accepts changes ids or distances."""
    import alayalite_amd

    rng = np.random.default_rng(61)
    n0, d = 600, 512
    base = _gist(n0 + 200, 1, d, centres=2)[0]
    idx = alayalite_amd.Client().create_index("upd_screen_int", metric="l2", capacity=n0 + 150)
    fit_rows = base[:n0].copy()
    idx.fit(fit_rows, ef_construction=100, num_threads=1)
    inner = idx._Index__index
    l0, levels, off, ue, ep, ur, _ = inner.graph_arrays()
    up = orc.Updater(orc.IndexView(fit_rows, l0, levels, off, ue, ur, ep), n0 + 150)
    idx.batch_search(base[:4].copy(), 10, 64)  # the copy exists before the first write
    assert inner.screen_stats()[0] > 0
    for i in range(n0, n0 + 120):
        assert idx.insert(base[i].copy(), 48) == up.insert(base[i], base[i], 48)
        if i % 7 == 0:
            r = int(rng.integers(0, i))
            up.remove(r)
            idx.remove(r)
    assert np.array_equal(inner.graph_arrays()[0], up.l0())
    qs = np.concatenate([base[n0 + 100:n0 + 110], base[n0 + 150:n0 + 160]])
    out = 0
    for q in qs:
        ids, dists = idx.batch_search_with_distance(q.reshape(1, -1).copy(), 10, 64)
        o_ids, o_d = up.search(q, 10, 64)
        assert np.array_equal(ids[0].astype(np.uint32), o_ids)
        assert np.array_equal(dists[0].view(np.uint32), o_d.view(np.uint32))
        out += inner.screen_stats()[1]
    assert out > 0


def test_int_screen_format_switch(native, orc, monkeypatch):
    """9 -> 8 -> 1 -> 0 on one index: the two record passes share one copy, the f16 copy lives beside it,
    and every launch gives the same bits."""
    _, queries, _, view, dev = _shape(native, orc, 960)
    runs = []
    for fmt in ["9", "8", "1"]:
        monkeypatch.setenv("ALAYA_SEARCH_SCREEN", fmt)
        runs.append(dev.search(queries, 10, 96))
        assert dev.screen_stats()[1] > 0
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "0")
    off = _check(view, dev, queries, 10, 96)
    assert dev.screen_stats() == (0, 0)
    for run in runs:
        for a, c in zip(run, off):
            assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(c).view(np.uint32))
