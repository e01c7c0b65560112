"""The candidate screen of the wide-row f32 L2 graph search (search kernel kMode 16, DESIGN.md
section 3): with ALAYA_SEARCH_SCREEN=1 the fresh candidates of an expansion are first measured on an
f16 copy of their rows, and those whose proven lower bound reaches the pool's worst distance never
read their f32 row.  Ids, distance bits and all four counters must stay those of the oracle, and
``screen_stats()`` (candidates screened, candidates screened out) shows the screen is running.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_EMPTY = 0xFFFFFFFF
_cache = {}


def _gist(n, nq, dim, centres=5):
    from workloads.datasets import gist_like

    return gist_like(n, nq, dim=dim, n_centres=centres)


def _graph_view(native, orc, base, valid=None, threads=8):
    g = native.Graph.build(base, 0, 32, 100, threads, 100)
    l0, levels, off, ue, ep, upper_r, _ = g.arrays()
    return g, orc.IndexView(base, l0, levels, off, ue, upper_r, ep, valid=valid)


def _dev(native, base, g, valid=None):
    d = native.DeviceIndex(0)
    d.set_base(base, 0, valid)
    d.set_graph(g)
    return d


def _check(view, dev, queries, k, ef):
    """tests/test_gpu.py::_check: ids, distance bits and the four counters against the oracle."""
    ids, dists, cnt = dev.search(queries, k, ef)
    for i, q in enumerate(queries):
        r_ids, r_d, r_c = view.search(q, k, ef, with_counters=True)
        assert np.array_equal(ids[i], r_ids), (i, ids[i], r_ids)
        assert np.array_equal(dists[i].view(np.uint32), r_d.view(np.uint32)), (i, dists[i], r_d)
        assert tuple(cnt[i]) == tuple(r_c), (i, cnt[i], r_c)
    return ids, dists, cnt


def _shape(native, orc, dim):
    """gist-shaped 5,000 x dim, 24 queries, graph, oracle view and device index: once per dimension."""
    if dim not in _cache:
        base, queries = _gist(5000, 24, dim)
        g, view = _graph_view(native, orc, base)
        _cache[dim] = (base, queries, g, view, _dev(native, base, g))
    return _cache[dim]


def _replay(orc, view, q, ef):
    """The reference's search of one query, restated in numpy on the oracle's distance: returns
    (pool ids, n_dist, n_expand, candidates evaluated in expansions that began with a full pool,
    those among them with exact d >= the pool's worst distance at the start of their expansion)."""
    base, l0 = view.base, view.l0
    u = int(view.s.ep)
    cur = orc.l2(q, base[u])
    up_r = int(view.s.upper_R)
    for level in range(int(view.levels[u]), 0, -1):
        changed = True
        while changed:
            changed = False
            off = int(view.upper_off[u]) + (level - 1) * up_r
            for v in view.upper_edges[off:off + up_r]:
                if v == K_EMPTY:
                    break
                d = orc.l2(q, base[v])
                if d < cur:
                    cur, nxt, changed = d, int(v), True
            if changed:
                u = nxt
    pool = [[cur, u, False]]  # sorted (dist, id, checked), capacity ef (LinearPool)
    visited = {u}
    pos = 0
    n_dist = n_expand = screened = rejectable = 0
    while pos < len(pool):
        pool[pos][2] = True
        node = pool[pos][1]
        while pos < len(pool) and pool[pos][2]:
            pos += 1
        n_expand += 1
        full = len(pool) == ef
        tau = pool[-1][0] if full else None
        for v in l0[node]:
            if v == K_EMPTY:
                break
            v = int(v)
            if v in visited:
                continue
            visited.add(v)
            d = orc.l2(q, base[v])
            n_dist += 1
            if full:
                screened += 1
                rejectable += 1 if d >= tau else 0
            if len(pool) == ef and d >= pool[-1][0]:
                continue
            at = len(pool)
            while at > 0 and pool[at - 1][0] > d:
                at -= 1
            pool.insert(at, [d, v, False])
            del pool[ef:]
            pos = min(pos, at)
    return [p[1] for p in pool], n_dist, n_expand, screened, rejectable


@pytest.mark.parametrize("ef", [32, 96])
@pytest.mark.parametrize("dim", [512, 768, 960, 1024])
def test_screen_parity_and_firing(native, orc, monkeypatch, dim, ef):
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "1")
    base, queries, g, view, dev = _shape(native, orc, dim)
    ids, _, cnt = _check(view, dev, queries, 10, ef)
    screened, out = dev.screen_stats()
    print(f"dim {dim} ef {ef}: screened {screened}, screened out {out}, n_dist {int(cnt[:, 0].sum())}")
    assert 0 < out <= screened <= int(cnt[:, 0].sum())
    if (dim, ef) == (960, 96):
        # how many candidates the screen may drop (exact d >= tau at the start of their expansion,
        # pool full), and that it drops nearly all of them
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
def test_screen_ties(native, orc, monkeypatch, ef):
    """Integer rows in {0, 1, 2} are exact in f16 (e_row is the absolute floor only) and tie on most
    distances, d == tau included: a tie is rejected by the reference and may be screened out, a
    candidate one step closer may not."""
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "1")
    rng = np.random.default_rng(512 + ef)
    base = rng.integers(0, 3, (3000, 512)).astype(np.float32)
    queries = rng.integers(0, 3, (24, 512)).astype(np.float32)
    queries[:4] = base[:4]
    g, view = _graph_view(native, orc, base)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, ef)
    assert dev.screen_stats()[1] > 0


def test_screen_pool_never_full(native, orc, monkeypatch):
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "1")
    base, queries = _gist(200, 8, 768, centres=2)
    g, view = _graph_view(native, orc, base, threads=1)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, 300)
    assert dev.screen_stats() == (0, 0)


def test_screen_invalid_rows(native, orc, monkeypatch):
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "1")
    base, queries, g, _, _ = _shape(native, orc, 768)
    valid = np.full(5000 // 8, 0xFF, np.uint8)
    valid[::5] = 0xA5  # half the rows of every fifth byte: 10 % invalid
    l0, levels, off, ue, ep, upper_r, _ = g.arrays()
    view = orc.IndexView(base, l0, levels, off, ue, upper_r, ep, valid=valid)
    dev = _dev(native, base, g, valid=valid)
    _check(view, dev, queries, 10, 96)
    assert dev.screen_stats()[1] > 0


def test_screen_unrepresentable_rows(native, orc, monkeypatch):
    """Rows x 1e5 overflow f16 (e_row = +inf: never screened out), rows x 1e-6 lose most of their
    bits to f16 subnormals (a large e_row relative to the row)."""
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "1")
    base, queries = _gist(3000, 16, 512, centres=3)
    base = base.copy()
    base[::7] *= np.float32(1e5)
    base[::7, 5] = np.float32(1e5)  # (whatever the row held there)
    base[3::11] *= np.float32(1e-6)
    g, view = _graph_view(native, orc, base)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, 64)
    assert dev.screen_stats()[1] > 0
    # every row out of range: all are screened, none may be dropped
    big = (_gist(2000, 8, 512, centres=2)[0] * np.float32(1e5)).astype(np.float32)
    big[:, 9] = np.float32(7e4)
    qs = big[:8] * np.float32(1.01)
    g, view = _graph_view(native, orc, big)
    dev = _dev(native, big, g)
    _check(view, dev, qs, 10, 48)
    screened, out = dev.screen_stats()
    assert screened > 0 and out == 0


@pytest.mark.parametrize("dim", [768, 960])
def test_screen_two_waves(native, orc, monkeypatch, dim):
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "1")
    monkeypatch.setenv("ALAYA_TWO_WAVES", "1")
    _, queries, _, view, dev = _shape(native, orc, dim)
    _check(view, dev, queries, 10, 96)
    assert dev.screen_stats()[1] > 0


def test_screen_follows_set_base(native, orc, monkeypatch):
    """set_base twice on one index, another n and dim each time: the copy is rebuilt for the new base."""
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "1")
    dev = native.DeviceIndex(0)
    for n, dim in [(3000, 512), (1500, 1024), (3000, 512)]:
        base, queries = _gist(n, 12, dim, centres=3)
        base = (base * np.float32(1 + dim / 512)).astype(np.float32)
        g, view = _graph_view(native, orc, base)
        dev.set_base(base, 0, None)
        dev.set_graph(g)
        _check(view, dev, queries, 10, 64)
        assert dev.screen_stats()[1] > 0


def test_screen_follows_updates(native, orc, monkeypatch):
    """Online insert / remove (the tests/test_updates.py sequence at d = 512): the copy follows the
    written rows."""
    import alayalite_amd

    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "1")
    rng = np.random.default_rng(61)
    n0, d = 600, 512
    base = _gist(n0 + 200, 1, d, centres=2)[0]
    idx = alayalite_amd.Client().create_index("upd_screen", metric="l2", capacity=n0 + 150)
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


def test_screen_off_switch(native, orc, monkeypatch):
    _, queries, _, view, dev = _shape(native, orc, 960)
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "1")
    on = dev.search(queries, 10, 96)
    assert dev.screen_stats()[1] > 0
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "0")
    off = _check(view, dev, queries, 10, 96)
    assert dev.screen_stats() == (0, 0)
    for a, b in zip(on, off):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
