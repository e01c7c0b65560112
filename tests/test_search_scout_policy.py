"""The scout's policy bits (``ALAYA_SEARCH_SCOUT_POLICY``, DESIGN.md section 3, "Round 12"): 1 = the
searcher requests the likely next pop right after the screen, 2 = the scout looks at the requests
again once a node's adjacency row has arrived and drops a node that is in neither.  Both are hints:
ids, distance bits, all four counters and ``screen_stats()`` must be those of the search without
scouts at every policy, and the verify mode (``ALAYA_SEARCH_SCOUT=2``) must find no bound different.
``scout_policy_stats()`` = (early requests, those the merge confirmed, nodes dropped at the second
look).  Bit 2 (4 = the scout warms the f32 rows of the neighbours that pass the screen) measured
slower at both widths and left the code with its counter and its row-bounds test; the variable's
values 4 .. 7 stay among the cases and must run as 0 .. 3.  The shapes, helpers and cached indexes
are those of ``test_search_screen.py``, the inputs those of ``test_search_scout.py``.
"""

import numpy as np
import pytest

from test_search_screen import _check, _dev, _gist, _graph_view, _shape

pytestmark = pytest.mark.gpu

_off = {}


@pytest.fixture(autouse=True)
def _verify_mode(monkeypatch):
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "9")
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "2")
    monkeypatch.delenv("ALAYA_SEARCH_SCOUT_MISS", raising=False)
    monkeypatch.delenv("ALAYA_SEARCH_SCOUT_GRID", raising=False)
    monkeypatch.delenv("ALAYA_SEARCH_SCOUT_POLICY", raising=False)


def _bits(out):
    return [np.asarray(a).view(np.uint32) for a in out]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _scout_off(native, orc, monkeypatch, dim, ef):
    """The oracle-checked search of the cached shape without scouts, once per (dim, ef)."""
    if (dim, ef) not in _off:
        monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "0")
        _, queries, _, view, dev = _shape(native, orc, dim)
        out = _check(view, dev, queries, 10, ef)
        assert dev.last_plan()["scout"] == 0 and dev.scout_policy_stats() == (0, 0, 0)
        _off[(dim, ef)] = (out, dev.screen_stats())
        monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "2")
    return _off[(dim, ef)]


def _fired(policy, stats):
    """Each counter is > 0 exactly when its bit is set; the second look may find nothing to drop."""
    posts, confirmed, abandoned = stats
    assert (posts > 0) == bool(policy & 1), (policy, stats)
    assert confirmed <= posts and (confirmed > 0) == bool(policy & 1), (policy, stats)
    assert abandoned == 0 or policy & 2, (policy, stats)


@pytest.mark.parametrize("ef", [32, 96])
@pytest.mark.parametrize("dim", [768, 960])
@pytest.mark.parametrize("policy", range(8))
def test_policy_parity_and_firing(native, orc, monkeypatch, policy, dim, ef):
    off, off_screen = _scout_off(native, orc, monkeypatch, dim, ef)
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT_POLICY", str(policy))
    _, queries, _, view, dev = _shape(native, orc, dim)
    out = _check(view, dev, queries, 10, ef)
    plan = dev.last_plan()
    expansions, hits, records, bad = dev.scout_stats()
    stats = dev.scout_policy_stats()
    print(f"policy {policy} dim {dim} ef {ef}: screened expansions {expansions}, memo hits {hits}, scout records "
          f"{records}, early / confirmed / abandoned {stats}")
    assert plan["scout"] == 3 and plan["scout_policy"] == policy & 3
    assert _same(out, off) and dev.screen_stats() == off_screen
    assert bad == 0 and 0 < hits <= expansions
    _fired(policy & 3, stats)


@pytest.mark.parametrize("nq, grid", [(24, 0), (7, 0), (24, 3)])
def test_policy_persistent_loop(native, orc, monkeypatch, nq, grid):
    """test_scout_persistent_loop's queries, alternating between the data's scale and 50 times it: a
    request or a second look that outlives its query must change nothing in the next."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT_POLICY", "7")
    if grid:
        monkeypatch.setenv("ALAYA_SEARCH_SCOUT_GRID", str(grid))
    _, queries, _, view, dev = _shape(native, orc, 960)
    qs = queries[:nq].copy()
    qs[1::2] *= np.float32(50)
    _check(view, dev, qs, 10, 64)
    expansions, hits, _, bad = dev.scout_stats()
    assert dev.last_launch() == (grid or nq, 2) and dev.last_plan()["scout_policy"] == 3
    assert bad == 0 and 0 < hits <= expansions
    _fired(3, dev.scout_policy_stats())


@pytest.mark.parametrize("dim", [768, 960])
def test_policy_ties(native, orc, monkeypatch, dim):
    """test_scout_ties' rows: integers in {0, 1, 2}, bounds and distances that tie at tau and at the
    first unchecked entry's distance."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT_POLICY", "7")
    rng = np.random.default_rng(dim + 64)
    base = rng.integers(0, 3, (3000, dim)).astype(np.float32)
    queries = rng.integers(0, 3, (24, dim)).astype(np.float32)
    queries[:4] = base[:4]
    g, view = _graph_view(native, orc, base)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, 64)
    expansions, hits, _, bad = dev.scout_stats()
    posts, confirmed, _ = dev.scout_policy_stats()
    assert dev.screen_stats()[1] > 0 and bad == 0 and 0 < hits <= expansions
    assert dev.last_plan()["scout_policy"] == 3 and confirmed <= posts


def test_policy_invalid_rows(native, orc, monkeypatch):
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT_POLICY", "7")
    base, queries, g, _, _ = _shape(native, orc, 768)
    valid = np.full(5000 // 8, 0xFF, np.uint8)
    valid[::5] = 0xA5  # half the rows of every fifth byte: 10 % invalid
    l0, levels, off, ue, ep, upper_r, _ = g.arrays()
    view = orc.IndexView(base, l0, levels, off, ue, upper_r, ep, valid=valid)
    dev = _dev(native, base, g, valid=valid)
    _check(view, dev, queries, 10, 96)
    expansions, hits, _, bad = dev.scout_stats()
    posts, confirmed, _ = dev.scout_policy_stats()
    assert dev.screen_stats()[1] > 0 and bad == 0 and 0 < hits <= expansions
    assert dev.last_plan()["scout_policy"] == 3 and confirmed <= posts


@pytest.mark.parametrize("dim", [768, 960])
def test_policy_fallback_only(native, orc, monkeypatch, dim):
    """No answer ever matches: the early requests and the second look run, and change nothing."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT_POLICY", "7")
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT_MISS", "1")
    off, off_screen = _scout_off(native, orc, monkeypatch, dim, 96)
    _, queries, _, view, dev = _shape(native, orc, dim)
    out = _check(view, dev, queries, 10, 96)
    expansions, hits, records, bad = dev.scout_stats()
    assert dev.last_plan()["scout"] == 7 and dev.last_plan()["scout_policy"] == 3
    assert hits <= 4 and expansions > 0 and records > 0 and bad == 0
    assert _same(out, off) and dev.screen_stats() == off_screen


def test_policy_pool_never_full(native, orc, monkeypatch):
    """Nothing is ever screened, so nothing is requested early or late, and nothing dropped."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT_POLICY", "7")
    base, queries = _gist(200, 8, 768, centres=2)
    g, view = _graph_view(native, orc, base, threads=1)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, 300)
    assert dev.last_plan()["scout"] == 3 and dev.last_plan()["scout_policy"] == 3
    assert dev.screen_stats() == (0, 0) and dev.scout_stats() == (0, 0, 0, 0)
    assert dev.scout_policy_stats() == (0, 0, 0)


def test_policy_absent_without_scouts(native, orc, monkeypatch):
    """Inner product, stamps, helpers, more queries than one round: no scouts, so no policy, whatever
    the variable says."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT_POLICY", "7")
    base, queries, g, view, dev = _shape(native, orc, 960)
    ref = _scout_off(native, orc, monkeypatch, 960, 96)[0]

    def absent(d):
        plan = d.last_plan()
        assert plan["scout"] == 0 and plan["scout_policy"] == 0
        assert d.scout_policy_stats() == (0, 0, 0)

    ids, cnt, _ = dev.profile_search(queries, 10, 96, 0)  # stamps
    absent(dev)
    assert np.array_equal(ids, ref[0]) and np.array_equal(cnt, ref[2])
    monkeypatch.setenv("ALAYA_HELPERS", "1")
    out = _check(view, dev, queries, 10, 96)
    absent(dev)
    assert _same(out, ref)
    monkeypatch.delenv("ALAYA_HELPERS")
    # more queries than resident searcher-plus-scout workgroups
    import torch

    _check(view, dev, queries, 10, 32)
    assert dev.last_plan()["scout_policy"] == 3
    nq = dev.last_plan()["groups_per_cu"] * torch.cuda.get_device_properties(0).multi_processor_count + 1
    big = np.tile(queries, (nq // len(queries) + 1, 1))[:nq]
    ids, dists, cnt = dev.search(big, 10, 32)
    absent(dev)
    n = len(queries)
    assert _same((ids[:n], dists[:n], cnt[:n]), dev.search(queries, 10, 32))
    # inner product: no screen, so no scout
    ip = native.DeviceIndex(0)
    ip.set_base(base, orc.IP, None)
    ip.set_graph(g)
    l0, levels, off, ue, ep, upper_r, _ = g.arrays()
    ip_view = orc.IndexView(base, l0, levels, off, ue, upper_r, ep, metric=orc.IP)
    _check(ip_view, ip, queries, 10, 96)
    absent(ip)
