"""The scout of the screened graph search (``ALAYA_SEARCH_SCOUT``, DESIGN.md section 3, "Round 11"):
in a batch that leaves the second wave per SIMD idle, every searcher of the d = 768 / 960 integer
screen gets a scout wave in its workgroup, which computes the screen's bounds for the neighbours of the
nodes the searcher will probably pop next; the searcher takes them from an LDS memo at the pop and
skips its screen pass, or runs the pass as before when they are not there.  A bound is a function of
the query and one row's record, so ids, distance bits, all four counters and ``screen_stats()`` must be
those of the search without scouts.  ``scout_stats()`` = (expansions that screened, those that took
the scout's bounds, records the scouts read, bounds the verify mode found different).  The shapes,
helpers and cached indexes are those of ``test_search_screen.py``.
"""

import numpy as np
import pytest

from test_search_screen import _check, _dev, _gist, _graph_view, _shape

pytestmark = pytest.mark.gpu

BOARD_BYTES = 440  # search_kernels.h kScoutBoardBytes: the memo and the requests of one searcher
_runs = {}


@pytest.fixture(autouse=True)
def _int_screen(monkeypatch):
    monkeypatch.setenv("ALAYA_SEARCH_SCREEN", "9")
    monkeypatch.delenv("ALAYA_SEARCH_SCOUT_MISS", raising=False)
    monkeypatch.delenv("ALAYA_SEARCH_SCOUT_GRID", raising=False)


def _bits(out):
    return [np.asarray(a).view(np.uint32) for a in out]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _scout_run(native, orc, monkeypatch, dim, ef, scout):
    """One oracle-checked search of the cached shape per (dim, ef, scout): results, both stats, plan."""
    key = (dim, ef, scout)
    if key not in _runs:
        monkeypatch.setenv("ALAYA_SEARCH_SCOUT", str(scout))
        _, queries, _, view, dev = _shape(native, orc, dim)
        out = _check(view, dev, queries, 10, ef)
        _runs[key] = (out, dev.screen_stats(), dev.scout_stats(), dev.last_launch(), dev.last_plan())
    return _runs[key]


@pytest.mark.parametrize("ef", [32, 96])
@pytest.mark.parametrize("dim", [768, 960])
def test_scout_parity_and_firing(native, orc, monkeypatch, dim, ef):
    off, off_screen, off_scout, _, _ = _scout_run(native, orc, monkeypatch, dim, ef, 0)
    on, on_screen, (expansions, hits, records, bad), _, plan = _scout_run(native, orc, monkeypatch, dim, ef, 1)
    print(f"dim {dim} ef {ef}: screened expansions {expansions}, memo hits {hits}, scout records {records}, "
          f"screen {on_screen}")
    assert plan["scout"] == 1 and off_scout == (0, 0, 0, 0)
    assert on_screen == off_screen and on_screen[1] > 0
    assert _same(on, off)
    assert 0 < hits <= expansions and records > 0 and bad == 0


@pytest.mark.parametrize("ef", [32, 96])
@pytest.mark.parametrize("dim", [768, 960])
def test_scout_verify(native, orc, monkeypatch, dim, ef):
    on = _scout_run(native, orc, monkeypatch, dim, ef, 1)[0]
    ver, _, (expansions, hits, _, bad), _, plan = _scout_run(native, orc, monkeypatch, dim, ef, 2)
    assert plan["scout"] == 3
    assert bad == 0 and 0 < hits <= expansions
    assert _same(ver, on)


@pytest.mark.parametrize("dim", [768, 960])
def test_scout_fallback_only(native, orc, monkeypatch, dim):
    """No answer ever matches: every expansion runs its own pass, and the scouts' work changes nothing."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "2")
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT_MISS", "1")
    _, queries, _, view, dev = _shape(native, orc, dim)
    _check(view, dev, queries, 10, 96)
    expansions, hits, records, bad = dev.scout_stats()
    print(f"dim {dim}: screened expansions {expansions}, memo hits {hits}, scout records {records}")
    assert dev.last_plan()["scout"] == 7
    assert hits <= 4 and expansions > 0 and records > 0 and bad == 0
    assert dev.screen_stats() == _scout_run(native, orc, monkeypatch, dim, 96, 0)[1]


@pytest.mark.parametrize("nq, grid", [(24, 0), (7, 0), (24, 3)])
def test_scout_persistent_loop(native, orc, monkeypatch, nq, grid):
    """Queries alternate between a vector at the data's scale and one far outside it (x 50): a bound kept
    from a searcher's previous query would drop candidates the other query accepts.  One round (a
    searcher per query, more and fewer queries than it takes to matter), and -- with the grid held to 3
    workgroups -- eight queries through every searcher and its scout, one after the other."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "2")
    if grid:
        monkeypatch.setenv("ALAYA_SEARCH_SCOUT_GRID", str(grid))
    _, queries, _, view, dev = _shape(native, orc, 960)
    qs = queries[:nq].copy()
    qs[1::2] *= np.float32(50)
    _check(view, dev, qs, 10, 64)
    expansions, hits, _, bad = dev.scout_stats()
    groups, waves = dev.last_launch()
    assert (groups, waves) == (grid or nq, 2)
    assert bad == 0 and 0 < hits <= expansions


def test_scout_needs_one_round(native, orc, monkeypatch):
    """More queries than resident searcher-plus-scout workgroups: today's plan, no scouts."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "1")
    _, queries, _, view, dev = _shape(native, orc, 960)
    _check(view, dev, queries, 10, 32)
    per_cu = dev.last_plan()["groups_per_cu"]
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nq = per_cu * cus + 1
    big = np.tile(queries, (nq // len(queries) + 1, 1))[:nq]
    ids, dists, cnt = dev.search(big, 10, 32)
    plan = dev.last_plan()
    assert plan["scout"] == 0 and dev.scout_stats() == (0, 0, 0, 0)
    small = dev.search(queries, 10, 32)
    n = len(queries)
    assert _same((ids[:n], dists[:n], cnt[:n]), small)


@pytest.mark.parametrize("dim", [768, 960])
def test_scout_ties(native, orc, monkeypatch, dim):
    """test_int_screen_ties' rows at the scout's widths: integers in {0, 1, 2}, ties at d == tau."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "2")
    rng = np.random.default_rng(dim + 64)
    base = rng.integers(0, 3, (3000, dim)).astype(np.float32)
    queries = rng.integers(0, 3, (24, dim)).astype(np.float32)
    queries[:4] = base[:4]
    g, view = _graph_view(native, orc, base)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, 64)
    expansions, hits, _, bad = dev.scout_stats()
    assert dev.screen_stats()[1] > 0 and bad == 0 and 0 < hits <= expansions


def test_scout_invalid_rows(native, orc, monkeypatch):
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "2")
    base, queries, g, _, _ = _shape(native, orc, 768)
    valid = np.full(5000 // 8, 0xFF, np.uint8)
    valid[::5] = 0xA5  # half the rows of every fifth byte: 10 % invalid
    l0, levels, off, ue, ep, upper_r, _ = g.arrays()
    view = orc.IndexView(base, l0, levels, off, ue, upper_r, ep, valid=valid)
    dev = _dev(native, base, g, valid=valid)
    _check(view, dev, queries, 10, 96)
    expansions, hits, _, bad = dev.scout_stats()
    assert dev.screen_stats()[1] > 0 and bad == 0 and 0 < hits <= expansions


def test_scout_pool_never_full(native, orc, monkeypatch):
    """Nothing is ever screened, so nothing is ever requested: the scouts leave with their searchers."""
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "2")
    base, queries = _gist(200, 8, 768, centres=2)
    g, view = _graph_view(native, orc, base, threads=1)
    dev = _dev(native, base, g)
    _check(view, dev, queries, 10, 300)
    assert dev.last_plan()["scout"] == 3
    assert dev.screen_stats() == (0, 0)
    assert dev.scout_stats() == (0, 0, 0, 0)


@pytest.mark.parametrize("dim", [768, 960])
def test_scout_plan(native, orc, monkeypatch, dim):
    """Two waves per searcher, and nothing else moves: the searcher's LDS (the workgroup's less the
    board), its visited table and the searchers per CU are the scout-off plan's."""
    off_launch, off_plan = _scout_run(native, orc, monkeypatch, dim, 96, 0)[3:]
    on_launch, on_plan = _scout_run(native, orc, monkeypatch, dim, 96, 1)[3:]
    assert off_launch[1] == 1 and off_plan["scout"] == 0
    assert on_launch == (off_launch[0], 2) and on_plan["scout"] == 1
    assert on_plan["lds_bytes"] - BOARD_BYTES == off_plan["lds_bytes"]
    for key in ("hash_log2", "compact", "groups_per_cu", "workgroups"):
        assert on_plan[key] == off_plan[key], key


def test_scout_absent_with_stamps_helpers_or_ip(native, orc, monkeypatch):
    monkeypatch.setenv("ALAYA_SEARCH_SCOUT", "1")
    base, queries, g, view, dev = _shape(native, orc, 960)
    ref = _scout_run(native, orc, monkeypatch, 960, 96, 0)[0]
    # stamps: the stamped kernel has neither the screen nor the scout
    ids, cnt, _ = dev.profile_search(queries, 10, 96, 0)
    assert dev.last_plan()["scout"] == 0 and dev.last_launch()[1] == 1
    assert np.array_equal(ids, ref[0]) and np.array_equal(cnt, ref[2])
    # helpers wanted
    monkeypatch.setenv("ALAYA_HELPERS", "1")
    out = _check(view, dev, queries, 10, 96)
    assert dev.last_plan()["scout"] == 0 and dev.scout_stats() == (0, 0, 0, 0)
    assert _same(out, ref)
    monkeypatch.delenv("ALAYA_HELPERS")
    # inner product: no screen, so no scout
    ip = native.DeviceIndex(0)
    ip.set_base(base, orc.IP, None)
    ip.set_graph(g)
    l0, levels, off, ue, ep, upper_r, _ = g.arrays()
    ip_view = orc.IndexView(base, l0, levels, off, ue, upper_r, ep, metric=orc.IP)
    _check(ip_view, ip, queries, 10, 96)
    assert ip.last_plan()["scout"] == 0 and ip.scout_stats() == (0, 0, 0, 0)
