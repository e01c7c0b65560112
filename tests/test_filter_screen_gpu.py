"""The filtered graph search under the integer candidate screen (filtered_screen_search_kernel) against the
filtered search's restatement (tests/filter_common.py): ids, distance bits and the four counters of every
query, and the launch's screen counts.  2000 rows, at most 12 queries a case (128 in the persistent one).

A candidate is dropped before its f32 row is read iff its proven lower bound lb is positive, reaches the
traversal pool's worst distance and -- if the row is allowed and valid -- the full result pool's; nothing is
dropped before the traversal pool is full.  The restatement screens nothing, so parity is the proof's test."""

import numpy as np
import pytest

import degree_common as dc
import filter_common as fc

pytestmark = pytest.mark.gpu

_devices = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("ALAYA_FILTER_GRID", "ALAYA_FILTER_SCREEN", "ALAYA_SEARCH_SCREEN", "ALAYA_SEARCH_WAVES",
                 "ALAYA_VIS_LIMIT", "ALAYA_VIS_LIMIT_PCT"):
        monkeypatch.delenv(name, raising=False)


def _words(allow):
    from alayalite_amd.utils import pack_allow

    return pack_allow(allow, fc.N)


def _device(native, orc, dim, kind="gist"):
    if (dim, kind) not in _devices:
        base, _, arrays = fc.graph(orc, dim, 0, kind)
        _devices[dim, kind] = dc.device_of(native, base, arrays)
    return _devices[dim, kind]


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("k,ef,share", [(10, 40, 0.1), (10, 40, 0.02), (65, 10, 0.5), (1, 40, 1.0)])
@pytest.mark.parametrize("dim", [512, 768, 960, 1024])
def test_parity_and_firing(native, orc, dim, k, ef, share):
    """Fails without the screen: the stats after a filtered launch are then (0, 0)."""
    _, queries, _ = fc.graph(orc, dim, 0)
    dev = _device(native, orc, dim)
    got = dev.filtered_search(queries, k, ef, _words(fc.mask(fc.N, share)))
    want = fc.replays(orc, dim, 0, "gist", k, ef, share)
    fc.assert_matches(got, want, (dim, k, ef, share))
    screened, out = dev.screen_stats()
    assert 0 < out <= screened <= sum(r["counters"][0] for r in want), (screened, out)


def test_result_pool_never_full(native, orc):
    """k = 224 at ef = 4, every row allowed: no query offers 224 rows (checked on the restatement), so the
    result pool never fills and nothing may be dropped.  (ef = 4, not 10: at ef 10, 8, 6 and 5 some query of
    these inputs offers 306, 265, 251 and 232 rows; at ef 4 the most is 220.)"""
    _, queries, _ = fc.graph(orc, 960, 0)
    want = fc.replays(orc, 960, 0, "gist", 224, 4, 1.0)
    assert max(len(r["pairs"]) for r in want) < 224
    dev = _device(native, orc, 960)
    fc.assert_matches(dev.filtered_search(queries, 224, 4, _words(fc.mask(fc.N, 1.0))), want, "never full")
    screened, out = dev.screen_stats()
    assert screened > 0 and out == 0


def test_ties(native, orc):
    """Rows of {0, 1, 2}: bounds and distances tie at both pools' worst distances."""
    _, queries, _ = fc.graph(orc, 512, 0, "tie")
    dev = _device(native, orc, 512, "tie")
    got = dev.filtered_search(queries, 10, 20, _words(fc.mask(fc.N, 0.3)))
    fc.assert_matches(got, fc.replays(orc, 512, 0, "tie", 10, 20, 0.3), "tie")
    assert dev.screen_stats()[0] > 0


def test_validity_bitmap(native, orc):
    base, queries, arrays = fc.graph(orc, 768, 0)
    valid = np.full(fc.N // 8, 0xFF, np.uint8)
    valid[::5] = 0xA5  # half the rows of every fifth byte: 10 % invalid
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0, valid)
    dev.set_graph(dc.graph_of(native, arrays))
    allow = fc.mask(fc.N, 0.5)
    view = dc.view_of(orc, base, arrays, valid=valid)
    want = fc.replays(orc, 768, 0, "invalid", 10, 40, 0.5, view=view, queries=queries, allow=allow)
    fc.assert_matches(dev.filtered_search(queries, 10, 40, _words(allow)), want, "invalid rows")
    assert dev.screen_stats()[1] > 0


def test_three_masks_and_persistent_waves(native, orc, monkeypatch):
    """Masks of three shares in one batch; then two workgroups run 128 queries, so each wave runs dozens of
    queries on one result pool and one set of query-code registers."""
    base, queries, arrays = fc.graph(orc, 960, 0)
    dev = _device(native, orc, 960)
    shares = (0.1, 0.5, 0.02)
    masks = np.stack([fc.mask(fc.N, s) for s in shares])
    groups = np.arange(len(queries)) % 3
    got = dev.filtered_search(queries, 10, 40, _words(masks), groups.astype(np.uint32))
    fc.assert_matches(got, [fc.replays(orc, 960, 0, "gist", 10, 40, shares[g])[i] for i, g in enumerate(groups)], "three masks")
    assert dev.screen_stats()[1] > 0
    monkeypatch.setenv("ALAYA_FILTER_GRID", "2")
    many = base[:128]
    groups = np.arange(len(many)) % 3
    got = dev.filtered_search(many, 10, 40, _words(masks), groups.astype(np.uint32))
    assert dev.last_launch()[0] == 2
    view = dc.view_of(orc, base, arrays)
    want = [fc.replay(orc, view, q, 10, 40, masks[g]) for q, g in zip(many, groups)]
    fc.assert_matches(got, want, "grid 2")
    assert dev.screen_stats()[1] > 0


def test_non_finite_query(native, orc):
    """e_q = +inf: no bound, so nothing is dropped for such a query."""
    base, queries, arrays = fc.graph(orc, 960, 0)
    bad = queries[:4].copy()
    bad[:, 3] = np.float32(np.inf)
    allow = fc.mask(fc.N, 0.1)
    dev = _device(native, orc, 960)
    want = fc.replays(orc, 960, 0, "inf", 10, 40, 0.1, view=dc.view_of(orc, base, arrays), queries=bad, allow=allow)
    fc.assert_matches(dev.filtered_search(bad, 10, 40, _words(allow)), want, "inf query")
    assert dev.screen_stats()[1] == 0


@pytest.mark.parametrize("name,value", [("ALAYA_FILTER_SCREEN", "0"), ("ALAYA_SEARCH_SCREEN", "0"), ("ALAYA_SEARCH_SCREEN", "1")])
def test_switches(native, orc, monkeypatch, name, value):
    """Each setting runs the unscreened kernel: equal ids, distance bits and counters, stats (0, 0)."""
    _, queries, _ = fc.graph(orc, 960, 0)
    dev = _device(native, orc, 960)
    words = _words(fc.mask(fc.N, 0.1))
    default = dev.filtered_search(queries, 10, 40, words)
    assert dev.screen_stats()[1] > 0
    monkeypatch.setenv(name, value)
    assert _same(dev.filtered_search(queries, 10, 40, words), default)
    assert tuple(dev.screen_stats()) == (0, 0)


def test_public_interface(native, orc, monkeypatch):
    import alayalite_amd

    base, queries = dc.rows(960)
    idx = alayalite_amd.Client().create_index("filter_screen", capacity=fc.N)
    idx.fit(base.copy(), ef_construction=100, num_threads=1)
    allow = fc.mask(fc.N, 0.1)
    got = idx.filtered_search(queries.copy(), 10, 40, allow=allow)
    assert idx.native().screen_stats()[1] > 0
    monkeypatch.setenv("ALAYA_FILTER_SCREEN", "0")
    assert _same(idx.filtered_search(queries.copy(), 10, 40, allow=allow), got)
    assert tuple(idx.native().screen_stats()) == (0, 0)
