"""A search launch is planned for the kernel it gets (csrc/search_variants.h).

Where the shape has no kernel with a wanted feature, resolve_search_variant drops the feature and
the host plans for the kernel that was chosen: dropped helpers give the launch shape of a search
without helpers and help_stats() of zero, and dropped stamps are an error, not stamps of zero."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2000


def _index(native, base, metric=0):
    g = native.Graph.build(base, metric, 32, 100, 8, 100)
    dev = native.DeviceIndex(0)
    dev.set_base(base, metric)
    dev.set_graph(g)
    return g, dev


def test_helpers_dropped_by_the_stamped_kernel(native):
    """f32 d = 256 has helper kernels (mode 4) and only the runtime-d stamped kernel (mode 1): a
    profiled search with helpers on runs the latter, so it is planned without helpers."""
    rng = np.random.default_rng(2560)
    base = rng.standard_normal((N, 256)).astype(np.float32)
    queries = rng.standard_normal((64, 256)).astype(np.float32)
    assert native.search_variant(256, False, 0, False, 1 | 4)[0] == (0, 0, 1)
    _, dev = _index(native, base)
    dev.set_helpers(0)
    ids0, _, cnt0 = dev.search(queries, 10, 32)
    dev.profile_search(queries, 10, 32, 0)
    shape0 = dev.last_launch()
    dev.set_helpers(1)
    dev.search(queries, 10, 32)
    assert dev.last_launch()[1] == 4 and dev.last_launch() != shape0  # (helpers do change the shape)
    ids, cnt, stamps = dev.profile_search(queries, 10, 32, 0)
    assert np.array_equal(ids, ids0) and np.array_equal(cnt, cnt0)
    assert dev.help_stats() == (0, 0, 0)
    assert dev.last_launch() == shape0
    assert (stamps[:, 6] > 0).all()  # the stamped kernel ran: every query has a total


def test_stamps_dropped_is_an_error(native, orc):
    """SQ8 d = 960 has no stamped kernel: profile_search says so and leaves the index as it was."""
    rng = np.random.default_rng(9600)
    base = rng.standard_normal((N, 960)).astype(np.float32)
    queries = rng.standard_normal((16, 960)).astype(np.float32)
    g, dev = _index(native, base)
    mn, mx = native.sq8_train(base)
    codes = native.sq8_encode(base, mn, mx, 8)
    dev.set_sq8(codes, mn, mx, 2)
    with pytest.raises(ValueError, match=r"no stamped search kernel for dim 960 SQ8"):
        dev.profile_search(queries, 10, 32, 1)
    l0, levels, off, ue, ep, ur, _ = g.arrays()
    view = orc.IndexView(base, l0, levels, off, ue, ur, ep, metric=0, sq8=(codes, mn, mx, 2))
    ids, dists, cnt = dev.search_sq8(queries, 10, 32, 0)
    for i, q in enumerate(queries):
        o_ids, o_d, o_c = view.search(q, 10, 32, with_counters=True)
        assert np.array_equal(ids[i], o_ids), i
        assert np.array_equal(dists[i].view(np.uint32), o_d.view(np.uint32)), i
        assert tuple(cnt[i]) == tuple(o_c), i
