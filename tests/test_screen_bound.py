"""The candidate screen's lower bound (csrc/screen_bound.h) on the CPU.

The graph search drops a candidate without reading its f32 row when
``screen_lower_bound(d~, e_row, dim) >= tau``; that is exact only if the bound never exceeds the
distance the reference computes (l2_sqr_avx2, ``oracle.l2``).  The header compiles for the host
into the engine's library (the kernel calls the same function), so this test evaluates it for
> 100k pairs: d~ summed in f32 in two different orders over the f16 copy, e_row taken in float64 and
rounded up, across the four screened dimensions, three row shapes and the edge cases of the copy
(identical rows, f16 rounding midpoints, magnitudes from 1e-7 to 6e4, rows past the f16 range).
"""

import numpy as np
import pytest

DIMS = [512, 768, 960, 1024]


def _copy_and_err(x):
    """(f16 copy as f32, e_row >= ||x - copy|| rounded up; +inf where the copy is not finite)."""
    with np.errstate(over="ignore"):
        y = x.astype(np.float16).astype(np.float32)
    e = np.sqrt(((x.astype(np.float64) - y.astype(np.float64)) ** 2).sum(-1)) * (1 + 1e-12)
    e32 = np.nextafter(e.astype(np.float32), np.float32(np.inf))
    e32 = np.where(e32.astype(np.float64) >= e, e32, np.nextafter(e32, np.float32(np.inf)))
    bad = ~np.isfinite(y).all(-1)
    e32[bad] = np.inf
    return y, e32.astype(np.float32)


def _d_tilde_orders(q, y):
    """f32 sums of (q - y)^2 in two orders: numpy's pairwise sum, and a strict left-to-right one."""
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (q - y) ** 2  # f32 differences, f32 products
        pairwise = sq.sum(-1, dtype=np.float32)
        sequential = np.cumsum(sq[..., ::-1], axis=-1, dtype=np.float32)[..., -1]
    return pairwise, sequential


def _check(native, orc, q, x):
    dim = x.shape[1]
    y, e = _copy_and_err(x)
    ref = np.array([orc.l2(a, b) for a, b in zip(q, x)], np.float32)
    for d_t in _d_tilde_orders(q, y):
        lb = native.screen_lower_bound(d_t, e, dim)
        assert lb.dtype == np.float32 and np.isfinite(lb).all() and (lb >= 0).all()
        assert (lb[~np.isfinite(e)] == 0).all()  # rows the copy cannot hold are never screened out
        ok = (lb <= ref) | ((lb == 0) & np.isnan(ref))
        assert ok.all(), (dim, np.flatnonzero(~ok)[:5], lb[~ok][:5], ref[~ok][:5], d_t[~ok][:5], e[~ok][:5])
    return len(x)


def _gist_rows(rng, n, dim):
    centres = rng.uniform(0, 0.5, (8, dim)).astype(np.float32)
    return np.clip(centres[rng.integers(0, 8, n)] + rng.normal(0, 0.05, (n, dim)), 0, 1).astype(np.float32)


@pytest.mark.parametrize("dim", DIMS)
def test_bound_below_reference_distance(native, orc, dim):
    rng = np.random.default_rng(dim)
    n = 4400
    total = 0
    # uniform, gist-shaped, integer-valued
    for x, q in [
        (rng.uniform(-1, 1, (n, dim)).astype(np.float32), rng.uniform(-1, 1, (n, dim)).astype(np.float32)),
        (_gist_rows(rng, n, dim), _gist_rows(rng, n, dim)),
        (rng.integers(0, 3, (n, dim)).astype(np.float32), rng.integers(0, 3, (n, dim)).astype(np.float32)),
        (rng.integers(-2048, 2049, (n, dim)).astype(np.float32), rng.uniform(-2048, 2048, (n, dim)).astype(np.float32)),
    ]:
        total += _check(native, orc, q, x)
    # the bound is not vacuous: on gist-shaped rows it is within 5 % of the distance
    x, q = _gist_rows(rng, 64, dim), _gist_rows(rng, 64, dim)
    y, e = _copy_and_err(x)
    lb = native.screen_lower_bound(_d_tilde_orders(q, y)[0], e, dim)
    ref = np.array([orc.l2(a, b) for a, b in zip(q, x)])
    assert (lb > 0.95 * ref).all()
    # q == x, and q one f32 ulp / one f16 ulp away from x
    x = rng.uniform(-1, 1, (n // 4, dim)).astype(np.float32)
    total += _check(native, orc, x.copy(), x)
    total += _check(native, orc, np.nextafter(x, np.float32(2)), x)
    total += _check(native, orc, x.astype(np.float16).astype(np.float32), x)
    # x at f16 rounding midpoints (the largest copy error), q near and far
    h = rng.uniform(0.25, 2, (n // 4, dim)).astype(np.float16)
    mid = (h.astype(np.float32) + np.nextafter(h, np.float16(4)).astype(np.float32)) / np.float32(2)
    total += _check(native, orc, h.astype(np.float32), mid)
    total += _check(native, orc, rng.uniform(0, 2, mid.shape).astype(np.float32), mid)
    # magnitudes 1e-7 .. 6e4, per row and mixed inside a row
    for scale in [1e-7, 1e-5, 1e-3, 1.0, 1e2, 6e4]:
        x = (rng.uniform(-1, 1, (n // 8, dim)) * scale).astype(np.float32)
        q = (rng.uniform(-1, 1, (n // 8, dim)) * scale).astype(np.float32)
        total += _check(native, orc, q, x)
    mixed = (10.0 ** rng.uniform(-7, np.log10(6e4), (n // 4, dim))).astype(np.float32)
    total += _check(native, orc, (mixed * rng.uniform(0.5, 1.5, mixed.shape)).astype(np.float32), mixed)
    # rows just past the f16 range: 65504 < x < 65520 still rounds to 65504, above it overflows
    x = rng.uniform(-1, 1, (n // 8, dim)).astype(np.float32)
    x[:, 3] = np.float32(65519.0)
    total += _check(native, orc, rng.uniform(-1, 1, x.shape).astype(np.float32), x)
    x[:, 3] = np.float32(65520.0)
    x[::2, 7] = np.float32(1e5)
    x[1::4, 9] = np.float32(-3e38)
    total += _check(native, orc, rng.uniform(-1, 1, x.shape).astype(np.float32), x)
    assert total >= 25000  # distinct (q, x) pairs; x 4 dimensions > 100k


def test_bound_special_values(native):
    f = native.screen_lower_bound
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    d = np.array([1.0, 1.0, nan, inf, 1e35, 0.0, 1e-30, 1.0, 1.0, 4.0], np.float32)
    e = np.array([inf, nan, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0, -1.0, 1.0], np.float32)
    out = f(d, e, 960)
    assert (out[:9] == 0).all()  # no bound: never screens
    assert 0.99 < out[9] <= 1.0  # (sqrt(4) - 1)^2, just below
    # monotone in d~ and in e_row
    dd = np.linspace(0.5, 50, 1000).astype(np.float32)
    assert (np.diff(f(dd, np.full_like(dd, 0.01), 960)) >= 0).all()
    ee = np.linspace(0, 3, 1000).astype(np.float32)
    assert (np.diff(f(np.full_like(ee, 9.0), ee, 960)) <= 0).all()
