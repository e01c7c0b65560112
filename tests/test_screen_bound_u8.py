"""The candidate screen's lower bound over the 8-bit screening copy (csrc/screen_bound.h, DESIGN.md
section 3, "Round 8") on the CPU.

``native.screen_u8_quantize`` runs, on the host, the quantiser, ``screen_u8_value`` and the e_row
formula that the device's copy kernel runs; the search kernel sums ``d~`` over the same
``screen_u8_value``.  As in ``test_screen_bound.py`` the bound must never exceed the distance the
reference computes (``oracle.l2``): d~ is summed in f32 in two orders over the values the codes stand
for, for the four screened dimensions, the row shapes of that test and the edge cases of this copy
(constant rows, rows x 1e5 and x 1e-6, one huge outlier per row, ``q == x``, a non-finite element).
"""

import numpy as np
import pytest

DIMS = [512, 768, 960, 1024]


def _d_tilde_orders(q, y):
    """f32 sums of (q - y)^2 in two orders: numpy's pairwise sum, and a strict left-to-right one."""
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (q - y) ** 2  # f32 differences, f32 products
        pairwise = sq.sum(-1, dtype=np.float32)
        sequential = np.cumsum(sq[..., ::-1], axis=-1, dtype=np.float32)[..., -1]
    return pairwise, sequential


def _copy(native, x, exact_in_f64=True):
    """(values y, e_row) of the host build of the copy; checks the record's own invariants.
    exact_in_f64: lo + c * scale fits float64 exactly (lo and the row's range of similar magnitude), so
    the one rounding of screen_u8_value can be checked there."""
    codes, head, y = native.screen_u8_quantize(x)
    e, lo, scale = head[:, 0], head[:, 1], head[:, 2]
    assert codes.dtype == np.uint8 and y.dtype == np.float32 and (head[:, 3] == 0).all()
    fin = np.isfinite(x).all(-1) & np.isfinite(e)
    with np.errstate(over="ignore", invalid="ignore"):
        # e_row >= ||x - y|| in float64, and y is lo + c * scale rounded once
        err64 = np.sqrt(((x[fin].astype(np.float64) - y[fin].astype(np.float64)) ** 2).sum(-1))
        assert (e[fin].astype(np.float64) >= err64).all()
        y64 = lo[fin, None].astype(np.float64) + codes[fin].astype(np.float64) * scale[fin, None].astype(np.float64)
        assert not exact_in_f64 or np.array_equal(y[fin], y64.astype(np.float32))
    assert np.isinf(e[~np.isfinite(x).all(-1)]).all()
    return y, e


def _check(native, orc, q, x, exact_in_f64=True):
    dim = x.shape[1]
    y, e = _copy(native, x, exact_in_f64)
    ref = np.array([orc.l2(a, b) for a, b in zip(q, x)], np.float32)
    for d_t in _d_tilde_orders(q, y):
        lb = native.screen_lower_bound(d_t, e, dim)
        assert lb.dtype == np.float32 and np.isfinite(lb).all() and (lb >= 0).all()
        assert (lb[~np.isfinite(e)] == 0).all()  # rows the copy cannot bound are never screened out
        ok = (lb <= ref) | ((lb == 0) & np.isnan(ref))
        assert ok.all(), (dim, np.flatnonzero(~ok)[:5], lb[~ok][:5], ref[~ok][:5], d_t[~ok][:5], e[~ok][:5])
    return len(x)


def _gist_rows(rng, n, dim):
    centres = rng.uniform(0, 0.5, (8, dim)).astype(np.float32)
    return np.clip(centres[rng.integers(0, 8, n)] + rng.normal(0, 0.05, (n, dim)), 0, 1).astype(np.float32)


@pytest.mark.parametrize("dim", DIMS)
def test_u8_bound_below_reference_distance(native, orc, dim):
    rng = np.random.default_rng(8000 + dim)
    n = 2000
    total = 0
    # uniform, gist-shaped, integer-valued ({0, 1, 2}: 1 is no code; and 4097 levels)
    for x, q in [
        (rng.uniform(-1, 1, (n, dim)).astype(np.float32), rng.uniform(-1, 1, (n, dim)).astype(np.float32)),
        (_gist_rows(rng, n, dim), _gist_rows(rng, n, dim)),
        (rng.integers(0, 3, (n, dim)).astype(np.float32), rng.integers(0, 3, (n, dim)).astype(np.float32)),
        (rng.integers(-2048, 2049, (n, dim)).astype(np.float32), rng.uniform(-2048, 2048, (n, dim)).astype(np.float32)),
    ]:
        total += _check(native, orc, q, x)
    # the bound is not vacuous: on gist-shaped rows it is above 0.9 of the distance
    x, q = _gist_rows(rng, 64, dim), _gist_rows(rng, 64, dim)
    y, e = _copy(native, x)
    lb = native.screen_lower_bound(_d_tilde_orders(q, y)[0], e, dim)
    ref = np.array([orc.l2(a, b) for a, b in zip(q, x)])
    assert (lb > 0.9 * ref).all()
    # q == x, q one f32 ulp away, and q == the values the codes stand for
    x = rng.uniform(-1, 1, (n // 4, dim)).astype(np.float32)
    total += _check(native, orc, x.copy(), x)
    total += _check(native, orc, np.nextafter(x, np.float32(2)), x)
    total += _check(native, orc, _copy(native, x)[0], x)
    # constant rows (scale 0, codes 0, the copy exact), q equal, near and far
    c = np.repeat(rng.uniform(-3, 3, (n // 8, 1)).astype(np.float32), dim, axis=1)
    assert (native.screen_u8_quantize(c)[0] == 0).all() and (native.screen_u8_quantize(c)[1][:, 2] == 0).all()
    total += _check(native, orc, c.copy(), c)
    total += _check(native, orc, np.nextafter(c, np.float32(4)), c)
    total += _check(native, orc, rng.uniform(-3, 3, c.shape).astype(np.float32), c)
    # rows x 1e5 and x 1e-6 (both representable here), and magnitudes between, per row
    for scale in [1e-6, 1e-3, 1.0, 1e2, 1e5]:
        x = (_gist_rows(rng, n // 8, dim) * np.float32(scale)).astype(np.float32)
        q = (_gist_rows(rng, n // 8, dim) * np.float32(scale)).astype(np.float32)
        total += _check(native, orc, q, x)
    # one huge outlier per row: the step swallows the rest of the row (a large e_row, a weak bound)
    x = rng.uniform(-1, 1, (n // 4, dim)).astype(np.float32)
    x[np.arange(len(x)), rng.integers(0, dim, len(x))] = rng.choice(np.array([1e4, -1e6, 3e30, -3e38], np.float32), len(x))
    total += _check(native, orc, rng.uniform(-1, 1, x.shape).astype(np.float32), x, exact_in_f64=False)
    total += _check(native, orc, x.copy(), x, exact_in_f64=False)
    # max - min overflows f32: no finite scale, no bound
    x = rng.uniform(-1, 1, (16, dim)).astype(np.float32)
    x[:, 1], x[:, 2] = np.float32(3e38), np.float32(-3e38)
    assert np.isinf(native.screen_u8_quantize(x)[1][:, 0]).all()
    total += _check(native, orc, rng.uniform(-1, 1, x.shape).astype(np.float32), x)
    # a non-finite element: e_row = +inf, bound 0
    x = rng.uniform(-1, 1, (48, dim)).astype(np.float32)
    x[0::3, 5] = np.float32(np.inf)
    x[1::3, 7] = np.float32(-np.inf)
    x[2::3, dim - 1] = np.float32(np.nan)
    q = rng.uniform(-1, 1, x.shape).astype(np.float32)
    y, e = _copy(native, x)
    assert np.isinf(e).all()
    for d_t in _d_tilde_orders(q, y):
        assert (native.screen_lower_bound(d_t, e, dim) == 0).all()
    total += _check(native, orc, q, x)
    assert total >= 12000  # distinct (q, x) pairs; x 4 dimensions, x 2 summation orders
