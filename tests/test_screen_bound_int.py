"""The integer screen's lower bound (csrc/screen_bound.h, DESIGN.md section 3, "Round 10") on the CPU.

``native.screen_int_bound(queries, rows)`` runs, on the host, what the search kernel runs for a
candidate under ``ALAYA_SEARCH_SCREEN=9``: both vectors through the 8-bit quantiser, the five exact
integer sums, ``screen_int_distance`` (a value ``d_in <= D^ = ||q^ - y^||^2`` over the real-valued grids
``lo + scale * code``), ``screen_int_err`` (``e_sum >= ||x - y^|| + ||q - q^||``) and ``screen_lower_bound``.

Checked, for the pair families of ``test_screen_bound_u8.py`` and the failure modes the query's own
quantisation adds:
* the bound never exceeds the distance the reference computes (``oracle.l2``);
* the integer sums are those of the codes ``native.screen_u8_quantize`` returns (Python / int64);
* ``d_in <= D^`` with ``D^`` evaluated exactly in ``fractions.Fraction`` from the headers and sums, on a
  sample of each family (every 8th pair of the four large ones, every 4th of the others, every pair of
  the overflow and non-finite ones: ~3k pairs per width; the other checks run on every pair), and on
  six pairs ``D^`` itself against the element-wise sum, also exact;
* ``e_sum`` against float64 norms over the real grids.  No margin is given to it: the float64 evaluation
  is off by at most ~2^-47 M (M = the largest grid magnitude), and ``e_sum`` carries 2^-18 M for a
  difference ``||y - y^||`` that is at most sqrt(n) 2^-24 M <= 2^-19 M here.
"""

from fractions import Fraction

import numpy as np
import pytest

DIMS = [512, 768, 960, 1024]


def _gist_rows(rng, n, dim):
    centres = rng.uniform(0, 0.5, (8, dim)).astype(np.float32)
    return np.clip(centres[rng.integers(0, 8, n)] + rng.normal(0, 0.05, (n, dim)), 0, 1).astype(np.float32)


def _exact_grid_distance(n, qh, rh, s):
    """D^ as a Fraction from the two headers (err, lo, scale, 0) and the sums (A1, A2, C1, C2, AC)."""
    qlo, qs, lo, sc = (Fraction(float(v)) for v in (qh[1], qh[2], rh[1], rh[2]))
    a1, a2, c1, c2, ac = (int(v) for v in s)
    delta = qlo - lo
    return n * delta * delta + 2 * delta * (qs * a1 - sc * c1) + qs * qs * a2 + sc * sc * c2 - 2 * qs * sc * ac


def _check(native, orc, q, x, every=1):
    """One family of pairs; `every`: the exact D^ check on every `every`-th pair (all other checks on all)."""
    n, dim = x.shape
    d_in, e_sum, bound, sums = native.screen_int_bound(q, x)
    assert d_in.dtype == e_sum.dtype == bound.dtype == np.float32 and sums.dtype == np.uint32
    a, qh, _ = native.screen_u8_quantize(q)
    c, rh, _ = native.screen_u8_quantize(x)
    a64, c64 = a.astype(np.int64), c.astype(np.int64)
    want = np.stack([a64.sum(-1), (a64 * a64).sum(-1), c64.sum(-1), (c64 * c64).sum(-1), (a64 * c64).sum(-1)], -1)
    assert np.array_equal(sums.astype(np.int64), want)
    # the bound against the reference
    ref = np.array([orc.l2(u, v) for u, v in zip(q, x)], np.float32)
    assert np.isfinite(bound).all() and (bound >= 0).all()
    ok = (bound <= ref) | ((bound == 0) & np.isnan(ref))
    assert ok.all(), (dim, np.flatnonzero(~ok)[:5], bound[~ok][:5], ref[~ok][:5], d_in[~ok][:5], e_sum[~ok][:5])
    # vectors the quantiser cannot bound are never screened out
    unbounded = ~np.isfinite(qh[:, 0]) | ~np.isfinite(rh[:, 0])
    assert (bound[unbounded] == 0).all() and np.isinf(e_sum[unbounded]).all()
    assert (~np.isfinite(q).all(-1) <= np.isinf(qh[:, 0])).all() and (~np.isfinite(x).all(-1) <= np.isinf(rh[:, 0])).all()
    # d_in <= D^, exactly
    assert np.isfinite(d_in).all() and (d_in >= 0).all()
    for i in range(0, n, every):
        exact = _exact_grid_distance(dim, qh[i], rh[i], sums[i])
        assert Fraction(float(d_in[i])) <= max(exact, 0), (dim, i, float(d_in[i]), float(exact))
    # e_sum >= ||x - y^|| + ||q - q^|| over the real grids, in float64
    fin = ~unbounded
    with np.errstate(over="ignore", invalid="ignore"):
        y_hat = rh[fin, 1:2].astype(np.float64) + rh[fin, 2:3].astype(np.float64) * c64[fin]
        q_hat = qh[fin, 1:2].astype(np.float64) + qh[fin, 2:3].astype(np.float64) * a64[fin]
        need = np.sqrt(((x[fin] - y_hat) ** 2).sum(-1)) + np.sqrt(((q[fin] - q_hat) ** 2).sum(-1))
    assert (e_sum[fin].astype(np.float64) >= need).all()
    return n


@pytest.mark.parametrize("dim", DIMS)
def test_int_bound_below_reference_distance(native, orc, dim):
    rng = np.random.default_rng(10000 + dim)
    n = 2000
    total = 0
    uni = lambda k: rng.uniform(-1, 1, (k, dim)).astype(np.float32)  # noqa: E731
    # uniform, gist-shaped, integer-valued ({0, 1, 2}: 1 is no code; and 4097 levels)
    for x, q in [
        (uni(n), uni(n)),
        (_gist_rows(rng, n, dim), _gist_rows(rng, n, dim)),
        (rng.integers(0, 3, (n, dim)).astype(np.float32), rng.integers(0, 3, (n, dim)).astype(np.float32)),
        (rng.integers(-2048, 2049, (n, dim)).astype(np.float32), rng.uniform(-2048, 2048, (n, dim)).astype(np.float32)),
    ]:
        total += _check(native, orc, q, x, every=8)
    # the bound is not vacuous: on gist-shaped rows it is above 0.9 of the distance
    x, q = _gist_rows(rng, 64, dim), _gist_rows(rng, 64, dim)
    bound = native.screen_int_bound(q, x)[2]
    ref = np.array([orc.l2(u, v) for u, v in zip(q, x)])
    print(f"dim {dim}: bound / reference distance min {float((bound / ref).min()):.4f}")
    assert (bound > 0.9 * ref).all()
    # the identity itself: D^ from the sums == sum (q^_j - y^_j)^2, both exact
    a, qh, _ = native.screen_u8_quantize(q[:6])
    c, rh, _ = native.screen_u8_quantize(x[:6])
    sums = native.screen_int_bound(q[:6], x[:6])[3]
    for i in range(6):
        qlo, qs, lo, sc = (Fraction(float(v)) for v in (qh[i, 1], qh[i, 2], rh[i, 1], rh[i, 2]))
        direct = sum(((qlo + qs * int(u)) - (lo + sc * int(v))) ** 2 for u, v in zip(a[i], c[i]))
        assert direct == _exact_grid_distance(dim, qh[i], rh[i], sums[i])
    # q == x, q one f32 ulp away, and q == the values the row's codes stand for
    x = uni(n // 4)
    total += _check(native, orc, x.copy(), x, every=4)
    total += _check(native, orc, np.nextafter(x, np.float32(2)), x, every=4)
    total += _check(native, orc, native.screen_u8_quantize(x)[2], x, every=4)
    # constant rows (scale 0) under equal, near and far queries; constant queries (qs = 0) on any row
    const = np.repeat(rng.uniform(-3, 3, (n // 8, 1)).astype(np.float32), dim, axis=1)
    total += _check(native, orc, const.copy(), const, every=4)
    total += _check(native, orc, np.nextafter(const, np.float32(4)), const, every=4)
    total += _check(native, orc, rng.uniform(-3, 3, const.shape).astype(np.float32), const, every=4)
    total += _check(native, orc, const, rng.uniform(-3, 3, const.shape).astype(np.float32), every=4)
    assert (native.screen_u8_quantize(const)[1][:, 2] == 0).all()
    # rows x 1e5 and x 1e-6 and magnitudes between, the query of the row's magnitude
    for scale in [1e-6, 1e-3, 1.0, 1e2, 1e5]:
        x = (_gist_rows(rng, n // 8, dim) * np.float32(scale)).astype(np.float32)
        q = (_gist_rows(rng, n // 8, dim) * np.float32(scale)).astype(np.float32)
        total += _check(native, orc, q, x, every=4)
    # a query x 1e5 against rows x 1e-6, and the other way round
    x = (_gist_rows(rng, n // 8, dim) * np.float32(1e-6)).astype(np.float32)
    q = (_gist_rows(rng, n // 8, dim) * np.float32(1e5)).astype(np.float32)
    total += _check(native, orc, q, x, every=4)
    total += _check(native, orc, x, q, every=4)
    # rows and queries shifted by +1e4: the identity's terms dwarf the distance and cancel
    x = (_gist_rows(rng, n // 4, dim) + np.float32(1e4)).astype(np.float32)
    q = (_gist_rows(rng, n // 4, dim) + np.float32(1e4)).astype(np.float32)
    total += _check(native, orc, q, x, every=4)
    total += _check(native, orc, (q - np.float32(2e4)).astype(np.float32), x, every=4)  # delta large, opposite signs
    # one huge outlier per row, and per query
    x = uni(n // 4)
    x[np.arange(len(x)), rng.integers(0, dim, len(x))] = rng.choice(np.array([1e4, -1e6, 3e30, -3e38], np.float32), len(x))
    total += _check(native, orc, uni(len(x)), x, every=4)
    total += _check(native, orc, x.copy(), x, every=4)
    total += _check(native, orc, x, uni(len(x)), every=4)
    # max - min overflows f32, in the row or in the query: no finite scale, no bound
    x = uni(16)
    x[:, 1], x[:, 2] = np.float32(3e38), np.float32(-3e38)
    assert (native.screen_int_bound(uni(16), x)[2] == 0).all() and (native.screen_int_bound(x, uni(16))[2] == 0).all()
    total += _check(native, orc, uni(16), x) + _check(native, orc, x, uni(16))
    # a non-finite element, in the row or in the query: bound 0
    x = uni(48)
    x[0::3, 5] = np.float32(np.inf)
    x[1::3, 7] = np.float32(-np.inf)
    x[2::3, dim - 1] = np.float32(np.nan)
    for q_, x_ in [(uni(48), x), (x, uni(48)), (x, x.copy())]:
        d_in, e_sum, bound, _ = native.screen_int_bound(q_, x_)
        assert (bound == 0).all() and np.isinf(e_sum).all()
        total += _check(native, orc, q_, x_)
    assert total >= 14000  # pairs per dimension
