"""The flat search's shortlist proof for inner products (alayalite_amd/csrc/flat_bound.h, DESIGN.md
"The flat shortlist bound for inner products"), where it can be wrong: the slack against emulated
contractions on the CPU, then on the device near-ties that walk each contraction's error bound
through the gap between the k-th and the shortlist's last distance, one outlier row that sets the
global row scale, and tiny bases with zero rows and zero queries.

Contract (include/alaya_hip.h): flat_search returns the exact top-k by (-(q.b), id) with the
oracle's distance bits; flat_search_device returns that for every query whose flag is 0."""

import numpy as np
import pytest

from flat_common import (FLAT_MODES, FLT_MAX, SWEEP_NQ, SWEEP_SHAPES, SWEEP_SIGMAS, _f16_exp, apply_flat_mode,
                         assert_exact, contraction_of, device_search, sweep_input)
from flat_ip_common import exact_ip, ip_gap64, ip_slack64

IP = 1


@pytest.fixture(params=FLAT_MODES)
def flat_mode(request, monkeypatch):
    """Every shortlist contraction and scan (flat_common.apply_flat_mode)."""
    return apply_flat_mode(monkeypatch, request.param)


_cache = {}


def _cached(key, make):
    """Inputs and references are computed once and shared by the eight modes (never modified)."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- 1. the slack against emulated contractions (CPU) ------------------------------------------
def _bf16(x):
    """bf16(x) as float32, round to nearest even, by integer operations on the f32 bits."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def _seq_sum(terms):
    """f32 sum of the columns of `terms` (pairs x terms, float32), left to right."""
    acc = np.zeros(terms.shape[0], np.float32)
    for j in range(terms.shape[1]):
        acc = (acc + terms[:, j]).astype(np.float32)
    return acc


def _pair_rows(rng, kind, m, d):
    if kind == "uniform":
        x = rng.random((m, d))
    elif kind == "gauss":
        x = rng.standard_normal((m, d))
    elif kind == "normalised":
        x = rng.standard_normal((m, d))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    else:  # integer-valued: products and most partial sums are exact, inner products cancel to 0
        x = rng.integers(-8, 9, (m, d)).astype(np.float64)
    if kind == "integer":
        scale = 2.0 ** rng.integers(-20, 14, (m, 1))  # 1e-6 .. 1e4, still integers times a power of two
    elif kind == "normalised":
        scale = np.ones((m, 1))
    else:
        scale = 10.0 ** rng.uniform(-6, 4, (m, 1))
    return np.ascontiguousarray((x * scale).astype(np.float32))


_SLACK_PAIRS = 6400  # per (d, kind): 4 d x 4 kinds x 6400 = 102,400 pairs


@pytest.mark.parametrize("kind", ["uniform", "gauss", "normalised", "integer"])
@pytest.mark.parametrize("d", [64, 128, 224, 960])
def test_flat_ip_slack_covers_emulated_contractions(native, orc, d, kind):
    """What the proof claims for an outside row and for the k-th row: the reference distance
    oracle.ip(q, b) lies within flat_ip_slack of fl32(-C~), for C~ emulated in numpy as the f32 form
    (two summation orders of rounded f32 products), the bf16 hi/lo split (qh.bh + qh.bl + ql.bh) and
    the single pass (power-of-two scaling, then float16; denormals kept and flushed).  b_max is the
    pair's own |b| (x 1.0001, as the index computes it): the tightest value the kernel can see."""
    rng = np.random.default_rng(7000 + d + len(kind))
    m = _SLACK_PAIRS
    q = _pair_rows(rng, kind, m, d)
    b = _pair_rows(rng, kind, m, d)
    lib = orc.lib()
    ref = np.array([lib.orc_ip_f32(q[i].ctypes.data, b[i].ctypes.data, d) for i in range(m)], np.float32)
    ref = ref.astype(np.float64)
    qn = (q.astype(np.float64) ** 2).sum(1).astype(np.float32)
    bmax = (np.sqrt((b.astype(np.float64) ** 2).sum(1)) * 1.0001).astype(np.float32)
    s_exp = np.array([_f16_exp(x) for x in bmax])
    t_exp = np.array([_f16_exp(x) for x in np.abs(q).max(1)])

    def slack(contraction):
        out = np.zeros(m)
        for i in range(m):
            out[i] = native.flat_ip_slack(contraction, d, qn[i:i + 1], t_exp[i:i + 1].astype(np.int32),
                                          float(bmax[i]), int(s_exp[i]))[0]
        assert np.isfinite(out).all()
        return out

    def check(what, c_tilde, sl):
        approx = (-c_tilde.astype(np.float32)).astype(np.float64)
        bad = np.nonzero(~((ref >= approx - sl) & (ref <= approx + sl)))[0]
        assert len(bad) == 0, (what, d, kind, len(bad), float(np.abs(ref - approx)[bad[0]]), float(sl[bad[0]]))

    # f32 MFMA: rounded products, two orders
    prod = (q * b).astype(np.float32)
    sl = slack(0)
    check("f32 forward", _seq_sum(prod), sl)
    check("f32 pairwise", prod.sum(1, dtype=np.float32), sl)
    # bf16 hi/lo split: the three kept products per element (exact in f32), the kernel's order
    qh, bh = _bf16(q), _bf16(b)
    ql, bl = _bf16(q - qh), _bf16(b - bh)
    terms = np.empty((m, 3 * d), np.float32)
    terms[:, 0::3], terms[:, 1::3], terms[:, 2::3] = ql * bh, qh * bl, qh * bh
    check("split", _seq_sum(terms), slack(1))
    # single pass: operands scaled by powers of two, rounded to f16, products exact in f32
    sl = slack(2)
    for flush in (False, True):
        with np.errstate(over="raise"):
            qs = np.ldexp(q, t_exp[:, None]).astype(np.float16)
            bs = np.ldexp(b, s_exp[:, None]).astype(np.float16)
        if flush:
            qs = np.where(np.abs(qs) < np.float16(2.0 ** -14), np.float16(0), qs)
            bs = np.where(np.abs(bs) < np.float16(2.0 ** -14), np.float16(0), bs)
        c = _seq_sum(qs.astype(np.float32) * bs.astype(np.float32))
        c = np.ldexp(c.astype(np.float64), -(s_exp + t_exp)).astype(np.float32)
        check("f16 flush" if flush else "f16", c, sl)


def test_flat_ip_proven_rounds_outward(native):
    """flat_ip_proven: exact when nothing is outside (cutoff FLT_MAX), never for an aborted block's
    cutoff, a NaN or an infinite slack; and a k-th distance equal to the rounded cutoff / 2 - slack
    is not proven (the comparison steps one float down from the rounded difference)."""
    f = np.float32
    kth = np.array([FLT_MAX, -1.0, -1.0, -1.0, -1.0, f(-1.0) - f(2.0 ** -23), -3.0, -0.0], np.float32)
    cut = np.array([FLT_MAX, -FLT_MAX, 4.0, np.nan, 4.0, -1.0, -1.0, 0.0], np.float32)
    slk = np.array([np.inf, 0.0, np.inf, 0.0, np.nan, 0.5, 0.5, 0.0], np.float32)
    got = native.flat_ip_proven(kth, cut, slk)
    #   cutoff/2 - slack = -1.0: kth = -1 - 2^-23 is the float below it (not proven), kth = -3 is
    assert got.tolist() == [1, 0, 0, 0, 0, 0, 1, 0]


# ---- 2. the sweep's inputs straddle the bound (CPU) --------------------------------------------
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=lambda s: "n%d-d%d-k%d" % s)
def test_flat_ip_sweep_inputs_straddle_bound(shape):
    """Describes the inputs, not the kernel: with flat_ip_slack restated in float64 and exact float64
    inner products, every query's gap (32nd - k-th distance; 128th - k-th for the big merge) is
    above 2 slack at sigma = 0.3 and below slack / 2 at sigma = 1e-5, in every mode."""
    n, d, k = shape
    for sigma, wide in ((0.3, True), (1e-5, False)):
        base, q = sweep_input(n, d, sigma)
        gap = ip_gap64(base, q, k)
        for mode in FLAT_MODES:
            sl = ip_slack64(mode, base, q)
            if wide:
                assert (gap > 2.0 * sl).all(), (mode, sigma, float((gap / sl).min()))
            else:
                assert (gap < 0.5 * sl).all(), (mode, sigma, float((gap / sl).max()))


def test_flat_ip_slack64_matches_native(native):
    """The float64 restatement used above is the function the kernels call (to f32 rounding)."""
    rng = np.random.default_rng(3)
    base = rng.random((500, 64), dtype=np.float32)
    q = rng.random((40, 64), dtype=np.float32)
    qn = (q.astype(np.float64) ** 2).sum(1).astype(np.float32)
    bmax = np.float32(np.sqrt((base.astype(np.float64) ** 2).sum(1).max()) * 1.0001)
    for mode, contraction in (("f32", 0), ("split", 1), ("f16-ws", 2)):
        t = np.array([_f16_exp(x) for x in np.abs(q).max(1)], np.int32)
        got = native.flat_ip_slack(contraction, 64, qn, t, float(bmax), _f16_exp(bmax))
        assert np.allclose(got, ip_slack64(mode, base, q), rtol=1e-5, atol=0)


def test_calc_gt_device_rejects_unknown_metric():
    """Before any device call (this test runs without a GPU)."""
    import alayalite_amd

    x = np.zeros((4, 8), np.float32)
    with pytest.raises(ValueError, match="metric"):
        alayalite_amd.utils.calc_gt_device(x, x, 2, metric="hamming")


# ---- 3. near-tie sweep -------------------------------------------------------------------------
_sweep_flags = {}  # (mode, (n, d, k), sigma) -> queries the device entry flagged, of SWEEP_NQ


def _sweep_case(native, orc, mode, shape, sigma):
    n, d, k = shape

    def make():
        base, q = sweep_input(n, d, sigma)
        return (base, q) + exact_ip(orc, base, q, k)

    base, q, ref_i, ref_d = _cached(("sweep", shape, sigma), make)
    dev = native.DeviceIndex(0)
    dev.set_base(base, IP)
    ids, dists, redo = dev.flat_search(q, k)
    ids_d, dists_d, flags = device_search(dev, q, k)
    nflag = int(flags.sum())
    _sweep_flags[(mode, shape, sigma)] = nflag
    print(f"flat ip sweep: mode={mode} shape={shape} sigma={sigma} device_flagged={nflag}/{len(q)} redo={redo}")
    assert_exact(ids, dists, ref_i, ref_d, what="flat_search")
    assert_exact(ids_d, dists_d, ref_i, ref_d, rows=flags == 0, what="flat_search_device, unflagged")
    if sigma == 0.3:
        assert nflag == 0 and redo == 0
    return nflag


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", SWEEP_SIGMAS)
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=lambda s: "n%d-d%d-k%d" % s)
def test_flat_ip_near_tie_sweep(native, orc, flat_mode, shape, sigma):
    """flat_common.sweep_input with metric IP: as sigma falls, the gap between the k-th inner-product
    distance and the shortlist's last one (linear in sigma, where L2's is quadratic) falls through
    each contraction's error bound.  flat_search is exact at every point; the device entry is exact
    on every query it does not flag; at sigma = 0.3 nothing is flagged.

    Queries the device entry flagged, of 48, on an MI355X (f16 stands for the four single-pass modes
    f16, f16-prescan2, f16-ws, f16-ws1; split for split and split-ws1; f32 for f32 and f32-prescan3;
    at d = 960 the f16 modes run the split).  The grid, then BOUNDARY_POINTS in brackets:

    shape (n, d, k)   contraction  0.3  0.1  0.03  0.01  0.003  0.001  1e-5
        (4000,  64, 10)   f16            0    0     0    48     48     48    48   [0.015: 5]
        (4000,  64, 10)   split          0    0     0     0      0      0    48   [0.000955: 36]
        (4000,  64, 10)   f32            0    0     0     0      0      0    48
        (4000, 128, 10)   f16            0    0     0    48     48     48    48   [0.025: 1, 0.02: 43]
        (4000, 128, 10)   split          0    0     0     0      0     48    48   [0.00206: 16]
        (4000, 128, 10)   f32            0    0     0     0      0      0    48   [0.000357: 39]
        (3000,  64, 50)   f16            0    0     0    48     48     48    48
        (3000,  64, 50)   split          0    0     0     0      0      0    48
        (3000,  64, 50)   f32            0    0     0     0      0      0    48
        (2000, 960, 10)   split          0    0     0    48     48     48    48   [0.015: 19]
        (2000, 960, 10)   f32            0    0     0     0     48     48    48   [0.00455: 0, 0.0044: 1,
                                                                                   0.00424: 25, 0.0041: 48, 0.00395: 48]

    The inner-product gap falls linearly with sigma (L2's quadratically), so every contraction
    proves more of the grid than for L2, and all 48 queries cross together (see BOUNDARY_POINTS)."""
    _sweep_case(native, orc, flat_mode, shape, sigma)


# The inner-product gap of sweep_input is c.(b_32 - b_k) to first order in sigma -- the same rows for
# every query -- so all 48 queries cross the bound within a few per cent of one sigma, and
# SWEEP_SIGMAS steps over that window in every mode.  These points sit in it: gap / slack (float64,
# flat_ip_common) between 0.93 and 1.07 over the queries for the contraction named.
BOUNDARY_POINTS = [
    ((4000, 64, 10), 0.015), ((4000, 128, 10), 0.025), ((4000, 128, 10), 0.02),  # single-pass f16
    ((2000, 960, 10), 0.015), ((4000, 128, 10), 0.00206), ((4000, 64, 10), 0.000955),  # bf16 hi/lo split
    ((2000, 960, 10), 0.00395), ((2000, 960, 10), 0.0041), ((2000, 960, 10), 0.00424),  # f32
    ((2000, 960, 10), 0.0044), ((2000, 960, 10), 0.00455), ((4000, 128, 10), 0.000357),
]


@pytest.mark.gpu
@pytest.mark.parametrize("point", BOUNDARY_POINTS, ids=lambda p: "n%d-d%d-k%d-s%g" % (p[0] + (p[1],)))
def test_flat_ip_near_tie_boundary(native, orc, flat_mode, point):
    """The sweep's checks at the sigmas where the gap crosses each contraction's bound."""
    _sweep_case(native, orc, flat_mode, *point)


@pytest.mark.gpu
def test_flat_ip_near_tie_sweep_has_mixed_point(native, orc, flat_mode):
    """The device-entry check of the sweep is not vacuous: in every mode some grid or boundary
    point has both flagged and unflagged queries."""
    counts = {}
    for shape, sigma in [(sh, sg) for sh in SWEEP_SHAPES for sg in SWEEP_SIGMAS] + BOUNDARY_POINTS:
        key = (flat_mode, shape, sigma)
        counts[(shape, sigma)] = _sweep_flags[key] if key in _sweep_flags else _sweep_case(
            native, orc, flat_mode, shape, sigma)
    mixed = [key for key, c in counts.items() if 0 < c < SWEEP_NQ]
    print(f"flat ip sweep: mode={flat_mode} mixed points {mixed}")
    assert mixed, counts


# ---- 4. one outlier row sets the global scale --------------------------------------------------
_OUTLIER = 1234


def _outlier_input(orc, m, sign, masked):
    def make():
        rng = np.random.default_rng(44)
        base = np.ascontiguousarray(rng.random((3000, 64), dtype=np.float32))
        q = np.ascontiguousarray(rng.random((8, 64), dtype=np.float32))
        base[_OUTLIER] *= np.float32(sign * 2.0 ** m)
        valid = np.ones(len(base), np.uint8)
        if masked:
            valid[_OUTLIER] = 0
        return (base, q, valid) + exact_ip(orc, base, q, 10, valid=valid)

    return _cached(("outlier", m, sign, masked), make)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["valid", "cleared"])
@pytest.mark.parametrize("sign", [1, -1], ids=["top1", "worst"])
@pytest.mark.parametrize("m", [12, 24, 40])
def test_flat_ip_outlier_row_sets_scale(native, orc, flat_mode, m, sign, masked):
    """Row 1234 is multiplied by +-2^m: as is it becomes every query's top-1, negated every query's
    worst row.  Either way the row scale 2^s and the bound's max|b| come from it, so the bound grows
    by 2^m past every gap between ordinary rows: the queries go through the split rerun and the
    exhaustive redo, and stay exact.  Cleared in the validity bitmap it is never returned (the scale
    still comes from every stored row)."""
    base, q, valid, ref_i, ref_d = _outlier_input(orc, m, sign, masked)
    if sign > 0 and not masked:
        assert (ref_i[:, 0] == _OUTLIER).all()
    dev = native.DeviceIndex(0)
    dev.set_base(base, IP, np.packbits(valid, bitorder="little") if masked else None)
    ids, dists, redo = dev.flat_search(q, 10)
    ids_d, dists_d, flags = device_search(dev, q, 10)
    print(f"flat ip outlier: mode={flat_mode} m={m} sign={sign} masked={masked} device_flagged={int(flags.sum())}/8 "
          f"redo={redo}")
    assert_exact(ids, dists, ref_i, ref_d, what="flat_search")
    assert_exact(ids_d, dists_d, ref_i, ref_d, rows=flags == 0, what="flat_search_device, unflagged")
    if masked or sign < 0:
        assert not (ids == _OUTLIER).any()
    if masked:
        assert not (ids_d == _OUTLIER).any()


# ---- 5. tiny bases -----------------------------------------------------------------------------
def _tiny_input(orc, n, d, nq):
    def make():
        rng = np.random.default_rng(1000 * n + d)
        base = np.ascontiguousarray(rng.random((n, d), dtype=np.float32))
        q = np.ascontiguousarray(rng.random((nq, d), dtype=np.float32))
        if n > 1 or d == 100:  # one all-zero row (the single row of n = 1 at d = 100 only)
            base[n // 2] = 0.0
        if nq > 1:  # all-zero queries: one inside a wave of ordinary ones, one alone in its wave
            q[7] = 0.0
            q[32] = 0.0
        return (base, q) + exact_ip(orc, base, q, 10)

    return _cached(("tiny", n, d, nq), make)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [32, 100, 960])
@pytest.mark.parametrize("n", [1, 9, 10, 11, 31, 32, 33, 64, 65, 257])
def test_flat_ip_tiny_base_exact(native, orc, flat_mode, n, d):
    """1 to 9 tile records against at least 8 chunks, a zero row, and zero queries whose distances
    all tie at the reference's -0.0: ids and distance bits are the oracle's, in order, for 1 and for
    33 queries; slots past n hold (0xffffffff, FLT_MAX)."""
    for nq in (1, 33):
        base, q, ref_i, ref_d = _tiny_input(orc, n, d, nq)
        if n < 10:
            assert (ref_i[:, n:] == 0xFFFFFFFF).all() and (ref_d[:, n:] == FLT_MAX).all()
        if nq > 1:  # the reference's zero-query distance is -0.0
            assert (ref_d[7, :min(n, 10)].view(np.uint32) == 0x80000000).all()
        dev = native.DeviceIndex(0)
        dev.set_base(base, IP)
        ids, dists, redo = dev.flat_search(q, 10)
        assert_exact(ids, dists, ref_i, ref_d, what=f"flat_search nq={nq}")
        ids_d, dists_d, flags = device_search(dev, q, 10)
        assert_exact(ids_d, dists_d, ref_i, ref_d, rows=flags == 0, what=f"flat_search_device nq={nq}, unflagged")
