"""The flat search's shortlist proof where it can be wrong: near-ties that walk each contraction's
error bound through the gap between the k-th and the shortlist's last distance, mixed magnitudes
inside one wave of queries, one outlier row that sets the global row scale, and tiny bases.

Contract (include/alaya_hip.h): flat_search returns the exact top-k by (distance, id) with the
oracle's distance bits; flat_search_device returns that for every query whose flag is 0."""

import numpy as np
import pytest

from flat_common import (FLAT_MODES, FLT_MAX, SWEEP_NQ, SWEEP_SHAPES, SWEEP_SIGMAS, apply_flat_mode, assert_exact,
                         contraction_of, device_search, exact, exact_fast, shortlist_eps64, shortlist_gap64,
                         sweep_input)


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


# ---- 1. near-tie sweep -------------------------------------------------------------------------
_sweep_flags = {}  # (mode, (n, d, k), sigma) -> queries the device entry flagged, of SWEEP_NQ


def _sweep_case(native, orc, mode, shape, sigma):
    n, d, k = shape

    def make():
        base, q = sweep_input(n, d, sigma)
        return (base, q) + exact_fast(orc, base, q, k)

    base, q, ref_i, ref_d = _cached(("sweep", shape, sigma), make)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0)
    ids, dists, redo = dev.flat_search(q, k)
    ids_d, dists_d, flags = device_search(dev, q, k)
    assert dev.flat_contraction() == contraction_of(mode, d)
    nflag = int(flags.sum())
    _sweep_flags[(mode, shape, sigma)] = nflag
    print(f"flat sweep: mode={mode} shape={shape} sigma={sigma} device_flagged={nflag}/{len(q)} redo={redo}")
    assert_exact(ids, dists, ref_i, ref_d, what="flat_search")
    assert_exact(ids_d, dists_d, ref_i, ref_d, rows=flags == 0, what="flat_search_device, unflagged")
    if sigma == 0.3:
        assert nflag == 0 and redo == 0
    return nflag


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", SWEEP_SIGMAS)
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=lambda s: "n%d-d%d-k%d" % s)
def test_flat_near_tie_sweep(native, orc, flat_mode, shape, sigma):
    """Rows and queries in a cluster of width sigma around one point: as sigma falls, the gap between
    the k-th distance and the shortlist's last one falls through each contraction's error bound
    (test_flat_sweep_inputs_straddle_bound pins that on the CPU), and the approximate ranking
    mis-orders hundreds of rows while the exact (distance, id) order still exists.  flat_search is
    exact at every point; the device entry is exact on every query it does not flag; at
    sigma = 0.3 nothing is flagged.  At sigma = 1e-5 most f16 operands are equal across rows, so the
    approximate distances differ through the f32 row norms alone.

    Queries the device entry flagged, of 48, on an MI355X (f16 stands for the four single-pass modes
    f16, f16-prescan2, f16-ws, f16-ws1; split for split and split-ws1; f32 for f32 and f32-prescan3;
    at d = 960 the f16 modes run the split):

    shape (n, d, k)   contraction  0.3  0.1  0.03  0.01  0.003  0.001  1e-5
        (4000,  64, 10)   f16            0    7    48    48     48     48    48
        (4000,  64, 10)   split          0    0     4    48     48     48    48
        (4000,  64, 10)   f32            0    0     0    37     48     48    48
        (4000, 128, 10)   f16            0   25    48    48     48     48    48
        (4000, 128, 10)   split          0    0    48    48     48     48    48
        (4000, 128, 10)   f32            0    0     0    48     48     48    48
        (3000,  64, 50)   f16            0    0    48    48     48     48    48
        (3000,  64, 50)   split          0    0     0    48     48     48    48
        (3000,  64, 50)   f32            0    0     0    28     48     48    48
        (2000, 960, 10)   split          0   46    48    48     48     48    48
        (2000, 960, 10)   f32            0    0    48    48     48     48    48

    Points with flagged and unflagged queries: f16 at sigma 0.1 (d = 64, 128, 960), split at 0.03
    (d = 64) and 0.1 (d = 960), f32 at 0.01 (d = 64, both k).  With the bound's slack multiplied by
    0 the f16 mode returns unflagged wrong rows from sigma = 0.01 down and the split from 0.003 down
    (at d = 960 both at 0.003 and 1e-5 only); multiplied by 1/8 every point still passes, and by 1/64 the f16
    mode fails at 0.01 and 1e-5 (k = 50: also 0.001) and the split at 1e-5 (d = 64): the
    contractions' real error sits between 8x and 64x below the bound, so the sweep proves the proof
    sound, not tight.
    """
    _sweep_case(native, orc, flat_mode, shape, sigma)


@pytest.mark.gpu
def test_flat_near_tie_sweep_has_mixed_point(native, orc, flat_mode):
    """The device-entry check of the sweep is not vacuous: in every mode some grid point has both
    flagged and unflagged queries, i.e. the proof is decided query by query right at its boundary
    and the unflagged ones are compared with the oracle there."""
    counts = {}
    for shape in SWEEP_SHAPES:
        for sigma in SWEEP_SIGMAS:
            key = (flat_mode, shape, sigma)
            counts[(shape, sigma)] = _sweep_flags[key] if key in _sweep_flags else _sweep_case(
                native, orc, flat_mode, shape, sigma)
    mixed = [key for key, c in counts.items() if 0 < c < SWEEP_NQ]
    print(f"flat sweep: mode={flat_mode} mixed points {mixed}")
    assert mixed, counts


# ---- 2. the sweep's inputs straddle the bound (CPU) --------------------------------------------
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=lambda s: "n%d-d%d-k%d" % s)
def test_flat_sweep_inputs_straddle_bound(shape):
    """Describes the inputs, not the kernel: with shortlist_eps restated in float64 and exact float64
    distances, every query's gap (32nd - k-th distance; 128th - k-th for the big merge) is above
    2 eps at sigma = 0.3 and below eps / 2 at sigma = 0.003, in every mode.  A change of shape or
    seed that turns the sweep into another wide-gap test fails here."""
    n, d, k = shape
    for sigma, wide in ((0.3, True), (0.003, False)):
        base, q = sweep_input(n, d, sigma)
        gap = shortlist_gap64(base, q, k)
        for mode in FLAT_MODES:
            eps = shortlist_eps64(mode, base, q)
            if wide:
                assert (gap > 2.0 * eps).all(), (mode, sigma, float((gap / eps).min()))
            else:
                assert (gap < 0.5 * eps).all(), (mode, sigma, float((gap / eps).max()))


# ---- 3. mixed query magnitudes inside one wave -------------------------------------------------
def _mixed_input(orc):
    def make():
        rng = np.random.default_rng(33)
        base = np.ascontiguousarray(rng.random((4000, 64), dtype=np.float32))
        q = np.ascontiguousarray(rng.random((64, 64), dtype=np.float32))
        return (base, q) + exact_fast(orc, base, q, 10)

    return _cached("mixed", make)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [4, 8, 12, 16, 24, 40, -4, -8, -12, -16, -24, -40])
def test_flat_mixed_query_scale_in_wave(native, orc, flat_mode, m):
    """Query 5 of a wave of 32 is multiplied by 2^m.  m > 0: the single-role scan scales the whole
    wave by its largest element, so the 31 ordinary queries keep ever fewer f16 bits and then land
    in the f16 denormals; their bound grows with 2^-t |b| and must flag what it cannot prove.
    m < 0: query 5 itself loses the bits.  Queries 32..63 are an untouched control wave.  The answer
    is exact for all 64, rows 0..31 other than 5 do not depend on query 5 being in the batch, and
    the device entry is exact where it does not flag.

    Rows 0..31 the device entry flagged on an MI355X:

    m                                  4   8  12  16  24  40  (every m < 0)
        f16, f16-prescan2 (per-wave scale) 0   0   1   1  32  32   0
        the six other modes                0   0   1   1   1   1   0

    The control wave 32..63 is never flagged.
    """
    base, q, ref_i0, ref_d0 = _mixed_input(orc)

    def make():
        qs = q.copy()
        qs[5] *= np.float32(2.0 ** m)
        ri, rd = exact_fast(orc, base, qs[5:6], 10)
        ref_i, ref_d = ref_i0.copy(), ref_d0.copy()
        ref_i[5], ref_d[5] = ri[0], rd[0]
        return qs, ref_i, ref_d

    qs, ref_i, ref_d = _cached(("mixed", m), make)
    dev = native.DeviceIndex(0)
    dev.set_base(base, 0)
    ids0, dists0, _ = dev.flat_search(q, 10)
    ids, dists, redo = dev.flat_search(qs, 10)
    ids_d, dists_d, flags = device_search(dev, qs, 10)
    print(f"flat mixed: mode={flat_mode} m={m} device_flagged_rows_0_31={int(flags[:32].sum())} "
          f"control_32_63={int(flags[32:].sum())} redo={redo}")
    assert_exact(ids, dists, ref_i, ref_d, what="flat_search")
    others = np.array([a for a in range(32) if a != 5])
    assert np.array_equal(ids[others], ids0[others])
    assert np.array_equal(dists[others].view(np.uint32), dists0[others].view(np.uint32))
    assert_exact(ids_d, dists_d, ref_i, ref_d, rows=flags == 0, what="flat_search_device, unflagged")


# ---- 4. one outlier row sets the global scale --------------------------------------------------
_OUTLIER = 1234


def _outlier_input(orc, m, masked):
    def make():
        rng = np.random.default_rng(44)
        base = np.ascontiguousarray(rng.random((3000, 64), dtype=np.float32))
        q = np.ascontiguousarray(rng.random((8, 64), dtype=np.float32))
        base[_OUTLIER] *= np.float32(2.0 ** m)
        valid = np.ones(len(base), np.uint8)
        if masked:
            valid[_OUTLIER] = 0
        live = np.nonzero(valid)[0]
        ref_i, ref_d = exact(orc, base[live], q, 10)
        return base, q, valid, live[ref_i].astype(np.uint32), ref_d

    return _cached(("outlier", m, masked), make)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["valid", "cleared"])
@pytest.mark.parametrize("m", [12, 24, 40, 60, 64])
def test_flat_outlier_row_sets_scale(native, orc, flat_mode, m, masked):
    """Row 1234 is multiplied by 2^m.  The row scale 2^s and the bound's max|b| come from the largest
    row norm, so every other row moves towards (and into) the f16 denormals and the bound grows by
    2^m: most queries go through the split rerun and the exhaustive redo, and stay exact.  At
    m = 64 the outlier's squared norm is inf in f32: max|b| is not finite and the f32 contraction
    runs.  With the outlier cleared in the validity bitmap it is never returned and the answer is
    the oracle's over the valid rows (the scale still comes from every stored row)."""
    base, q, valid, ref_i, ref_d = _outlier_input(orc, m, masked)
    dev = native.DeviceIndex(0)
    # the validity bitmap: bit i % 8 of byte i / 8 set = row i valid
    dev.set_base(base, 0, np.packbits(valid, bitorder="little") if masked else None)
    ids, dists, redo = dev.flat_search(q, 10)
    if m == 64 and flat_mode.startswith("f16"):
        assert dev.flat_contraction() == 0
    ids_d, dists_d, flags = device_search(dev, q, 10)
    print(f"flat outlier: mode={flat_mode} m={m} masked={masked} device_flagged={int(flags.sum())}/8 redo={redo}")
    assert_exact(ids, dists, ref_i, ref_d, what="flat_search")
    assert_exact(ids_d, dists_d, ref_i, ref_d, rows=flags == 0, what="flat_search_device, unflagged")
    if masked:
        assert not (ids == _OUTLIER).any() and not (ids_d == _OUTLIER).any()


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
        return (base, q) + exact(orc, base, q, 10)

    return _cached(("tiny", n, d, nq), make)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [32, 100, 960])
@pytest.mark.parametrize("n", [1, 9, 10, 11, 31, 32, 33, 64, 65, 100, 257])
def test_flat_tiny_base_exact(native, orc, flat_mode, n, d):
    """1 to 9 tile records against at least 8 chunks: most chunks are empty and the shortlists are
    short.  ids and distance bits are the oracle's, in order, for 1 and for 33 queries; slots past
    n hold (0xffffffff, FLT_MAX)."""
    for nq in (1, 33):
        base, q, ref_i, ref_d = _tiny_input(orc, n, d, nq)
        if n < 10:
            assert (ref_i[:, n:] == 0xFFFFFFFF).all() and (ref_d[:, n:] == FLT_MAX).all()
        dev = native.DeviceIndex(0)
        dev.set_base(base, 0)
        ids, dists, redo = dev.flat_search(q, 10)
        assert_exact(ids, dists, ref_i, ref_d, what=f"flat_search nq={nq}")
        ids_d, dists_d, flags = device_search(dev, q, 10)
        assert_exact(ids_d, dists_d, ref_i, ref_d, rows=flags == 0, what=f"flat_search_device nq={nq}, unflagged")
