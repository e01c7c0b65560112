"""The MFMA range scan's thresholds (alayalite_amd/csrc/flat_range_bound.h, DESIGN.md "Round 24") and its launch
plan, on the CPU: the function the scan's prologue calls against a bf16-split contraction emulated in numpy."""

import numpy as np
import pytest

from test_flat_ip_bound import _bf16, _pair_rows, _seq_sum

SPLIT = 1


def _split_contraction(q, b, forward):
    """qh.bh + qh.bl + ql.bh summed in f32: the kernel's order, or numpy's pairwise one."""
    qh, bh = _bf16(q), _bf16(b)
    ql, bl = _bf16(q - qh), _bf16(b - bh)
    terms = np.empty((len(q), 3 * q.shape[1]), np.float32)
    terms[:, 0::3], terms[:, 1::3], terms[:, 2::3] = ql * bh, qh * bl, qh * bh
    return _seq_sum(terms) if forward else terms.sum(1, dtype=np.float32)


@pytest.mark.parametrize("kind", ["uniform", "gauss", "normalised", "integer"])
@pytest.mark.parametrize("d", [64, 100, 960])
@pytest.mark.parametrize("ip", [0, 1])
def test_thresholds_never_misjudge(native, orc, ip, d, kind):
    """d~ <= lo implies d_ref <= r and d~ > hi implies d_ref > r, for radii at and around d_ref (the steps span
    the band of every scale drawn) and at the infinities; b_max is the pair's own |b| x 1.0001."""
    rng = np.random.default_rng(9000 + d + len(kind) + ip)
    m = 1500
    q, b = _pair_rows(rng, kind, m, d), _pair_rows(rng, kind, m, d)
    if kind == "gauss":  # near pairs: the distance cancels against the norms
        b[::2] = (q[::2] * (1 + 1e-3 * rng.standard_normal((m // 2 + m % 2, d)))).astype(np.float32)
    lib = orc.lib()
    f = lib.orc_ip_f32 if ip else lib.orc_l2_f32
    ref = np.array([f(q[i].ctypes.data, b[i].ctypes.data, d) for i in range(m)], np.float32)
    k_acc = -(-d // 64) * 64
    qn = _seq_sum(q * q)
    bn = (b * b).sum(1, dtype=np.float32)
    bmax = (np.sqrt((b.astype(np.float64) ** 2).sum(1)) * 1.0001).astype(np.float32)
    exact64 = (-(q.astype(np.float64) * b).sum(1)) if ip else ((q.astype(np.float64) - b) ** 2).sum(1)
    assert np.allclose(ref, exact64, rtol=1e-4, atol=1e-4 * np.sqrt(qn.astype(np.float64)) * bmax + 1e-30)
    for forward in (True, False):
        c = _split_contraction(q, b, forward)
        approx = -c if ip else ((qn + bn).astype(np.float32) - np.float32(2) * c).astype(np.float32)
        for step in (0, 1, -1, 2.0 ** -20, -2.0 ** -20, 2.0 ** -14, -2.0 ** -14, 2.0 ** -8, -2.0 ** -8, np.inf, -np.inf):
            if abs(step) == 1:
                radii = np.nextafter(ref, np.float32(step * np.inf))
            elif np.isinf(step):
                radii = np.full(m, step, np.float32)
            else:
                radii = (ref + np.float32(step) * np.maximum(np.abs(ref), qn + bn)).astype(np.float32)
            lo, hi = (np.empty(m, np.float32) for _ in range(2))
            for i in range(m):
                lo[i], hi[i] = (x[0] for x in native.flat_range_bound(ip, SPLIT, k_acc, float(bmax[i]), radii[i:i + 1], qn[i:i + 1]))
            assert not np.isnan(lo).any() and (lo <= hi).all()
            wrong_in = np.nonzero((approx <= lo) & ~(ref <= radii))[0]
            wrong_out = np.nonzero((approx > hi) & ~(ref > radii))[0]
            assert len(wrong_in) == 0 and len(wrong_out) == 0, (ip, d, kind, step, wrong_in[:3], wrong_out[:3])
            if step in (2.0 ** -8, -2.0 ** -8):  # far from the radius nothing is left to verify
                assert ((approx <= lo) | (approx > hi)).mean() > 0.9, (ip, d, kind, step)


def test_no_bound_and_special_radii(native):
    one = np.ones(1, np.float32)
    for ip in (0, 1):
        for bmax, qn, k_acc in ((1e18, 1.0, 64), (np.inf, 1.0, 64), (1.0, np.inf, 64), (1.0, np.nan, 64), (1.0, 1.0, 0),
                                (1.0, 1.0, 65600)):
            lo, hi = native.flat_range_bound(ip, SPLIT, k_acc, bmax, one, one * np.float32(qn))
            assert lo[0] == -np.inf and hi[0] == np.inf
        lo, hi = native.flat_range_bound(ip, SPLIT, 64, 2.0, np.array([-np.inf, np.inf, np.nan], np.float32), np.ones(3, np.float32))
        assert hi[0] == -np.inf and lo[1] == np.inf and np.isnan(lo[2]) and np.isnan(hi[2])


@pytest.mark.parametrize("n", [1, 127, 128, 129, 5000, 1_000_000, 100_000_000])
@pytest.mark.parametrize("nq", [1, 128, 129, 1000, 100_000])
def test_plan_invariants(native, n, nq):
    for cap in (1, 100, 4096):
        for cus in (1, 256):
            rows, chunks, tile, sub, slots, staging = native.flat_range_mfma_plan(n, nq, cap, cus)
            assert rows % 128 == 0 and chunks * rows >= n > (chunks - 1) * rows
            assert tile == 128 and sub % 128 == 0 and sub >= 128 and slots == min(cap, rows)
            assert staging == chunks * min(-(-nq // 128) * 128, sub) * (8 * slots + 4) <= 256 << 20
