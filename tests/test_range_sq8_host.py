"""The restatement of the range search on an SQ8 index (tests/range_sq8_common.py) and the inputs of
test_range_sq8_gpu.py, without a GPU.

The restatement is filter_sq8_common's replay read another way, so what is pinned here is the reading itself,
on a hand-made stream, and that the inputs reach both directions in which a code distance and an exact one
disagree: rows the code radius lets in and the rerank cut removes ("coarse": 75 of 279 candidates), and rows
that slack 0 misses (the IP shapes: 32 of 204).  The figures are sums over the 12 queries at ef 40 without a
mask, radius = the query's m-th smallest exact distance among its pairs, slack 0, measured with the oracle on
these inputs; the two code orders differ in none of them.  They are the issue's table re-measured, and equal it
but for one cell: (7, L2) at m = 64 has 4 rows that are in by code and out by exact distance, where the table
says 7 -- 4 is what agrees with the table's own 765 candidates (768 exact hits - 7 code-out + 4 code-in).  No
query offers 4096 pairs: a cap of 4096 never truncates, caps of 64 and below do."""

import numpy as np
import pytest

import filter_sq8_common as sc
import range_sq8_common as rq

# (dim, metric, kind): pairs per query (lo, hi), then per m in (17, 64): (exact hits, candidates, code in and
# exact out, code out and exact in)
FIGURES = {
    (64, 0, "gist"): ((448, 553), (204, 206, 4, 2), (768, 772, 5, 1)),
    (64, 0, "coarse"): ((447, 558), (204, 279, 75, 0), (768, 1027, 259, 0)),
    (128, 1, "gist"): ((451, 649), (204, 172, 0, 32), (768, 692, 0, 76)),
    (768, 1, "gist"): ((575, 671), (204, 169, 0, 35), (768, 680, 0, 88)),
    (960, 0, "gist"): ((577, 657), (204, 213, 9, 0), (768, 788, 20, 0)),
    (100, 0, "gist"): ((504, 603), (204, 204, 2, 2), (768, 779, 11, 0)),
    (7, 0, "gist"): ((216, 351), (204, 202, 6, 8), (768, 765, 4, 7)),
}


class _Orc:
    """orc.dist of the hand-made stream: the 'row' is its exact distance."""

    @staticmethod
    def dist(metric, rq_, row):
        return row


def _want(pairs, exact, radius, c, cap):
    base = {v: np.float32(e) for (v, _), e in zip(pairs, exact)}
    return rq.want_row(_Orc, base, 0, None, pairs, radius, c, cap)


def test_restatement_on_a_hand_made_stream():
    f = np.float32
    pairs = [(7, f(2.0)), (3, f(1.0)), (9, f(3.5)), (1, f(2.0)), (5, f(0.5)), (2, f(2.5)), (8, f(1.5))]
    exact = [2.25, -0.0, 1.75, 2.0, 0.0, 1.0, 2.0]  # row 9: code out, exact in; row 7: code in, exact out
    n, cand, ids, d = _want(pairs, exact, 2.0, 2.0, 8)
    assert (n, cand) == (4, 5) and ids.tolist() == [3, 5, 1, 8] + [sc.EMPTY] * 4  # -0.0 ties +0.0: the id decides
    assert d.view(np.uint32)[0] == 0x80000000 and d.view(np.uint32)[1] == 0 and (d[4:] == sc.FLT_MAX).all()
    assert d[2] == 2.0  # the exact distance comes back, inclusive at the radius
    n, cand, ids, d = _want(pairs, exact, 2.0, rq.code_radius(2.0, 0.5), 8)  # the slack admits row 2, not row 9
    assert (n, cand) == (5, 6) and ids.tolist() == [3, 5, 2, 1, 8] + [sc.EMPTY] * 3
    n, cand, ids, d = _want(pairs, exact, 2.0, rq.code_radius(2.0, np.inf), 8)  # every pair a candidate
    assert (n, cand) == (6, 7) and ids.tolist() == [3, 5, 2, 9, 1, 8] + [sc.EMPTY] * 2
    n, cand, ids, d = _want(pairs, exact, 2.0, np.inf, 3)  # truncated: the first three to arrive, then the cut
    assert (n, cand) == (2, 7) and ids.tolist() == [3, 9, sc.EMPTY]
    n, cand, ids, d = _want(pairs, exact, np.nextafter(f(-0.0), f(-np.inf)), np.inf, 8)  # below every exact distance
    assert (n, cand) == (0, 7) and (ids == sc.EMPTY).all() and (d == sc.FLT_MAX).all()
    assert _want(pairs, exact, 2.0, np.nextafter(f(0.5), f(0.0)), 8)[:2] == (0, 0)
    assert rq.code_radius(3.0e38, 3.0e38) == np.inf and rq.code_radius(-1.0, 0.0) == f(-1.0)


def test_slack_above_covers_the_gap():
    for radius, gap in [(1.0, 0.1), (-0.7, 3e-9), (100.0, 1e-7), (0.0, 0.0), (-3.0, 0.25)]:
        s = rq.slack_above(radius, gap)
        assert s >= 0 and float(rq.code_radius(radius, s)) >= float(np.float32(radius)) + gap, (radius, gap, s)


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("dim,metric,kind", list(FIGURES))
def test_inputs_reach_both_disagreements(orc, dim, metric, kind, order):
    base, queries, _, _ = sc.inputs(orc, dim, metric, kind)
    rs = rq.replays(orc, dim, metric, kind, order, 40)
    n = [len(r["pairs"]) for r in rs]
    got = [(min(n), max(n))]
    for m in (17, 64):
        hits = cands = code_in = code_out = 0
        for q, r in zip(queries, rs):
            radius = rq.mth_exact(orc, base, metric, q, r["pairs"], m)
            exact = rq.exact_of(orc, base, metric, q, r["pairs"])
            for (_, d), e in zip(r["pairs"], exact):
                c_in, e_in = bool(np.float32(d) <= radius), bool(e <= radius)
                hits += e_in
                cands += c_in
                code_in += c_in and not e_in
                code_out += e_in and not c_in
            # the restatement at slack 0 and a cap nothing reaches: candidates and hits as counted here
            w = rq.want_row(orc, base, metric, q, r["pairs"], radius, rq.code_radius(radius, 0.0), 4096)
            assert w[1] == sum(np.float32(d) <= radius for _, d in r["pairs"])
            # with the worst overstatement as slack every exact-in pair is a candidate
            s = rq.slack_above(radius, rq.worst_overstatement(orc, base, metric, q, r["pairs"], radius))
            w = rq.want_row(orc, base, metric, q, r["pairs"], radius, rq.code_radius(radius, s), 4096)
            assert w[0] == sum(e <= radius for e in exact), (dim, metric, kind, order, m)
        got.append((hits, cands, code_in, code_out))
    print(dim, metric, kind, order, got)
    assert tuple(got) == FIGURES[(dim, metric, kind)], (dim, metric, kind, order, got)
    assert max(n) < 4096 and min(n) > 64
