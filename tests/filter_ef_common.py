"""Shared by test_filter_ef_host.py and test_filter_ef_gpu.py: the case lists of the three filtered graph
searches at ef above 64 and at the row widths the other filter files leave out.  The GPU file runs them against
the restatements (filter_common, filter_hop_common, filter_sq8_common); the host file asserts, for the same
tuples, that the restatement fills its traversal pool and goes on rejecting, so no GPU case is vacuous.

A plain or through case is (dim, metric, kind, k, ef, share); an SQ8 case is (dim, metric, order, k, ef, m,
share).  Inputs are filter_common.graph's: 2000 rows, 12 queries, orc.build_hnsw(base, metric, 32, 100)."""

import numpy as np

import degree_common as dc
import filter_common as fc
import filter_hop_common as hc
import filter_sq8_common as sc

# d = 256, 512, 768, 1024: the chunk-8 / 16 / 24 / 32 kernels
WIDE_SHAPES = [(256, 0), (512, 1), (768, 0), (1024, 0)]
PLAIN_KEFS = [(10, 65, 0.1), (10, 129, 0.1), (10, 200, 0.02), (100, 387, 0.5)]
# the through pool holds allowed rows only: at share 0.1 (about 200 rows) it never reaches ef 129
HOP_KEFS = [(10, 65, 0.2), (10, 129, 0.5), (32, 200, 0.5), (100, 387, 0.5)]
HOP_ROUND17 = (960, 0, "gist", 10, 387, 0.5)  # the through search's measured configuration

# the register merge (d = 128 and 256, ef <= 128: lane l holds entries l and 64 + l) and its two edges
MERGE_SHAPES = [(128, 0), (256, 1)]
MERGE_EFS = [64, 65, 127, 128, 129]
MERGE_PLAIN_SHARE, MERGE_HOP_SHARE = 0.1, 0.5
TIE = (128, 0, "tie", 10, 100, 0.3)

SQ8_SHAPES = [(768, 1), (128, 0), (100, 0)]
SQ8_KEFS = [(10, 200, 40, 0.1), (10, 129, 224, 0.5), (10, 387, 10, 0.02), (10, 65, 65, 0.1)]
SQ8_FORCED = (768, 1, 2, 10, 200, 40, 0.1)  # once under the spill-table forcing, once under the bitset forcing

PLAN = (960, 0, 224, 40, 387, 0.5)  # (dim, metric, k, small ef, large ef, share): the plan moves with ef

# several queries per wave: the queries are base rows 0..47, masks of these two shares alternate by query
WAVE_EF, WAVE_NQ, WAVE_SHARES = 200, 48, (0.5, 0.02)
WAVE_F32 = (256, 0)
WAVE_SQ8 = (128, 0, 2)  # (dim, metric, order)

# three masks in one batch at ef 387 (d = 512 IP); the through search's second mask is a second draw of
# share 0.5 and its third all ones, so every pool fills
THREE = (512, 1, 10, 387)
THREE_PLAIN_SHARES = (0.5, 0.2, 0.02)
THREE_HOP_SEED = 4242

# ef at and above the row count: the pool never fills
OVER = (64, 0, 10, 0.1)  # (dim, metric, k, share)
OVER_EFS = [2000, 2048]

# the LDS-budget edge: (dim, metric, k, share), SQ8 with m = k
EDGE = (1024, 0, 224, 0.5)


def plain_cases():
    """Every (dim, metric, kind, k, ef, share) the plain filtered search runs with one mask on fc.graph's own
    queries (the batch cases -- several queries per wave, three masks -- are listed apart)."""
    out = [(d, m, "gist", k, ef, s) for d, m in WIDE_SHAPES for k, ef, s in PLAIN_KEFS]
    out += [(d, m, "gist", 10, ef, MERGE_PLAIN_SHARE) for d, m in MERGE_SHAPES for ef in MERGE_EFS]
    out += [TIE]
    out += [(PLAN[0], PLAN[1], "gist", PLAN[2], ef, PLAN[5]) for ef in PLAN[3:5]]
    out += [(THREE[0], THREE[1], "gist", THREE[2], THREE[3], s) for s in THREE_PLAIN_SHARES]
    return out


def hop_cases():
    out = [(d, m, "gist", k, ef, s) for d, m in WIDE_SHAPES for k, ef, s in HOP_KEFS]
    out += [HOP_ROUND17]
    out += [(d, m, "gist", 10, ef, MERGE_HOP_SHARE) for d, m in MERGE_SHAPES for ef in MERGE_EFS]
    out += [TIE]
    out += [(PLAN[0], PLAN[1], "gist", PLAN[2], ef, PLAN[5]) for ef in PLAN[3:5]]
    out += [(THREE[0], THREE[1], "gist", THREE[2], THREE[3], s) for s in (0.5, 1.0)]
    return out


def sq8_cases():
    return [(d, m, o, k, ef, pool, s) for d, m in SQ8_SHAPES for o in (2, 1) for k, ef, pool, s in SQ8_KEFS]


def second_half_mask(n):
    """The through search's second mask of about half the rows (another draw than filter_common.mask's)."""
    return np.random.default_rng(THREE_HOP_SEED).random(n) < 0.5


_wave = {}


def wave_wants(orc, kernel):
    """The restatement's rows of the several-queries-per-wave case of a kernel ("plain", "through" or "sq8"),
    in query order: query i is base row i under the mask of share WAVE_SHARES[i % 2]."""
    if kernel not in _wave:
        masks = [fc.mask(fc.N, s) for s in WAVE_SHARES]
        if kernel == "sq8":
            dim, metric, order = WAVE_SQ8
            base, _, arrays, quant = sc.inputs(orc, dim, metric)
            view = dc.view_of(orc, base, arrays, metric)
            _wave[kernel] = [sc.replay(orc, view, quant, order, base[i], 10, WAVE_EF, WAVE_EF, masks[i % 2], metric)
                             for i in range(WAVE_NQ)]
        else:
            dim, metric = WAVE_F32
            base, _, arrays = fc.graph(orc, dim, metric)
            view = dc.view_of(orc, base, arrays, metric)
            one = fc.replay if kernel == "plain" else hc.replay
            _wave[kernel] = [one(orc, view, base[i], 10, WAVE_EF, masks[i % 2], metric) for i in range(WAVE_NQ)]
    return _wave[kernel]
