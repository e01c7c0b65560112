"""Shared by test_spill_clean_host.py and test_spill_clean.py: the inputs with which every graph search kernel
family is driven into the visited set's second level on a few persistent searchers, and the host conditions
that make a clean read-back (DeviceIndex.spill_residue) mean something.

The second level is per-index scratch (include/alaya_hip.h, alaya_index_spill_residue): per searcher slot an
n-bit bitset with a dirty-word list of ALAYA_DIRTY_CAP words and, for AVX-512-order SQ8 searches, a spill table.
A query that spilled puts back what it set before its slot takes the next query -- word by word from its dirty
list, or the whole bitset when the list overflowed.

Nothing here is a new reference: every family's expected answer is the restatement its own tests use
(degree_common / filter_common / filter_hop_common / filter_sq8_common / range_common / range_more_common /
range_sq8_common, and the oracle's search for the two unfiltered families), on filter_common's 2000-row graphs.
The queries are 250 of the base rows, so that with the grid held to two workgroups every slot runs 30 to 125
queries one after the other.

Conditions (check_inputs), per query, from the replay's own counts:
  * visited > fill limit of the 64-slot first level (64 * 11 // 16): the query spills;
  * bitset ids > 3 * 32, where bitset ids = visited - 64 (the first level never holds more) - table entries
    (64 with ALAYA_SPILL_TABLE=6, whose entries the first level is flushed into; 0 for the f32 kernels): the ids
    that reach the bitset cannot fit three 32-bit words, so a 3-word dirty list overflows and the query takes the
    whole-bitset wipe.
``visited`` is the number of rows the query marks: n_dist + the entry for the traversals that mark only what
they measure, n_dist + n_through + the entry for the through search, and the replay's own count for the radius
mode."""

import numpy as np

import degree_common as dc
import filter_common as fc
import filter_hop_common as hc
import filter_sq8_common as sc
import range_common as rc
import range_more_common as rm
import range_sq8_common as rq

EMPTY, FLT_MAX, N = fc.EMPTY, fc.FLT_MAX, fc.N
INF = np.float32(np.inf)
HASH_LOG2 = 6                                 # set_hash_log2(6): 64 first-level slots
FILL_LIMIT = (1 << HASH_LOG2) * 11 // 16      # entries after which the first level spills
SPILL_TABLE_LOG2 = 6                          # ALAYA_SPILL_TABLE=6: 64-entry tables, buckets fill, ids go on to the bitset
K = 10
NQ = 250
SHARE = 0.1
ORDER = 2                                     # AVX-512 reduction order: the SQ8 kernels that have spill tables
FLOOD_AT = 3                                  # the radius mode's FLT_MAX query: others follow it in both directions
FAMILIES = ("plain", "sq8", "filtered", "hop", "filtered_sq8", "range", "range_more", "range_sq8")
SQ8_FAMILIES = ("sq8", "filtered_sq8", "range_sq8")
EF = {"plain": 24, "sq8": 40, "filtered": 24, "hop": 16, "filtered_sq8": 40, "range": 24, "range_more": 16, "range_sq8": 40}
RANGE_CAP = {"range": 24, "range_more": 512, "range_sq8": 64}
MAX_FRONTIER = 4096
_cases = {}


def queries_of(base):
    """NQ base rows, every eighth."""
    return np.ascontiguousarray(base[:NQ * 8:8])


def words(allow, n=N):
    from alayalite_amd.utils import pack_allow

    return pack_allow(allow, n)


def _exact_mth(base, queries, m):
    """Per query, about the m-th smallest L2 distance to a base row (float64 arithmetic, rounded to f32): a
    radius, not a reference."""
    b = base.astype(np.float64)
    q = queries.astype(np.float64)
    d = (q * q).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (q @ b.T)
    return np.sort(d, axis=1)[:, m - 1].astype(np.float32)


def case(orc, family, dim=64):
    """The family's input and expected answers on the (dim, L2) graph, cached: a dict with base, queries, arrays,
    ef, want (one restatement per query), visited (rows each query marks), table (ids the spill table can hold
    before the bitset is used) and what the family's call needs beside them (allow, radii, code_radii, quant)."""
    key = (family, dim)
    if key in _cases:
        return _cases[key]
    ef = EF[family]
    if family in SQ8_FAMILIES:
        base, _, arrays, quant = sc.inputs(orc, dim, 0)
    else:
        base, _, arrays = fc.graph(orc, dim, 0)
        quant = None
    queries = queries_of(base)
    view = dc.view_of(orc, base, arrays, 0)
    allow = fc.mask(N, SHARE)
    ones = np.ones(N, bool)
    c = dict(family=family, dim=dim, base=base, queries=queries, arrays=arrays, ef=ef, quant=quant,
             table=(1 << SPILL_TABLE_LOG2) if family in SQ8_FAMILIES else 0)
    if family in ("plain", "sq8"):
        v = view if family == "plain" else sc.view_of(orc, base, arrays, 0, quant, ORDER)
        want = [v.search(q, K, ef, with_counters=True) for q in queries]
        c.update(want=want, visited=[int(w[2][0]) + 1 for w in want])
    elif family == "filtered":
        want = fc.replays(orc, dim, 0, "spill", K, ef, SHARE, view=view, queries=queries, allow=allow)
        c.update(want=want, allow=allow, visited=[r["counters"][0] + 1 for r in want])
    elif family == "hop":
        want = hc.replays(orc, dim, 0, "spill", K, ef, SHARE, view=view, queries=queries, allow=allow)
        c.update(want=want, allow=allow, visited=[r["counters"][0] + r["counters"][4] + len(r["entries"]) for r in want])
    elif family == "filtered_sq8":
        want = [sc.replay(orc, view, quant, ORDER, q, K, ef, ef, allow, 0) for q in queries]
        c.update(want=want, allow=allow, pool=ef, visited=[r["counters"][0] + 1 for r in want])
    elif family == "range":
        want = rc.replays(orc, dim, 0, "spill", ef, SHARE, view=view, queries=queries, allow=allow)
        # the 25th hit of the cap-24 list where the query has that many pairs, so lists both fill and overflow
        radii = np.array([rc.mth_distance(r, min(25, len(r["pairs"]))) if r["pairs"] else 0.0 for r in want], np.float32)
        radii[:] = np.median(radii)
        c.update(want=want, allow=allow, radii=radii, visited=[r["counters"][0] + 1 for r in want])
    elif family == "range_more":
        radii = _exact_mth(base, queries, 400)
        radii[FLOOD_AT] = FLT_MAX
        want = [rm.replay(orc, view, q, ef, radii[i], MAX_FRONTIER, ones, 0) for i, q in enumerate(queries)]
        c.update(want=want, radii=radii, visited=[r["visited"] for r in want])
    elif family == "range_sq8":
        want = [rq.replay(orc, view, quant, ORDER, q, ef, ones, 0) for q in queries]
        radii = np.array([rq.mth_exact(orc, base, 0, q, r["pairs"], 17) for q, r in zip(queries, want)], np.float32)
        code_radii = np.array([rq.code_radius(r, INF) for r in radii], np.float32)
        c.update(want=want, radii=radii, code_radii=code_radii, visited=[r["counters"][0] + 1 for r in want])
    else:
        raise KeyError(family)
    _cases[key] = c
    return c


def bitset_ids(c):
    """Per query, a lower bound on the ids that reach the bitset: the rows it marks, less what the 64-slot first
    level and the spill table can hold."""
    return [v - (1 << HASH_LOG2) - c["table"] for v in c["visited"]]


def check_inputs(c, dirty_cap=3):
    """The conditions without which a clean read-back shows nothing: every query spills, and every query sets
    more bitset words than a `dirty_cap`-word list holds.  Fails (never skips) with the figures."""
    low = min(c["visited"])
    assert low > FILL_LIMIT, f"vacuous: a {c['family']} query marks {low} rows, no more than the first level's fill limit {FILL_LIMIT}"
    low = min(bitset_ids(c))
    assert low > 32 * dirty_cap, (f"vacuous: a {c['family']} query sends as few as {low} ids to the bitset, which can fit "
                                  f"{dirty_cap} words: its dirty list need not overflow")
    if c["family"] == "range_more":
        assert c["want"][FLOOD_AT]["visited"] > N * 9 // 10, "vacuous: the FLT_MAX query does not flood the graph"
        assert max(r["more_dist"] for i, r in enumerate(c["want"]) if i != FLOOD_AT) > 0, "vacuous: phase 2 never runs"


def in_order(c, order):
    """The case's per-query fields in the order of a batch (an index array)."""
    return [c["want"][i] for i in order]
