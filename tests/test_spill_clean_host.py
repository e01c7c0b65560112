"""The inputs of test_spill_clean.py do what its read-back relies on (spill_common.check_inputs), checked on the
restatements alone: every query of every family marks more rows than the 64-slot first level takes before it
spills, and sends more ids to the bitset than fit the three words of an ALAYA_DIRTY_CAP=3 dirty list, so each
query of those runs ends in the whole-bitset wipe; the radius mode's batch has a query that floods the graph
and others whose second phase runs."""

import numpy as np
import pytest

import spill_common as sp

CASES = [(f, 64) for f in sp.FAMILIES] + [("hop", 960), ("range_more", 960)]


@pytest.mark.parametrize("family,dim", CASES)
def test_inputs_spill_and_overflow_a_three_word_dirty_list(orc, family, dim):
    c = sp.case(orc, family, dim)
    assert len(c["want"]) == len(c["queries"]) == sp.NQ
    sp.check_inputs(c, 3)


def test_check_inputs_refuses_a_batch_that_need_not_overflow(orc):
    """The bound is live: the same batch against a dirty list of 4096 words is called vacuous."""
    c = sp.case(orc, "filtered", 64)
    with pytest.raises(AssertionError, match="vacuous"):
        sp.check_inputs(c, 4096)


def test_range_lists_both_fill_and_overflow(orc):
    c = sp.case(orc, "range", 64)
    counts = np.array([len(sp.rc.hits(r, rad)) for r, rad in zip(c["want"], c["radii"])])
    cap = sp.RANGE_CAP["range"]
    assert (counts > cap).any() and (counts <= cap).any() and (counts > 0).any()
