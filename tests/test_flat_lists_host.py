"""The lists scan's launch plan without a GPU (alaya_flat_lists_plan, pure host arithmetic): the pieces cover the
entries, the piece table bounds the pieces of any lists of that total, the partial lists stay under the cap, and a
forced piece is honoured."""

import itertools

import pytest

import flat_filtered_common as fc

TOTALS = [0, 1, 63, 10 ** 4, 10 ** 6, 10 ** 8, 10 ** 10]
NQ = [1, 37, 1000, 10 ** 6]
KS = [1, 10, 224]
STRIDES = [32, 128, 960]
CUS = 256
PASS = 8  # candidates one wave takes per pass


@pytest.mark.parametrize("forced", [None, 8, 64, 100, 512])
def test_plan_conditions(native, monkeypatch, forced):
    if forced is None:
        monkeypatch.delenv("ALAYA_FLAT_LISTS_PIECE", raising=False)
    else:
        monkeypatch.setenv("ALAYA_FLAT_LISTS_PIECE", str(forced))
    split = 0
    for total, nq, k, stride in itertools.product(TOTALS, NQ, KS, STRIDES):
        piece, table, sub, part, launches = plan = native.flat_lists_plan(total, nq, k, stride, CUS)
        what = (total, nq, k, stride, plan)
        assert piece > 0 and piece % PASS == 0, what
        assert 1 <= sub <= nq and launches == -(-nq // sub), what
        # the table bound: sub lists whose lengths sum to at most total have sum(ceil(len / piece)) <=
        # total // piece + sub pieces; and the pieces cover the entries even when one list holds them all
        assert table == total // piece + sub and -(-total // piece) <= table, what
        assert part == table * k * 8 and 4 * (stride * 4 + k * 8) <= 160 * 1024, what
        split += launches > 1
        if forced is None:
            assert part <= fc.CAP and 64 <= piece, what
            assert piece <= 1024 or total * k * 8 > (piece - PASS) * (fc.CAP // 2), what  # longer only for the cap
        else:
            assert piece == -(-forced // PASS) * PASS, what
    assert forced is not None or split > 0  # the grid reaches batches that have to be split


def test_plan_rejects_bad_arguments(native, monkeypatch):
    monkeypatch.delenv("ALAYA_FLAT_LISTS_PIECE", raising=False)
    for k in (0, 225):
        with pytest.raises(ValueError):
            native.flat_lists_plan(100, 10, k, 128, CUS)
    with pytest.raises(ValueError):  # four queries of such rows do not fit a CU's LDS
        native.flat_lists_plan(100, 10, 10, 1 << 14, CUS)
