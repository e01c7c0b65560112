"""Which graph-search kernel a request gets (csrc/search_variants.h), on the CPU.

The kernels are listed once, as (space, chunks, mode, metrics) rows; ``resolve_search_variant``
picks one per launch and the launch is planned from the one it picked.  ``native.search_variant``
evaluates that choice on the host and ``native.search_variants`` returns the list.

tests/golden/search_variants.json is the choice of the hand-written if-ladder the list replaced,
recorded from that ladder (not from the list) for every request below: 8 dims x {L2, IP} x 3 spaces
x {float order, generic order} x the 32 sets of wanted features = 3,072 requests, in that nesting
order."""

import itertools
import json
import os

import pytest

STAMP, CHECK, HELP, TWO_WAVES, SCREEN = 1, 2, 4, 8, 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_variants.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["axes"] == ["dim", "ip", "sq8_order", "generic", "wanted_mode_bits"]
    assert g["dims"] == [100, 64, 128, 256, 512, 768, 960, 1024]
    requests = list(itertools.product(g["dims"], (False, True), (0, 1, 2), (False, True), range(32)))
    assert len(requests) == len(g["chosen_space_chunks_mode"]) == 3072
    return requests, [tuple(c) for c in g["chosen_space_chunks_mode"]]


@pytest.fixture(scope="module")
def chosen(native, golden):
    return [native.search_variant(*r)[0] for r in golden[0]]


def test_selection_is_the_ladders(golden, chosen):
    requests, want = golden
    wrong = [(r, c, w) for r, c, w in zip(requests, chosen, want) if tuple(c) != w]
    assert not wrong, f"{len(wrong)} of {len(requests)} requests; first (request, chosen, golden): {wrong[0]}"


def test_never_more_than_asked(golden, chosen):
    for (dim, ip, order, generic, wanted), (space, chunks, mode) in zip(golden[0], chosen):
        assert mode & ~wanted == 0, ((dim, ip, order, generic, wanted), mode)
        assert space == order and chunks in (0, dim // 32)


def test_chosen_variants_are_rows_of_the_list(native, golden, chosen):
    rows = native.search_variants()
    assert len(rows) == len(set(rows)) == 37
    assert {r[:3] for r in rows} == set(chosen), "a listed kernel that no request reaches, or the reverse"
    for (_, ip, *_), c in zip(golden[0], chosen):
        assert not (ip and (*c, True) in rows), "an L2-only kernel chosen for IP"


def test_predicates_match_the_list(native, golden):
    rows = native.search_variants()
    for dim, ip, order, generic in sorted({r[:4] for r in golden[0]}):
        chunks = 0 if generic or dim % 32 else dim // 32
        want = 0
        for bit in (HELP, TWO_WAVES, SCREEN):
            if any(s == order and c == chunks and m & bit and not (l2_only and ip) for s, c, m, l2_only in rows):
                want |= bit
        assert native.search_variant(dim, ip, order, generic, 0)[1] == want, (dim, ip, order, generic)
