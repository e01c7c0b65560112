"""The MFMA filtered scan's launch plan (alaya_flat_filtered_mfma_plan), pure host arithmetic."""

import pytest

import flat_filtered_common as fc


@pytest.mark.parametrize("n,nq,k", [(1, 1, 1), (5000, 17, 224), (10 ** 6, 1000, 10), (10 ** 7, 10000, 224)])
def test_plan(native, n, nq, k):
    rows, chunks, tile, sub, part = plan = native.flat_filtered_mfma_plan(n, nq, k, 256)
    assert tile == 128 and rows % 128 == 0 and rows >= max(1024, 32 * k), plan
    assert chunks * rows >= n and (chunks - 1) * rows < n, plan  # the chunks cover n, none is empty
    assert sub % 128 == 0 and sub > 0 and part == chunks * min(nq, sub) * k * 8 and part <= fc.CAP, plan
    # no more chunks than fill the CUs twice over for the query groups in flight
    assert chunks <= max(1, 2 * 256 // (min(sub, -(-nq // 128) * 128) // 128)), plan
