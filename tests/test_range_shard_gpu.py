"""ShardedIndex.range_search on the device: two ranks on cuda:0 over gloo (tests/range_shard_worker.py), this
process opens no GPU.  Every rank gets the same global masks and radii, packs its own row range
(sharded.shard_allow_words), runs its shard's range search -- f32 rows, or SQ8 codes with a slack plus the exact
rerank -- and the ranks merge with exchange_and_merge; one small all-gather carries the per-shard counts.

Parity is per shard: each shard's answer equals the restatement of the range search of that shard under its
slice of the mask, the merged rows equal merge_reference over the per-shard restatements at k = max_results, ids
and distance bits, on every rank, and counts is the sum.  ``truncated`` is checked once with a cap above every
shard's list (all false) and once with a cap below one shard's (true exactly where a shard dropped rows or the
shards' rows together exceed the cap)."""

import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NQ, EF = 15, 40
CAP_HI, CAP_LO = 512, 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_ranks(tmp_path, n, dim, seed, mode, world=2):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "range_shard_worker.py"), str(tmp_path),
                                       str(n), str(dim), str(NQ), str(EF), str(seed), mode, str(CAP_HI), str(CAP_LO)],
                                      env=env))
    try:
        rcs = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * world, rcs
    return [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("mode,n,dim,seed", [("f32", 4000, 64, 5), ("sq8", 4000, 128, 21)])
def test_sharded_range_search_two_ranks(tmp_path, mode, n, dim, seed):
    from alayalite_amd.sharded import EMPTY, merge_reference

    parts = _run_ranks(tmp_path, n, dim, seed, mode)
    flt_max = np.finfo(np.float32).max
    seen = {}
    for cap in (CAP_HI, CAP_LO):
        t = f"_{cap}"
        for p in parts:  # each shard's own answer is the restatement's, local ids
            lo = int(p["lo"])
            assert np.array_equal(p["local_ids" + t].view(np.uint32), p["shard_ids" + t]), (cap, lo)
            assert np.array_equal(p["local_d" + t].view(np.uint32), p["shard_d" + t].view(np.uint32)), (cap, lo)
            assert np.array_equal(p["local_n" + t].view(np.uint32), p["shard_n" + t]), (cap, lo)
            assert np.array_equal(p["local_cand" + t].view(np.uint32), p["shard_cand" + t]), (cap, lo)
            assert np.array_equal(p["local_counters" + t].view(np.uint32), p["shard_counters"]), (cap, lo)
        ref_i, ref_d = merge_reference([p["shard_ids" + t] for p in parts], [p["shard_d" + t] for p in parts],
                                       [int(p["lo"]) for p in parts], cap)
        total = sum(p["shard_n" + t] for p in parts)
        rows = sum(np.minimum(p["shard_n" + t], cap) for p in parts)  # what the shards returned together
        dropped = np.any([p["shard_cand" + t] > cap for p in parts], axis=0)
        want_trunc = dropped | (rows > cap)
        for p in parts:  # every rank holds the same merged result
            got_i = p["merged_ids" + t].astype(np.int64) & 0xFFFFFFFF
            assert np.array_equal(got_i, ref_i), cap
            assert np.array_equal(p["merged_d" + t].view(np.uint32), ref_d.view(np.uint32)), cap
            assert np.array_equal(p["counts" + t], total), cap
            assert np.array_equal(p["truncated" + t], want_trunc), (cap, p["truncated" + t], want_trunc)
        for i in np.flatnonzero(~want_trunc):  # the whole union, first counts[i] slots filled, then empty
            c = int(total[i])
            assert (ref_i[i, :c] != EMPTY).all() and (ref_i[i, c:] == EMPTY).all() and (ref_d[i, c:] == flt_max).all()
        seen[cap] = (want_trunc, total, ref_i)
    assert not seen[CAP_HI][0].any()  # a cap above every shard's list
    assert max(int(p["shard_cand" + f"_{CAP_HI}"].max()) for p in parts) <= CAP_HI
    assert seen[CAP_LO][0].any() and not seen[CAP_LO][0].all()  # a cap below one shard's
    assert any((p["shard_cand" + f"_{CAP_LO}"] > CAP_LO).any() for p in parts)
    lo1 = int(parts[1]["lo"])
    both = seen[CAP_HI][2]
    assert ((both != EMPTY) & (both >= lo1)).any() and (both < lo1).any()  # both shards contribute
    assert (seen[CAP_HI][1] > CAP_LO).any() and (seen[CAP_HI][1] <= CAP_LO).any()
