"""ShardedIndex.filtered_search on the device: two ranks on cuda:0 over gloo (tests/filter_shard_worker.py),
this process opens no GPU.  Every rank gets the same global masks, packs its own row range
(sharded.shard_allow_words), runs its shard's filtered search -- f32 rows, or SQ8 codes plus the rerank -- and
the ranks merge with exchange_and_merge.

Parity is per shard: each shard's answer equals the restatement of the filtered search of
that shard under its slice of the mask, and the merged result equals merge_reference over the per-shard
restatements, ids and distance bits, on every rank.  Two masks through ``groups``: a share of 0.1 (both shards
contribute) and one that allows six rows of shard 0 and nothing in shard 1 (merged rows end in empty slots)."""

import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NQ, K, EF = 16, 10, 40


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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "filter_shard_worker.py"), str(tmp_path),
                                       str(n), str(dim), str(NQ), str(K), str(EF), str(seed), mode], env=env))
    try:
        rcs = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * world, rcs
    return [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]


@pytest.mark.parametrize("mode,n,dim,seed", [("f32", 4000, 64, 5), ("sq8", 4000, 128, 21)])
def test_sharded_filtered_search_two_ranks(tmp_path, mode, n, dim, seed):
    from alayalite_amd.sharded import EMPTY, merge_reference

    parts = _run_ranks(tmp_path, n, dim, seed, mode)
    flt_max = np.finfo(np.float32).max
    for p in parts:  # each shard's own answer is the restatement's, local ids
        assert np.array_equal(p["local_ids"].view(np.uint32), p["shard_ids"]), int(p["lo"])
        assert np.array_equal(p["local_d"].view(np.uint32), p["shard_d"].view(np.uint32)), int(p["lo"])
    ref_i, ref_d = merge_reference([p["shard_ids"] for p in parts], [p["shard_d"] for p in parts],
                                   [int(p["lo"]) for p in parts], K)
    for p in parts:  # every rank holds the same merged result
        got_i = p["merged_ids"].astype(np.int64) & 0xFFFFFFFF
        assert np.array_equal(got_i, ref_i)
        assert np.array_equal(p["merged_d"].view(np.uint32), ref_d.view(np.uint32))
    groups = parts[0]["groups"]
    lo1 = int(parts[1]["lo"])
    first = ref_i[groups == 0]
    assert (first != EMPTY).all()
    assert (first >= lo1).any() and (first < lo1).any()  # both shards contribute under the first mask
    second, second_d = ref_i[groups == 1], ref_d[groups == 1]
    real = second != EMPTY
    assert (parts[1]["shard_ids"][groups == 1] == EMPTY).all()  # shard 1 allows nothing
    assert (second[real] < lo1).all() and (real.sum(1) <= 6).all() and real.any()
    for row, d in zip(real, second_d):  # real rows first, then (EMPTY, FLT_MAX) to the end
        cnt = int(row.sum())
        assert row[:cnt].all() and not row[cnt:].any() and (d[cnt:] == flt_max).all()
