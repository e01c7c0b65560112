"""One rank of the sharded filtered-search GPU test (tests/test_filter_shard_gpu.py), started as a child
process: every rank runs on cuda:0 with a gloo group, as tests/shard_worker.py does.

The rank builds its shard (mode "f32": 64-d L2 rows; mode "sq8": 128-d unit-sphere rows, IP, its own SQ8
space), runs ShardedIndex.filtered_search with the global masks -- two masks chosen per query through
``groups``: a share of 0.1 of all rows, and one that allows six rows of shard 0 and none of shard 1 -- and
writes the merged result, its own shard's answer, and the restatement of the filtered search of its own shard
under the shard's slice of each mask (filter_common.replay / filter_sq8_common.replay), local ids.

argv: out_dir n dim nq k ef seed mode
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def masks(n, seed):
    """(2, n) bool: a share of 0.1, and six rows of the first half only."""
    rng = np.random.default_rng(seed + 1)
    allow = np.zeros((2, n), bool)
    allow[0] = rng.random(n) < 0.1
    allow[1, rng.choice((n + 1) // 2, 6, replace=False)] = True
    return allow


def main():
    out_dir, n, dim, nq, k, ef, seed = sys.argv[1], *map(int, sys.argv[2:8])
    mode = sys.argv[8]
    import torch
    import torch.distributed as dist

    import filter_common as fc
    import filter_sq8_common as sc
    import oracle
    from alayalite_amd.sharded import ShardedIndex
    from shard_worker import _data

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    base, queries = _data(mode, n, dim, nq, seed)
    metric = 1 if mode == "sq8" else 0
    allow = masks(n, seed)
    groups = (np.arange(nq) % 2).astype(np.int64)

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    shard = ShardedIndex(base, world, rank, device=0, metric=metric, num_threads=4, sq8=(mode == "sq8"))
    q_dev = torch.from_numpy(queries).to(dev)
    stream = torch.cuda.current_stream(dev)
    ids, dists = shard.filtered_search(q_dev, k, ef, allow, stream.cuda_stream, groups=groups)
    torch.cuda.synchronize()
    local_ids, local_d, _ = shard.last_local

    oracle.build()
    l0, levels, off, ue, ep, upper_r, _ = shard.graph.arrays()
    view = oracle.IndexView(shard.rows, l0, levels, off, ue, upper_r, ep, metric=metric)
    mine = allow[:, shard.lo:shard.hi]
    o_ids = np.zeros((nq, k), np.uint32)
    o_d = np.zeros((nq, k), np.float32)
    for i in range(nq):
        if mode == "sq8":
            codes, mn, mx, order = shard.sq8
            r = sc.replay(oracle, view, (mn, mx, codes), order, queries[i], k, ef, sc.default_pool(k, ef), mine[groups[i]],
                          metric)
        else:
            r = fc.replay(oracle, view, queries[i], k, ef, mine[groups[i]], metric)
        o_ids[i], o_d[i] = r["ids"], r["dists"]
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), merged_ids=ids.cpu().numpy(), merged_d=dists.cpu().numpy(),
             local_ids=local_ids.cpu().numpy(), local_d=local_d.cpu().numpy(), shard_ids=o_ids, shard_d=o_d,
             lo=shard.lo, hi=shard.hi, groups=groups)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
