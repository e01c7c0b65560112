"""One rank of the sharded range-search GPU test (tests/test_range_shard_gpu.py), started as a child process:
every rank runs on cuda:0 with a gloo group, as tests/filter_shard_worker.py does.

The rank builds its shard (mode "f32": 64-d L2 rows; mode "sq8": 128-d unit-sphere rows, IP, its own SQ8 space)
and runs ShardedIndex.range_search with the global masks -- two masks chosen per query through ``groups``: a
share of 0.5 of all rows, and every row -- once per cap.  The radius of query i is its exact m-th neighbour
distance over the whole base, m = 3, 20 or 60 by turns, computed the same way on every rank; SQ8 shards get a
slack of 0.01.  It writes, per cap, the merged result, its own shard's answer and the restatement of the range
search of its own shard under the shard's slice of each mask (range_common / range_sq8_common), local ids.

argv: out_dir n dim nq ef seed mode cap [cap ...]
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLACK = 0.01


def masks(n, seed):
    """(2, n) bool: a share of 0.5, and every row."""
    rng = np.random.default_rng(seed + 1)
    allow = np.ones((2, n), bool)
    allow[0] = rng.random(n) < 0.5
    return allow


def radii_of(base, queries, metric):
    """Query i's exact m-th neighbour distance in float64, rounded to float32; m = 3, 20, 60 by turns."""
    b, q = base.astype(np.float64), queries.astype(np.float64)
    d = -(q @ b.T) if metric else ((q[:, None, :] - b[None, :, :]) ** 2).sum(2)
    d.sort(axis=1)
    return np.array([d[i, (3, 20, 60)[i % 3] - 1] for i in range(len(queries))], np.float32)


def main():
    out_dir, n, dim, nq, ef, seed = sys.argv[1], *map(int, sys.argv[2:7])
    mode = sys.argv[7]
    caps = [int(c) for c in sys.argv[8:]]
    import torch
    import torch.distributed as dist

    import filter_common as fc
    import oracle
    import range_common as rc
    import range_sq8_common as rq
    from alayalite_amd.sharded import ShardedIndex
    from shard_worker import _data

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    base, queries = _data(mode, n, dim, nq, seed)
    sq8 = mode == "sq8"
    metric = 1 if sq8 else 0
    allow = masks(n, seed)
    groups = (np.arange(nq) % 2).astype(np.int64)
    radii = radii_of(base, queries, metric)

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    shard = ShardedIndex(base, world, rank, device=0, metric=metric, num_threads=4, sq8=sq8)
    q_dev = torch.from_numpy(queries).to(dev)
    stream = torch.cuda.current_stream(dev)

    oracle.build()
    l0, levels, off, ue, ep, upper_r, _ = shard.graph.arrays()
    view = oracle.IndexView(shard.rows, l0, levels, off, ue, upper_r, ep, metric=metric)
    mine = allow[:, shard.lo:shard.hi]
    if sq8:
        codes, mn, mx, order = shard.sq8
        rs = [rq.replay(oracle, view, (mn, mx, codes), order, queries[i], ef, mine[groups[i]], metric) for i in range(nq)]
    else:
        rs = [fc.replay(oracle, view, queries[i], rc.K, ef, mine[groups[i]], metric) for i in range(nq)]

    out = dict(lo=shard.lo, hi=shard.hi, groups=groups, radii=radii)
    for cap in caps:
        ids, d, counts, truncated = shard.range_search(q_dev, radii, ef, cap, stream.cuda_stream, allow=allow, groups=groups,
                                                       slack=SLACK if sq8 else None)
        torch.cuda.synchronize()
        local_ids, local_d, local_c, local_n, local_cand = shard.last_local
        o_ids = np.zeros((nq, cap), np.uint32)
        o_d = np.zeros((nq, cap), np.float32)
        o_n = np.zeros(nq, np.int64)
        o_cand = np.zeros(nq, np.int64)  # f32 shards: the count itself
        for i, r in enumerate(rs):
            if sq8:
                o_n[i], o_cand[i], o_ids[i], o_d[i] = rq.want_row(oracle, shard.rows, metric, queries[i], r["pairs"], radii[i],
                                                                  rq.code_radius(radii[i], SLACK), cap)
            else:
                o_n[i], o_ids[i], o_d[i] = rc.want_row(r, radii[i], cap)
                o_cand[i] = o_n[i]
        tag = f"_{cap}"
        out.update({
            "merged_ids" + tag: ids.cpu().numpy(), "merged_d" + tag: d.cpu().numpy(), "counts" + tag: counts.cpu().numpy(),
            "truncated" + tag: truncated.cpu().numpy(), "local_ids" + tag: local_ids.cpu().numpy(),
            "local_d" + tag: local_d.cpu().numpy(), "local_n" + tag: local_n.cpu().numpy(),
            "local_counters" + tag: local_c.cpu().numpy(),
            "local_cand" + tag: (local_n if local_cand is None else local_cand).cpu().numpy(),
            "shard_ids" + tag: o_ids, "shard_d" + tag: o_d, "shard_n" + tag: o_n, "shard_cand" + tag: o_cand,
        })
    out["shard_counters"] = np.array([r["counters"] for r in rs], np.int64)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
