"""Index.add measured: fit(n - add) + add(add) beside fit(n), on a GIST-shaped base.

usage: python tools/add_sweep.py [--n 1000000 --add 100000 --small 1000 --inserts 200 --ef 387] --out FILE

One JSON line per leg:
  insert   `--inserts` timed Index.insert calls on the fit(n - add) index, the first (which hands the
           device its host mirror) apart, and their mean extrapolated to `add` rows -- an extrapolation;
  add      fit(n - add, builder="gpu") then add(add): wall and device ms of both, recall@10 at --ef
           against exact_search of the same index, and whether n - add is a batch boundary of the
           build for n rows (only then the two graphs are the same);
  small    one add of `--small` further rows into the n-row index: the fixed cost of a call;
  onego    fit(n, builder="gpu"): wall and device ms, the same recall.
Wall times include the host's copies of the rows; device ms is the build steps' (stats of the call)."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def recall(idx, queries, ef):
    gt = idx.exact_search(queries.copy(), 10)[0]
    ids = idx.batch_search(queries.copy(), 10, ef)
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / 10 for a, b in zip(ids, gt)]))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--add", type=int, default=100_000)
    ap.add_argument("--small", type=int, default=1000)
    ap.add_argument("--inserts", type=int, default=200)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--ef", type=int, default=387)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    try:  # torch's bundled HIP runtime first (bench.py's order)
        import torch

        torch.cuda.is_available()
    except Exception:
        pass
    import alayalite_amd
    from alayalite_amd import _native
    from workloads.datasets import gist_like

    n, n0 = args.n, args.n - args.add
    base, queries = gist_like(n + args.small, args.nq, dim=args.dim)
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    client = alayalite_amd.Client()

    def fitted(name, rows):
        idx = client.create_index(name, capacity=n + args.small + args.inserts)
        _, wall = timed(lambda: idx.fit(rows, builder="gpu"))
        return idx, wall, idx.native().last_build_device_ms()

    if args.inserts:
        idx, _, _ = fitted("sweep_insert", base[:n0])
        _, first = timed(lambda: idx.insert(base[n0].copy(), 100))
        each = [timed(lambda i=i: idx.insert(base[n0 + 1 + i].copy(), 100))[1] for i in range(args.inserts)]
        emit(leg="insert", n0=n0, calls=args.inserts, first_ms=first, mean_ms=float(np.mean(each)),
             median_ms=float(np.median(each)), extrapolated_ms_for_add=float(np.mean(each)) * args.add,
             extrapolated=True)
        client.delete_index("sweep_insert")
        del idx

    idx, fit_wall, fit_dev = fitted("sweep_add", base[:n0])
    _, add_wall = timed(lambda: idx.add(base[n0:n]))
    add_dev = idx.native().last_build_device_ms()
    levels = idx.native().graph_arrays()[1]
    ends = _native._ext.build_batches(np.ascontiguousarray(levels, np.uint32), 1, 0, 0, 0)
    emit(leg="add", n0=n0, add=args.add, fit_wall_ms=fit_wall, fit_device_ms=fit_dev, add_wall_ms=add_wall,
         add_device_ms=add_dev, n0_is_batch_boundary=bool(n0 in set(ends.tolist())), ef=args.ef,
         recall_at_10=recall(idx, queries, args.ef))
    if args.small:
        _, small_wall = timed(lambda: idx.add(base[n:n + args.small]))
        emit(leg="small", n0=n, add=args.small, add_wall_ms=small_wall, add_device_ms=idx.native().last_build_device_ms())
    client.delete_index("sweep_add")
    del idx

    idx, wall, dev = fitted("sweep_onego", base[:n])
    emit(leg="onego", n=n, fit_wall_ms=wall, fit_device_ms=dev, ef=args.ef, recall_at_10=recall(idx, queries, args.ef))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
