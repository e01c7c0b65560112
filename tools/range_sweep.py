"""Range search on a GIST-shaped device-built index: recall, counts and the two launches' times per radius.

usage: python tools/range_sweep.py [--n 1000000] [--nq 1000] [--dim 960] [--ef 387] [--reps 10] [--rounds 5] [--out FILE]

Radii: per query, the exact m-th neighbour distance of the flat search's top 224 (exact_search's answer), for
m in 1, 10, 50, 200, at max_results 1024 -- so the ground truth, the rows of that answer with d <= r, is exact;
a query whose 224th distance is <= r has no complete ground truth and is left out (reported; none expected).
One more leg runs radius FLT_MAX at max_results 4096: every measured row is appended, the worst append traffic;
the same radius at max_results 1 counts the same hits and stores one row, which separates the stores' time from
the counting's.

Per leg: range recall (hits returned / ground-truth rows, over the queries kept), mean and maximum count,
truncated queries, and the time of DeviceIndex.range_search_device split into the search launch
(ALAYA_RANGE_SORT=0) and the sort (the difference).  The same process alternates the range launches with the
all-ones filtered_search_device launch (k 10) and search_device under ALAYA_SEARCH_SCREEN=0 -- the plain
kernel the other two are built from -- --rounds rounds of --reps launches each after 3 warm-ups: medians, with
the spread (max - min) / median of each.  One JSON line per measurement; --out appends them to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 10
GT = 224
FLT_MAX = float(np.finfo(np.float32).max)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--ef", type=int, default=387)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from alayalite_amd import _native
    from alayalite_amd.utils import pack_allow
    from workloads.datasets import gist_like

    ext = _native._ext
    st = torch.cuda.current_stream()
    n, nq, ef = args.n, args.nq, args.ef
    base, queries = gist_like(n, nq, dim=args.dim)
    dev = ext.DeviceIndex(0)
    dev.set_base(base, 0)
    dev.build_graph(32, 100, 100, 0, 0, 2)
    print("index ready", file=sys.stderr, flush=True)
    gt_ids, gt_d, _ = dev.flat_search(queries, GT)

    def emit(rec):
        rec.update(n=n, nq=nq, dim=args.dim, ef=ef)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    qd = torch.from_numpy(np.ascontiguousarray(queries)).cuda()
    ones = torch.from_numpy(pack_allow(np.ones(n, bool), n).view(np.int32)).cuda()
    k_ids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    k_d = torch.empty((nq, K), dtype=torch.float32, device="cuda")
    cnt = torch.empty((nq, 4), dtype=torch.int32, device="cuda")
    counts = torch.empty((nq,), dtype=torch.int32, device="cuda")

    def timed(run):
        for _ in range(3):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.reps):
            run()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def env(name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value

    def plain():
        dev.search_device(qd.data_ptr(), nq, K, ef, k_ids.data_ptr(), k_d.data_ptr(), cnt.data_ptr(), st.cuda_stream)

    def filtered():
        dev.filtered_search_device(qd.data_ptr(), nq, K, ef, ones.data_ptr(), 1, 0, k_ids.data_ptr(), k_d.data_ptr(),
                                   cnt.data_ptr(), st.cuda_stream)

    legs = [(f"m={m}", np.ascontiguousarray(gt_d[:, m - 1]), 1024) for m in (1, 10, 50, 200)]
    legs.append(("FLT_MAX", np.full(nq, FLT_MAX, np.float32), 4096))
    legs.append(("FLT_MAX, counted only", np.full(nq, FLT_MAX, np.float32), 1))  # the same hits, one row stored
    bufs = {}
    for name, radii, cap in legs:
        bufs[name] = (torch.from_numpy(radii).cuda(), torch.empty((nq, cap), dtype=torch.int32, device="cuda"),
                      torch.empty((nq, cap), dtype=torch.float32, device="cuda"))

    def ranged(name, cap):
        r, ids, d = bufs[name]
        dev.range_search_device(qd.data_ptr(), nq, ef, r.data_ptr(), cap, 0, 0, 0, counts.data_ptr(), ids.data_ptr(),
                                d.data_ptr(), cnt.data_ptr(), st.cuda_stream)

    # ---- answers ------------------------------------------------------------------------------------
    for name, radii, cap in legs:
        ranged(name, cap)
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(np.uint32)
        rec = dict(leg="answer", radius=name, max_results=cap, mean_count=float(c.mean()), max_count=int(c.max()),
                   truncated=int((c > cap).sum()), n_dist=float(cnt.cpu().numpy()[:, 0].mean()),
                   plan={k: int(v) for k, v in dev.last_plan().items()})
        if name.startswith("m="):
            got = bufs[name][1].cpu().numpy().view(np.uint32)
            keep = gt_d[:, GT - 1] > radii  # the ground truth is complete
            found = truth = 0
            for i in np.flatnonzero(keep):
                want = set(int(v) for v in gt_ids[i][gt_d[i] <= radii[i]])
                truth += len(want)
                found += len(want & set(int(v) for v in got[i][:min(int(c[i]), cap)]))
            rec.update(left_out=int((~keep).sum()), truth_rows=truth, recall=found / float(truth or 1))
        emit(rec)

    # ---- times: alternated in one process, same rows, graph, queries and clocks ----------------------
    ms = {"plain": [], "filtered": []}
    for name, _, _ in legs:
        ms[name] = []
        ms[name + " search"] = []
    for _ in range(args.rounds):
        env("ALAYA_SEARCH_SCREEN", "0")
        ms["plain"].append(timed(plain))
        env("ALAYA_SEARCH_SCREEN", None)
        ms["filtered"].append(timed(filtered))
        for name, _, cap in legs:
            ms[name].append(timed(lambda: ranged(name, cap)))
            env("ALAYA_RANGE_SORT", "0")
            ms[name + " search"].append(timed(lambda: ranged(name, cap)))
            env("ALAYA_RANGE_SORT", None)

    def stat(v):
        med = float(np.median(v))
        return dict(median_ms=med, spread=(max(v) - min(v)) / med, ms=sorted(v))

    emit(dict(leg="time", what="plain", **stat(ms["plain"])))
    filt = stat(ms["filtered"])
    emit(dict(leg="time", what="filtered", **filt))
    for name, _, cap in legs:
        total, search = stat(ms[name]), stat(ms[name + " search"])
        emit(dict(leg="time", what="range", radius=name, max_results=cap, total=total, search=search,
                  sort_ms=total["median_ms"] - search["median_ms"],
                  search_over_filtered=search["median_ms"] / filt["median_ms"]))


if __name__ == "__main__":
    main()
