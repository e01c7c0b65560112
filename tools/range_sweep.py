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
the spread (max - min) / median of each.  One JSON line per measurement; --out appends them to a file.

--leg radius measures expand="radius" against expand="fixed" instead (radius_leg below): the same index,
queries and radii, [--small-ef 64] [--sweep-efs 500,700,...] [--small-sweep-efs 64,72,...] [--max-frontier 4096]."""
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


def radius_leg(args, dev, torch, st, qd, gt_ids, gt_d, cnt, counts, emit, timed, env):
    """--leg radius: expand="radius" against expand="fixed".  Per radius m = 1, 10, 50, 200 (max_results 1024,
    --max-frontier): (1) fixed at --ef, (2) radius at --ef, (3) radius at --small-ef, (3f) fixed at --small-ef,
    (4s) fixed at the smallest ef of --small-sweep-efs whose range recall reaches leg 3's, (4) fixed at the
    smallest ef of --sweep-efs whose range recall reaches leg 2's (or none, if none does below the kernel's ef
    limit) -- the honest comparisons.  `answer` lines: range recall, mean and maximum counts / frontier / more_dist, distances
    per query; `time` lines: the search launch alone (ALAYA_RANGE_SORT=0), every launch alternated in this
    process, medians of --rounds rounds.  Then the empty continuation: the radius-mode launch with a radius
    below every distance against the fixed launch (the parent's kernel, instruction for instruction) at the
    same radius."""
    nq, cap, front = args.nq, 1024, args.max_frontier
    ids = torch.empty((nq, cap), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, cap), dtype=torch.float32, device="cuda")
    more = torch.zeros((nq, 2), dtype=torch.int32, device="cuda")

    def run(radii_t, ef, radius_mode):
        if radius_mode:
            dev.range_search_radius_device(qd.data_ptr(), nq, ef, radii_t.data_ptr(), cap, 0, 0, 0, counts.data_ptr(),
                                           ids.data_ptr(), d.data_ptr(), cnt.data_ptr(), st.cuda_stream, front,
                                           more.data_ptr())
        else:
            dev.range_search_device(qd.data_ptr(), nq, ef, radii_t.data_ptr(), cap, 0, 0, 0, counts.data_ptr(),
                                    ids.data_ptr(), d.data_ptr(), cnt.data_ptr(), st.cuda_stream)

    def answer(name, radii, radii_t, ef, radius_mode, leg):
        more.zero_()
        run(radii_t, ef, radius_mode)
        torch.cuda.synchronize()
        c = counts.cpu().numpy().view(np.uint32)
        mo = more.cpu().numpy().view(np.uint32)
        got = ids.cpu().numpy().view(np.uint32)
        keep = gt_d[:, GT - 1] > radii  # the ground truth is complete
        found = truth = 0
        for i in np.flatnonzero(keep):
            want = set(int(v) for v in gt_ids[i][gt_d[i] <= radii[i]])
            truth += len(want)
            found += len(want & set(int(v) for v in got[i][:min(int(c[i]), cap)]))
        rec = dict(leg="answer", what=leg, radius=name, expand="radius" if radius_mode else "fixed", search_ef=ef,
                   max_results=cap, max_frontier=front if radius_mode else None, recall=found / float(truth or 1),
                   truth_rows=truth, left_out=int((~keep).sum()), mean_count=float(c.mean()), max_count=int(c.max()),
                   truncated=int((c > cap).sum()), mean_frontier=float(mo[:, 0].mean()), max_frontier_seen=int(mo[:, 0].max()),
                   frontier_cut=int((mo[:, 0] > front).sum()), mean_more_dist=float(mo[:, 1].mean()),
                   max_more_dist=int(mo[:, 1].max()), n_dist=float(cnt.cpu().numpy()[:, 0].mean()),
                   plan={k: int(v) for k, v in dev.last_plan().items()})
        emit(rec)
        return rec["recall"]

    runs = []  # (label, radii tensor, ef, radius_mode)
    for m in (1, 10, 50, 200):
        name = f"m={m}"
        radii = np.ascontiguousarray(gt_d[:, m - 1])
        radii_t = torch.from_numpy(radii).cuda()
        answer(name, radii, radii_t, args.ef, False, "1 fixed")
        target = answer(name, radii, radii_t, args.ef, True, "2 radius")
        small = answer(name, radii, radii_t, args.small_ef, True, "3 radius, small ef")
        answer(name, radii, radii_t, args.small_ef, False, "3f fixed, small ef")
        runs += [((name, "1 fixed"), radii_t, args.ef, False), ((name, "2 radius"), radii_t, args.ef, True),
                 ((name, "3 radius, small ef"), radii_t, args.small_ef, True),
                 ((name, "3f fixed, small ef"), radii_t, args.small_ef, False)]
        # what leg 3 is worth: the smallest fixed ef between the two that reaches its recall
        for ef in [int(e) for e in args.small_sweep_efs.split(",")]:
            if answer(name, radii, radii_t, ef, False, "4s fixed, swept ef for leg 3") >= small:
                emit(dict(leg="sweep", radius=name, of="3 radius, small ef", target_recall=small, reached_at_ef=ef))
                runs.append(((name, "4s fixed, swept ef for leg 3"), radii_t, ef, False))
                break
        reached = None
        for ef in [int(e) for e in args.sweep_efs.split(",")]:
            try:
                rec = answer(name, radii, radii_t, ef, False, "4 fixed, swept ef")
            except (ValueError, RuntimeError) as err:  # past the kernel's ef limit (LDS)
                emit(dict(leg="answer", what="4 fixed, swept ef", radius=name, search_ef=ef, refused=str(err)))
                break
            if rec >= target:
                reached = ef
                break
        emit(dict(leg="sweep", radius=name, target_recall=target, reached_at_ef=reached))
        if reached is not None:
            runs.append(((name, "4 fixed, swept ef"), radii_t, reached, False))
    below = torch.full((nq,), -1.0, dtype=torch.float32, device="cuda")  # squared L2: below every distance
    runs += [(("below", "fixed"), below, args.ef, False), (("below", "radius"), below, args.ef, True)]

    ms = {label: [] for label, _, _, _ in runs}
    env("ALAYA_RANGE_SORT", "0")
    for _ in range(args.rounds):
        for label, radii_t, ef, radius_mode in runs:
            ms[label].append(timed(lambda: run(radii_t, ef, radius_mode)))
    env("ALAYA_RANGE_SORT", None)
    for label, _, ef, radius_mode in runs:
        v = ms[label]
        med = float(np.median(v))
        emit(dict(leg="time", radius=label[0], what=label[1], expand="radius" if radius_mode else "fixed", search_ef=ef,
                  median_ms=med, spread=(max(v) - min(v)) / med, ms=sorted(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--ef", type=int, default=387)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=("fixed", "radius"), default="fixed")
    ap.add_argument("--small-ef", type=int, default=64)
    ap.add_argument("--sweep-efs", default="500,700,1000,1400,2000,2800,4000")
    ap.add_argument("--small-sweep-efs", default="64,72,80,96,112,128,160,200,256,320,387")
    ap.add_argument("--max-frontier", type=int, default=4096)
    args = ap.parse_args()

    import torch
    from alayalite_amd import _native
    from alayalite_amd.utils import pack_allow
    from workloads.datasets import gist_like

    ext = _native._ext
    st = torch.cuda.current_stream()
    n, nq, ef = args.n, args.nq, args.ef
    base, queries = gist_like(n, nq, dim=args.dim)
    print("rows ready", file=sys.stderr, flush=True)
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

    if args.leg == "radius":
        radius_leg(args, dev, torch, st, qd, gt_ids, gt_d, cnt, counts, emit, timed, env)
        return

    legs = [(f"m={m}", np.ascontiguousarray(gt_d[:, m - 1]), 1024) for m in (1, 10, 50, 200)]
    legs.append(("FLT_MAX",np.full(nq, FLT_MAX, np.float32), 4096))
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
