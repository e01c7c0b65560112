"""Range search on a GIST-shaped device-built index: recall, counts and the two launches' times per radius.

usage: python tools/range_sweep.py [--leg fixed|radius|sq8|exact] [--n 1000000] [--nq 1000] [--dim 960] [--ef 387] [--reps 10] [--rounds 5] [--out FILE]

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
queries and radii, [--small-ef 64] [--sweep-efs 500,700,...] [--small-sweep-efs 64,72,...] [--max-frontier 4096].

--leg sq8 measures range search on an SQ8 index (sq8_leg below): filter_sweep.py --leg sq8's index -- config 5's
shape, 768-d IP text-like rows, SQ8 codes, device-built graph; --n 1000000 --dim 768 --ef 200 are this leg's
defaults.

--leg exact measures the exact range scan (exact_leg below): against the exact filtered k-NN with a radius that
admits nothing, its scan, gather and sort per radius and cap, and -- with the exact call as the ground truth, no
query left out -- the range recall of both graph range searches, [--target-rows 1000] [--no-graph]."""
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


def sq8_leg(args):
    """--leg sq8.  The radius is each query's exact m-th neighbour distance (flat search), m = 10, 50, 200, at
    max_results 1024.  Per m: the quantiles (0.5, 0.9, 0.99, max) of d_code - d_exact over the rows inside the
    radius that the traversal measured (the hits of a call with slack inf at max_results 4096; d_code from the
    oracle's code distance of the encoded query and row), then one run per slack -- 0, each quantile, inf --
    with range recall against the exact in-radius set, hits and candidates (mean, max), truncated queries, and
    the search launch (ALAYA_RANGE_SORT=0), the search and rerank (ALAYA_RANGE_SORT=2) and the whole call, every
    launch alternated in this process, medians of --rounds rounds with spreads; the rerank and the sort are the
    differences of those medians (the rerank consumes the search's list, so it cannot be launched alone).
    Then the search stage against search_sq8_device(rerank = 0), the plain mode-0 kernel (ALAYA_HELPERS=0), on
    the same grid: with a code radius that admits nothing, and at m = 200 with the 0.99 slack."""
    import torch

    import oracle
    from alayalite_amd import _native
    from workloads.datasets import text_like

    ext = _native._ext
    oracle.build()
    st = torch.cuda.current_stream()
    n, nq, ef, cap = args.n, args.nq, args.ef, 1024
    base, queries = text_like(n, nq, dim=args.dim)
    print(f"rows {base.shape}", file=sys.stderr, flush=True)
    dev = ext.DeviceIndex(0)
    dev.set_base(base, 1)
    dev.build_graph(32, 100, 100, 0, 0, 2)
    print("graph built", file=sys.stderr, flush=True)
    mn, mx = ext.sq8_train(base)
    codes = ext.sq8_encode(base, mn, mx, 16)
    order = int(ext.host_sq8_order())
    dev.set_sq8(codes, mn, mx, order)
    qcodes = ext.sq8_encode(queries, mn, mx, 16)
    gt_ids, gt_d, _ = dev.flat_search(queries, GT)
    print("ground truth ready", file=sys.stderr, flush=True)

    def emit(rec):
        rec.update(n=n, nq=nq, dim=args.dim, ef=ef, metric="ip", sq8_order=order)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    qd = torch.from_numpy(np.ascontiguousarray(queries)).cuda()
    ids = torch.empty((nq, 4096), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, 4096), dtype=torch.float32, device="cuda")
    cnt = torch.empty((nq, 4), dtype=torch.int32, device="cuda")
    counts = torch.empty((nq,), dtype=torch.int32, device="cuda")
    cand = torch.empty((nq,), dtype=torch.int32, device="cuda")
    k_ids = torch.empty((nq, K), dtype=torch.int32, device="cuda")

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

    def ranged(r_t, c_t, width):
        dev.range_search_sq8_device(qd.data_ptr(), 0, nq, ef, r_t.data_ptr(), c_t.data_ptr(), width, 0, 0, 0,
                                    counts.data_ptr(), cand.data_ptr(), ids.data_ptr(), d.data_ptr(), cnt.data_ptr(),
                                    st.cuda_stream)

    def rows_of(t, width):
        """The nq x width result the last call wrote at the front of a (nq, 4096) buffer."""
        return t.reshape(-1)[:nq * width].reshape(nq, width).cpu().numpy()

    def plain():
        dev.search_sq8_device(qd.data_ptr(), 0, nq, K, ef, 0, k_ids.data_ptr(), 0, cnt.data_ptr(), st.cuda_stream)

    def stat(v):
        med = float(np.median(v))
        return dict(median_ms=med, spread=(max(v) - min(v)) / med, ms=sorted(v))

    runs = []  # (m, slack name, radii tensor, code radii tensor)
    inf_t = torch.full((nq,), float("inf"), dtype=torch.float32, device="cuda")
    for m in (10, 50, 200):
        radii = np.ascontiguousarray(gt_d[:, m - 1])
        r_t = torch.from_numpy(radii).cuda()
        keep = gt_d[:, GT - 1] > radii  # the ground truth is complete
        truth = [set(int(v) for v in gt_ids[i][gt_d[i] <= radii[i]]) for i in range(nq)]
        # the measured rows inside the radius, and how far their code distances sit above the exact ones
        ranged(r_t, inf_t, 4096)
        torch.cuda.synchronize()
        c, cd = counts.cpu().numpy().view(np.uint32), cand.cpu().numpy().view(np.uint32)
        got_i, got_d = rows_of(ids, 4096).view(np.uint32), rows_of(d, 4096)
        gaps = []
        for i in np.flatnonzero(cd <= 4096):
            for v, e in zip(got_i[i][:c[i]], got_d[i][:c[i]]):
                gaps.append(float(np.float32(oracle.sq8_dist(1, qcodes[i], codes[v], mn, mx, order))) - float(e))
        gaps = np.array(gaps)
        qs = {"q50": float(np.quantile(gaps, 0.5)), "q90": float(np.quantile(gaps, 0.9)),
              "q99": float(np.quantile(gaps, 0.99)), "max": float(gaps.max())}
        emit(dict(leg="gap", m=m, rows=len(gaps), queries_left_out=int((cd > 4096).sum()), min=float(gaps.min()), **qs))
        slacks = [("0", 0.0)] + [(k, max(v, 0.0)) for k, v in qs.items()] + [("inf", float("inf"))]
        for name, slack in slacks:
            c_t = torch.from_numpy((radii + np.float32(slack)).astype(np.float32)).cuda()
            ranged(r_t, c_t, cap)
            torch.cuda.synchronize()
            c, cd = counts.cpu().numpy().view(np.uint32), cand.cpu().numpy().view(np.uint32)
            got_i = rows_of(ids, cap).view(np.uint32)
            found = want = 0
            for i in np.flatnonzero(keep):
                want += len(truth[i])
                found += len(truth[i] & set(int(v) for v in got_i[i][:c[i]]))
            emit(dict(leg="answer", m=m, slack=name, slack_value=slack, max_results=cap, recall=found / float(want or 1),
                      truth_rows=want, left_out=int((~keep).sum()), mean_hits=float(c.mean()), max_hits=int(c.max()),
                      mean_cand=float(cd.mean()), max_cand=int(cd.max()), truncated=int((cd > cap).sum()),
                      stored=int(np.minimum(cd, cap).sum()), n_dist=float(cnt.cpu().numpy()[:, 0].mean()),
                      plan={k: int(v) for k, v in dev.last_plan().items()}))
            runs.append((m, name, r_t, c_t))
    none_t = torch.full((nq,), -FLT_MAX, dtype=torch.float32, device="cuda")  # admits no candidate
    q99_200 = next(r for r in runs if r[0] == 200 and r[1] == "q99")

    env("ALAYA_HELPERS", "0")
    ms = {(m, name, stage): [] for m, name, _, _ in runs for stage in ("search", "rerank+", "all")}
    ab = {"plain": [], "range, no candidate": [], "range, m=200 q99": []}
    for _ in range(args.rounds):
        ab["plain"].append(timed(plain))
        plan_plain = dev.last_plan()
        env("ALAYA_RANGE_SORT", "0")
        ab["range, no candidate"].append(timed(lambda: ranged(none_t, none_t, cap)))
        plan_range = dev.last_plan()
        ab["range, m=200 q99"].append(timed(lambda: ranged(q99_200[2], q99_200[3], cap)))
        for m, name, r_t, c_t in runs:
            env("ALAYA_RANGE_SORT", "0")
            ms[(m, name, "search")].append(timed(lambda: ranged(r_t, c_t, cap)))
            env("ALAYA_RANGE_SORT", "2")
            ms[(m, name, "rerank+")].append(timed(lambda: ranged(r_t, c_t, cap)))
            env("ALAYA_RANGE_SORT", None)
            ms[(m, name, "all")].append(timed(lambda: ranged(r_t, c_t, cap)))
    for m, name, _, _ in runs:
        s, r, a = (ms[(m, name, k)] for k in ("search", "rerank+", "all"))
        # the rerank and the sort are differences of launches timed one after the other in the same round
        emit(dict(leg="time", m=m, slack=name, search=stat(s), search_rerank=stat(r), total=stat(a),
                  rerank_ms=float(np.median(r) - np.median(s)), sort_ms=float(np.median(a) - np.median(r)),
                  rerank_rounds=[y - x for x, y in zip(s, r)], sort_rounds=[y - x for x, y in zip(r, a)]))
    p = stat(ab["plain"])
    for what in ("range, no candidate", "range, m=200 q99"):
        v = stat(ab[what])
        emit(dict(leg="ab", what=what, plain=p, range_search=v, ratio=v["median_ms"] / p["median_ms"],
                  plain_plan={k: int(x) for k, x in plan_plain.items()}, range_plan={k: int(x) for k, x in plan_range.items()}))


def exact_leg(args):
    """--leg exact: the exact range scan (DeviceIndex.flat_range_search_device), GIST-shaped rows, squared L2.
    Every launch is timed with device events after 3 warm-ups, --rounds rounds of --reps launches, all the
    launches of a comparison alternated in this process; medians with the spread (max - min) / median.
      scan    a radius that admits nothing (-1) at max_results 1024 against flat_search_filtered_device (k 10) at
              the same mask, shares 0.01, 0.1 and 1: the same loads and FMAs without the k-best lists.
      stores  no mask; radii at each query's exact 10th and 200th neighbour distance and +inf, max_results 1024
              and 4096; the scans alone (ALAYA_FLAT_RANGE_STAGES=1), with the gathers (2) and the whole call:
              gather and sort are differences of medians.
      recall  (skipped with --no-graph) the exact call is the ground truth, no query left out: range recall of
              range_search expand="fixed" and "radius" at ef --small-ef and --ef, max_results 4096, at the m = 200
              radius and at a per-query radius whose exact count is about --target-rows (bisection on counts)."""
    import torch
    from alayalite_amd import _native
    from alayalite_amd.utils import pack_allow
    from workloads.datasets import gist_like

    ext = _native._ext
    st = torch.cuda.current_stream()
    n, nq = args.n, args.nq
    base, queries = gist_like(n, nq, dim=args.dim)
    print("rows ready", file=sys.stderr, flush=True)
    dev = ext.DeviceIndex(0)
    dev.set_base(base, 0)

    def emit(rec):
        rec.update(n=n, nq=nq, dim=args.dim)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def env(name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value

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

    def stat(v):
        med = float(np.median(v))
        return dict(median_ms=med, spread=(max(v) - min(v)) / med, ms=sorted(v))

    qd = torch.from_numpy(np.ascontiguousarray(queries)).cuda()
    counts = torch.empty((nq,), dtype=torch.int32, device="cuda")
    ids = torch.empty((nq, 4096), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, 4096), dtype=torch.float32, device="cuda")
    k_ids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    k_d = torch.empty((nq, K), dtype=torch.float32, device="cuda")

    def ranged(radii_t, cap, words=None):
        dev.flat_range_search_device(qd.data_ptr(), nq, radii_t.data_ptr(), cap, 0 if words is None else words.data_ptr(),
                                     0 if words is None else 1, 0, counts.data_ptr(), ids.data_ptr(), d.data_ptr(),
                                     st.cuda_stream)

    def exact(radii, cap):
        """(counts, ids, dists) of the exact call on the host; ids / dists (nq, cap)."""
        ranged(torch.from_numpy(np.ascontiguousarray(radii, np.float32)).cuda(), cap)
        torch.cuda.synchronize()
        flat = ids.flatten()[:nq * cap].view(nq, cap), d.flatten()[:nq * cap].view(nq, cap)
        return counts.cpu().numpy().view(np.uint32).copy(), flat[0].cpu().numpy().view(np.uint32), flat[1].cpu().numpy()

    # ---- scan: a radius that admits nothing against the exact filtered k-NN ---------------------------
    nothing = torch.full((nq,), -1.0, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(5)
    for share in (0.01, 0.1, 1.0):
        allow = rng.random(n) < share if share < 1 else np.ones(n, bool)
        words = torch.from_numpy(pack_allow(allow, n).view(np.int32)).cuda()

        def knn():
            dev.flat_search_filtered_device(qd.data_ptr(), nq, K, words.data_ptr(), 1, 0, k_ids.data_ptr(), k_d.data_ptr(),
                                            st.cuda_stream)

        ms = {"knn": [], "range": []}
        for _ in range(args.rounds):
            ms["knn"].append(timed(knn))
            ms["range"].append(timed(lambda: ranged(nothing, 1024, words)))
        torch.cuda.synchronize()
        assert int(counts.cpu().numpy().view(np.uint32).max()) == 0
        a, b = stat(ms["knn"]), stat(ms["range"])
        emit(dict(leg="scan", share=share, eligible=int(allow.sum()), knn_k10=a, range_nothing=b,
                  ratio=b["median_ms"] / a["median_ms"], margin=a["spread"],
                  knn_last=[int(v) for v in dev.flat_filtered_last()], range_last=[int(v) for v in dev.flat_range_last()]))

    # ---- stores: scan, gather and sort per radius and cap ---------------------------------------------
    gt_ids, gt_d, _ = dev.flat_search(queries, GT)
    legs = [(f"m={m}", np.ascontiguousarray(gt_d[:, m - 1])) for m in (10, 200)] + [("inf", np.full(nq, np.inf, np.float32))]
    for name, radii in legs:
        radii_t = torch.from_numpy(radii).cuda()
        for cap in (1024, 4096):
            ms = {1: [], 2: [], 3: []}
            for _ in range(args.rounds):
                for stages in (1, 2, 3):
                    env("ALAYA_FLAT_RANGE_STAGES", None if stages == 3 else str(stages))
                    ms[stages].append(timed(lambda: ranged(radii_t, cap)))
            env("ALAYA_FLAT_RANGE_STAGES", None)
            torch.cuda.synchronize()
            c = counts.cpu().numpy().view(np.uint32)
            s1, s2, s3 = stat(ms[1]), stat(ms[2]), stat(ms[3])
            emit(dict(leg="stores", radius=name, max_results=cap, mean_count=float(c.mean()), max_count=int(c.max()),
                      truncated=int((c > cap).sum()), scan=s1, scan_gather=s2, total=s3,
                      gather_ms=s2["median_ms"] - s1["median_ms"], sort_ms=s3["median_ms"] - s2["median_ms"],
                      range_last=[int(v) for v in dev.flat_range_last()]))
    if args.no_graph:
        return

    # ---- recall: the graph range searches against the full ground truth --------------------------------
    dev.build_graph(32, 100, 100, 0, 0, 2)
    print("index ready", file=sys.stderr, flush=True)
    cap, front = 4096, args.max_frontier
    cnt = torch.empty((nq, 4), dtype=torch.int32, device="cuda")
    more = torch.zeros((nq, 2), dtype=torch.int32, device="cuda")
    # per query, a radius whose exact count is about --target-rows: doubled from the 200th distance until
    # the count passes the target, then 24 bisection steps on the exact counts (cap 1: counts are never capped)
    lo = np.ascontiguousarray(gt_d[:, 199]).astype(np.float64)
    hi = lo.copy()
    for _ in range(12):
        short = exact(hi, 1)[0] < args.target_rows
        if not short.any():
            break
        hi[short] *= 2
    for _ in range(24):
        mid = (lo + hi) / 2
        over = exact(mid, 1)[0] >= args.target_rows
        hi[over], lo[~over] = mid[over], mid[~over]
    wide = hi.astype(np.float32)
    for name, radii in (("m=200", np.ascontiguousarray(gt_d[:, 199])), (f"about {args.target_rows} rows", wide)):
        t_counts, t_ids, _ = exact(radii, cap)
        truth = [set(t_ids[i, :min(int(t_counts[i]), cap)].tolist()) for i in range(nq)]
        emit(dict(leg="truth", radius=name, mean_count=float(t_counts.mean()), min_count=int(t_counts.min()),
                  max_count=int(t_counts.max()), truncated=int((t_counts > cap).sum()), left_out=0,
                  radius_min=float(radii.min()), radius_median=float(np.median(radii)), radius_max=float(radii.max())))
        radii_t = torch.from_numpy(radii).cuda()
        for ef in (args.small_ef, args.ef):
            for radius_mode in (False, True):
                more.zero_()
                if radius_mode:
                    dev.range_search_radius_device(qd.data_ptr(), nq, ef, radii_t.data_ptr(), cap, 0, 0, 0, counts.data_ptr(),
                                                   ids.data_ptr(), d.data_ptr(), cnt.data_ptr(), st.cuda_stream, front,
                                                   more.data_ptr())
                else:
                    dev.range_search_device(qd.data_ptr(), nq, ef, radii_t.data_ptr(), cap, 0, 0, 0, counts.data_ptr(),
                                            ids.data_ptr(), d.data_ptr(), cnt.data_ptr(), st.cuda_stream)
                torch.cuda.synchronize()
                c = counts.cpu().numpy().view(np.uint32)
                got = ids.cpu().numpy().view(np.uint32)
                mo = more.cpu().numpy().view(np.uint32)
                found = sum(len(truth[i] & set(got[i, :min(int(c[i]), cap)].tolist())) for i in range(nq))
                emit(dict(leg="recall", radius=name, expand="radius" if radius_mode else "fixed", search_ef=ef,
                          max_results=cap, max_frontier=front if radius_mode else None,
                          recall=found / float(sum(len(t) for t in truth) or 1), truth_rows=sum(len(t) for t in truth),
                          mean_count=float(c.mean()), truncated=int((c > cap).sum()),
                          frontier_cut=int((mo[:, 0] > front).sum()), n_dist=float(cnt.cpu().numpy()[:, 0].mean())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=0, help="0 = 960 (768 for the sq8 leg)")
    ap.add_argument("--ef", type=int, default=0, help="0 = 387 (200 for the sq8 leg)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=("fixed", "radius", "sq8", "exact"), default="fixed")
    ap.add_argument("--target-rows", type=int, default=1000, help="exact leg: rows per query of the wide radius")
    ap.add_argument("--no-graph", action="store_true", help="exact leg: skip the recall part (no graph build)")
    ap.add_argument("--small-ef", type=int, default=64)
    ap.add_argument("--sweep-efs", default="500,700,1000,1400,2000,2800,4000")
    ap.add_argument("--small-sweep-efs", default="64,72,80,96,112,128,160,200,256,320,387")
    ap.add_argument("--max-frontier", type=int, default=4096)
    args = ap.parse_args()
    if args.leg == "sq8":
        args.dim, args.ef = args.dim or 768, args.ef or 200
        return sq8_leg(args)
    args.dim, args.ef = args.dim or 960, args.ef or 387
    if args.leg == "exact":
        return exact_leg(args)

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
