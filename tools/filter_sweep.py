"""Filtered graph search on a GIST-shaped device-built index: rate and recall per allowed share.

usage: python tools/filter_sweep.py [--leg sweep|filtered|plain|sq8|sq8-ab|exact|through] [--n 1000000] [--nq 1000] [--ef 387]
                                    [--shares 1,0.5,0.1,0.01] [--reps 20] [--out FILE]

  sweep     per share of allowed rows: queries/s of DeviceIndex.filtered_search_device, recall@10 of its
            answer against the exact top-10 over the allowed rows (calc_gt_device on base[allow], ids
            mapped back), and for comparison the recall@10 of post-filtering the ef ids of the plain
            search at the same ef.
  filtered  the all-ones filtered launch alone, then the plain search of the same process: their times
            (for A/B against `plain`).
  plain     the plain search (k = 10) alone: its time.  With ALAYA_AB_ROOT=<a saved build of the package>
            this runs another build's kernel -- the parent commit's, which has no filtered search -- on
            the same rows, graph (the device build is deterministic) and queries.
  sq8       the config-5 shape (768-d IP text-like unit-sphere rows, SQ8 codes + f32 rerank, device-built
            graph; --n 1000000 --dim 768 are this leg's defaults): ef is the smallest of --ef-ladder at
            which batch search (SQ8 + reference rerank) reaches recall@10 0.95 (--ef N skips the ladder),
            then per share and per candidate pool m in k, 4k, 224: queries/s of
            DeviceIndex.filtered_search_sq8_device, the search stage's ms (ALAYA_FILTER_RERANK=0), the
            rerank's ms (the difference), recall@10 over the allowed rows against the exact IP top-10 on
            base[allow], and the recall of post-filtering batch_search's ef ids.
  sq8-ab    the all-ones filtered SQ8 launch, search stage only, against search_sq8(rerank = 0) of the
            same process with ALAYA_HELPERS=0 (the plain mode-0 kernel the filtered one is built from):
            --rounds alternated rounds of --reps launches each; medians and spreads.
  exact     the exact filtered scan (DeviceIndex.flat_search_filtered_device: compaction, scan and merge
            together, one mask per batch) alternated with the graph filtered search in one process,
            --rounds rounds of --reps launches each after 3 warm-ups, per share of 0.001 .. 1: medians
            and spreads, whether the ids and distance bits equal calc_gt_device(base[rows]) mapped through
            rows, the graph search's recall, the scan's plan and achieved f32 rate; first the unmasked
            flat search's time, last the two crossover shares.  --space sq8 runs config 5's shape
            (768-d IP, SQ8 codes) against filtered_search_sq8_device at m = k, ef 200; --dim 128 the
            narrow L2 shape.
  through   the through search (DeviceIndex.filtered_search_hop_device: the traversal that steps through
            disallowed neighbours) alternated with the plain filtered search and the exact filtered scan in
            one process, --rounds rounds of --reps launches each after 3 warm-ups, per share of 1 .. 0.01:
            medians and spreads, distances and rows stepped through per query, recall@10 over the allowed
            rows against calc_gt_device(base[rows]) -- at --ef, and at the smallest ef of --hop-ladder that
            reaches recall 0.95, where one does -- and which of the three calls is the fastest that reaches
            0.95.  At share 1 the through / plain ratio is the all-ones launch's cost.
Every leg prints one JSON line per measurement; --out appends them to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if os.environ.get("ALAYA_AB_ROOT"):
    sys.path.insert(0, os.environ["ALAYA_AB_ROOT"])

K = 10


def recall(ids, gt):
    hits = sum(len(set(int(v) for v in ids[i] if v != 0xFFFFFFFF) & set(int(v) for v in gt[i] if v >= 0))
               for i in range(len(gt)))
    return hits / float(sum(int((gt[i] >= 0).sum()) for i in range(len(gt))) or 1)


def sq8_legs(args):
    import torch
    from alayalite_amd import _native
    from alayalite_amd.utils import calc_gt_device, pack_allow
    from workloads.datasets import text_like

    ext = _native._ext
    st = torch.cuda.current_stream()
    n, nq = args.n, args.nq
    base, queries = text_like(n, nq, dim=args.dim)
    print(f"rows {base.shape}", file=sys.stderr, flush=True)
    dev = ext.DeviceIndex(0)
    dev.set_base(base, 1)
    dev.build_graph(32, 100, 100, 0, 0, 2)
    print("graph built", file=sys.stderr, flush=True)
    mn, mx = ext.sq8_train(base)
    dev.set_sq8(ext.sq8_encode(base, mn, mx, 16), mn, mx, ext.host_sq8_order())
    print("codes set", file=sys.stderr, flush=True)
    qd = torch.from_numpy(np.ascontiguousarray(queries)).cuda()
    ids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    dd = torch.empty((nq, K), dtype=torch.float32, device="cuda")
    cnt = torch.empty((nq, 4), dtype=torch.int32, device="cuda")

    def emit(rec):
        rec.update(n=n, nq=nq, dim=args.dim, k=K, metric="ip", sq8_order=int(ext.host_sq8_order()))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def timed(run, reps=args.reps):
        for _ in range(3):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            run()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def batch(ef, rerank, out=ids, k=K):
        dev.search_sq8_device(qd.data_ptr(), 0, nq, k, ef, rerank, out.data_ptr(), dd.data_ptr() if k == K else 0,
                              cnt.data_ptr(), st.cuda_stream)

    def stage_only(on):
        if on:
            os.environ["ALAYA_FILTER_RERANK"] = "0"
        else:
            os.environ.pop("ALAYA_FILTER_RERANK", None)

    ones = torch.from_numpy(pack_allow(np.ones(n, bool), n).view(np.int32)).cuda()

    def filtered(ef, m, words):
        dev.filtered_search_sq8_device(qd.data_ptr(), 0, nq, K, ef, m, words.data_ptr(), 1, 0, ids.data_ptr(), dd.data_ptr(),
                                       cnt.data_ptr(), st.cuda_stream)

    if args.leg == "sq8-ab":
        ef = args.ef or 340
        os.environ["ALAYA_HELPERS"] = "0"
        plain_ms, filt_ms = [], []
        for _ in range(args.rounds):  # alternated in one process: same rows, graph, queries and clocks
            plain_ms.append(timed(lambda: batch(ef, 0)))
            plan_plain = dev.last_plan()
            stage_only(True)
            filt_ms.append(timed(lambda: filtered(ef, K, ones)))
            stage_only(False)
            plan_filt = dev.last_plan()
        med_p, med_f = float(np.median(plain_ms)), float(np.median(filt_ms))
        emit(dict(leg="sq8-ab", ef=ef, pool=K, plain_ms=sorted(plain_ms), filtered_ms=sorted(filt_ms), plain_median=med_p,
                  filtered_median=med_f, ratio=med_f / med_p, plain_spread=(max(plain_ms) - min(plain_ms)) / med_p,
                  plain_plan={k: int(v) for k, v in plan_plain.items()}, filtered_plan={k: int(v) for k, v in plan_filt.items()}))
        return

    gt_all, _ = calc_gt_device(base, queries, K, metric="ip")
    ef = args.ef
    if not ef:  # the shape's recall-0.95 point of batch_search (SQ8 search + reference rerank)
        for ef in [int(s) for s in args.ef_ladder.split(",")]:
            batch(ef, 1)
            torch.cuda.synchronize()
            r = recall(ids.cpu().numpy().view(np.uint32), gt_all)
            emit(dict(leg="sq8-ladder", ef=ef, recall_at_10=r))
            if r >= 0.95:
                break
    wide = torch.empty((nq, ef), dtype=torch.int32, device="cuda")  # batch search's whole pool by code distance
    batch(ef, 0, wide, ef)
    torch.cuda.synchronize()
    pool_ids = wide.cpu().numpy().view(np.uint32)
    ms_plain = timed(lambda: batch(ef, 1))
    emit(dict(leg="sq8-batch", ef=ef, ms=ms_plain, qps=nq / ms_plain * 1e3, plan={k: int(v) for k, v in dev.last_plan().items()}))
    for share in [float(s) for s in args.shares.split(",")]:
        allow = np.ones(n, bool) if share >= 1.0 else np.random.default_rng(100 + round(1000 * share)).random(n) < share
        words = torch.from_numpy(pack_allow(allow, n).view(np.int32)).cuda()
        rows = np.flatnonzero(allow)
        gt_local, _ = calc_gt_device(base[rows], queries, K, metric="ip")
        gt = np.where(gt_local >= 0, rows[np.clip(gt_local, 0, len(rows) - 1)], -1)
        post = np.full((nq, K), 0xFFFFFFFF, np.uint32)
        kept = []
        for i in range(nq):
            keep = pool_ids[i][allow[pool_ids[i]]][:K]
            post[i, :len(keep)] = keep
            kept.append(len(keep))
        for m in (K, 4 * K, 224):
            ms = timed(lambda: filtered(ef, m, words))
            got = ids.cpu().numpy().view(np.uint32)
            n_dist = float(cnt.cpu().numpy()[:, 0].mean())
            groups, waves = dev.last_launch()
            stage_only(True)
            ms_search = timed(lambda: filtered(ef, m, words))
            stage_only(False)
            emit(dict(leg="sq8", share=share, allowed=int(allow.sum()), ef=ef, pool=m, ms=ms, qps=nq / ms * 1e3,
                      search_ms=ms_search, rerank_ms=ms - ms_search, recall_at_10=recall(got, gt),
                      results_per_query=float((got != 0xFFFFFFFF).sum(1).mean()), post_filter_recall_at_10=recall(post, gt),
                      post_filter_results_per_query=float(np.mean(kept)), workgroups=groups, waves=waves, n_dist=n_dist))


def exact_leg(args):
    """The exact filtered scan against the graph filtered search, alternated in one process."""
    import torch
    from alayalite_amd import _native
    from alayalite_amd.utils import calc_gt_device, pack_allow
    from workloads.datasets import gist_like, text_like

    ext = _native._ext
    st = torch.cuda.current_stream()
    n, nq, ef, sq8 = args.n, args.nq, args.ef, args.space == "sq8"
    metric = "ip" if sq8 else "l2"
    base, queries = (text_like if sq8 else gist_like)(n, nq, dim=args.dim)
    dev = ext.DeviceIndex(0)
    dev.set_base(base, 1 if sq8 else 0)
    dev.build_graph(32, 100, 100, 0, 0, 2)
    if sq8:
        mn, mx = ext.sq8_train(base)
        dev.set_sq8(ext.sq8_encode(base, mn, mx, 16), mn, mx, ext.host_sq8_order())
    print("index ready", file=sys.stderr, flush=True)
    qd = torch.from_numpy(np.ascontiguousarray(queries)).cuda()
    ids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    dd = torch.empty((nq, K), dtype=torch.float32, device="cuda")
    gids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    gdd = torch.empty((nq, K), dtype=torch.float32, device="cuda")
    cnt = torch.empty((nq, 4), dtype=torch.int32, device="cuda")
    flags = torch.empty((nq,), dtype=torch.int32, device="cuda")

    def emit(rec):
        rec.update(n=n, nq=nq, dim=args.dim, k=K, ef=ef, metric=metric, space=args.space)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

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

    def flat():
        dev.flat_search_device(qd.data_ptr(), nq, K, ids.data_ptr(), dd.data_ptr(), flags.data_ptr(), st.cuda_stream)

    flat_ms = sorted(timed(flat) for _ in range(args.rounds))
    emit(dict(leg="exact-unmasked", ms=flat_ms, median=float(np.median(flat_ms)), qps=nq / float(np.median(flat_ms)) * 1e3,
              flagged=int(flags.cpu().numpy().sum())))
    table = []
    for share in [float(s) for s in args.shares.split(",")]:
        allow = np.ones(n, bool) if share >= 1.0 else np.random.default_rng(100 + round(1000 * share)).random(n) < share
        words = torch.from_numpy(pack_allow(allow, n).view(np.int32)).cuda()
        rows = np.flatnonzero(allow)

        def exact():
            dev.flat_search_filtered_device(qd.data_ptr(), nq, K, words.data_ptr(), 1, 0, ids.data_ptr(), dd.data_ptr(),
                                            st.cuda_stream)

        def graph():
            if sq8:
                dev.filtered_search_sq8_device(qd.data_ptr(), 0, nq, K, ef, K, words.data_ptr(), 1, 0, gids.data_ptr(),
                                               gdd.data_ptr(), cnt.data_ptr(), st.cuda_stream)
            else:
                dev.filtered_search_device(qd.data_ptr(), nq, K, ef, words.data_ptr(), 1, 0, gids.data_ptr(), gdd.data_ptr(),
                                           cnt.data_ptr(), st.cuda_stream)

        exact_ms, graph_ms = [], []
        for _ in range(args.rounds):  # alternated: same rows, graph, queries and clocks
            exact_ms.append(timed(exact))
            graph_ms.append(timed(graph))
        last = [int(v) for v in dev.flat_filtered_last()]
        got = ids.cpu().numpy().view(np.uint32)
        got_d = dd.cpu().numpy()
        ggot = gids.cpu().numpy().view(np.uint32)
        gt_local, gt_d = calc_gt_device(base[rows], queries, K, metric=metric)
        gt = np.where(gt_local >= 0, rows[np.clip(gt_local, 0, len(rows) - 1)], -1)
        want = np.where(gt >= 0, gt, 0xFFFFFFFF).astype(np.uint32)
        med_e, med_g = float(np.median(exact_ms)), float(np.median(graph_ms))
        rec = dict(leg="exact", share=share, allowed=int(allow.sum()), exact_ms=sorted(exact_ms), graph_ms=sorted(graph_ms),
                   exact_median=med_e, graph_median=med_g, exact_spread=(max(exact_ms) - min(exact_ms)) / med_e,
                   graph_spread=(max(graph_ms) - min(graph_ms)) / med_g, exact_qps=nq / med_e * 1e3,
                   ids_equal_ground_truth=bool(np.array_equal(got, want)),
                   distance_bits_equal_ground_truth=bool(np.array_equal(got_d.view(np.uint32), gt_d.view(np.uint32))),
                   graph_recall_at_10=recall(ggot, gt), allowed_valid=last[0], row_chunks=last[1], query_tile=last[2],
                   scan_launches=last[3],
                   # two f32 operations per element of every (query, allowed row) pair, over the whole call
                   achieved_tflops=2.0 * nq * float(allow.sum()) * args.dim / (med_e * 1e-3) / 1e12,
                   exact_below_graph_median=med_e < med_g, every_exact_below_every_graph=max(exact_ms) < min(graph_ms))
        emit(rec)
        table.append((share, med_e, med_g))

    def crossover(against):
        """The share at which the exact scan's median passes `against` (linear between sweep points)."""
        for (s0, e0, g0), (s1, e1, g1) in zip(table, table[1:]):
            a0, a1 = against(g0), against(g1)
            if (e0 - a0) <= 0 < (e1 - a1):
                t = (a0 - e0) / ((e1 - a1) - (e0 - a0))
                return s0 + t * (s1 - s0)
        return None

    table.sort()
    emit(dict(leg="exact-crossover", against_graph_share=crossover(lambda g: g),
              against_unmasked_exact_share=crossover(lambda g: float(np.median(flat_ms)))))


def through_leg(args):
    """The through search against the plain filtered search and the exact filtered scan, alternated."""
    import torch
    from alayalite_amd import _native
    from alayalite_amd.utils import calc_gt_device, pack_allow
    from workloads.datasets import gist_like

    ext = _native._ext
    st = torch.cuda.current_stream()
    n, nq, ef = args.n, args.nq, args.ef
    base, queries = gist_like(n, nq, dim=args.dim)
    dev = ext.DeviceIndex(0)
    dev.set_base(base, 0)
    dev.build_graph(32, 100, 100, 0, 0, 2)
    print("index ready", file=sys.stderr, flush=True)
    qd = torch.from_numpy(np.ascontiguousarray(queries)).cuda()
    ids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    dd = torch.empty((nq, K), dtype=torch.float32, device="cuda")
    pids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    eids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    cnt = torch.empty((nq, 4), dtype=torch.int32, device="cuda")
    pcnt = torch.empty((nq, 4), dtype=torch.int32, device="cuda")
    thr = torch.empty((nq,), dtype=torch.int32, device="cuda")

    def emit(rec):
        rec.update(n=n, nq=nq, dim=args.dim, k=K, metric="l2")
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def timed(run, reps):
        for _ in range(3):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            run()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def stats(ms):
        med = float(np.median(ms))
        return dict(ms=sorted(ms), median=med, spread=(max(ms) - min(ms)) / med, qps=nq / med * 1e3)

    for share in [float(s) for s in args.shares.split(",")]:
        allow = np.ones(n, bool) if share >= 1.0 else np.random.default_rng(100 + round(1000 * share)).random(n) < share
        words = torch.from_numpy(pack_allow(allow, n).view(np.int32)).cuda()
        rows = np.flatnonzero(allow)
        gt_local, _ = calc_gt_device(base[rows], queries, K)
        gt = np.where(gt_local >= 0, rows[np.clip(gt_local, 0, len(rows) - 1)], -1)

        def through(e=ef):
            dev.filtered_search_hop_device(qd.data_ptr(), nq, K, e, words.data_ptr(), 1, 0, ids.data_ptr(), dd.data_ptr(),
                                           cnt.data_ptr(), thr.data_ptr(), st.cuda_stream)

        def plain():
            dev.filtered_search_device(qd.data_ptr(), nq, K, ef, words.data_ptr(), 1, 0, pids.data_ptr(), dd.data_ptr(),
                                       pcnt.data_ptr(), st.cuda_stream)

        def exact():
            dev.flat_search_filtered_device(qd.data_ptr(), nq, K, words.data_ptr(), 1, 0, eids.data_ptr(), dd.data_ptr(),
                                            st.cuda_stream)

        def measured():
            torch.cuda.synchronize()
            return (recall(ids.cpu().numpy().view(np.uint32), gt), float(cnt.cpu().numpy()[:, 0].mean()),
                    float(cnt.cpu().numpy()[:, 1].mean()), float(thr.cpu().numpy().mean()))

        # the exact scan costs allowed rows x queries: fewer launches per round at the large shares
        exact_reps = max(2, min(args.reps, int(args.reps * 0.05 / share)))
        t_ms, p_ms, e_ms = [], [], []
        for _ in range(args.rounds):  # alternated: same rows, graph, queries and clocks
            t_ms.append(timed(through, args.reps))
            p_ms.append(timed(plain, args.reps))
            e_ms.append(timed(exact, exact_reps))
        through()
        t_recall, t_dist, t_pops, t_rows = measured()
        plan_t = {k: int(v) for k, v in dev.last_plan().items()}
        plain()
        torch.cuda.synchronize()
        plan_p = {k: int(v) for k, v in dev.last_plan().items()}
        p_recall = recall(pids.cpu().numpy().view(np.uint32), gt)
        rec = dict(leg="through", share=share, allowed=int(allow.sum()), ef=ef, through=stats(t_ms), plain=stats(p_ms),
                   exact=stats(e_ms), through_recall_at_10=t_recall, plain_recall_at_10=p_recall,
                   exact_recall_at_10=recall(eids.cpu().numpy().view(np.uint32), gt), through_n_dist=t_dist,
                   through_pops=t_pops, through_rows=t_rows, plain_n_dist=float(pcnt.cpu().numpy()[:, 0].mean()),
                   through_over_plain=float(np.median(t_ms)) / float(np.median(p_ms)), through_plan=plan_t, plain_plan=plan_p)
        # the smallest ef of the ladder at which the through search reaches recall 0.95
        small = None
        for e in [int(v) for v in args.hop_ladder.split(",")]:
            if e >= ef:
                break
            through(e)
            r, nd, pops, nr = measured()
            if r >= 0.95:
                ms = [timed(lambda: through(e), args.reps) for _ in range(args.rounds)]
                small = dict(ef=e, recall_at_10=r, n_dist=nd, pops=pops, rows=nr, **stats(ms))
                break
        rec["through_smallest_ef_at_0.95"] = small
        calls = {"exact": float(np.median(e_ms))}
        if p_recall >= 0.95:
            calls["plain"] = float(np.median(p_ms))
        if small is not None:
            calls["through"] = small["median"]
        elif t_recall >= 0.95:
            calls["through"] = float(np.median(t_ms))
        rec["fastest_call_at_0.95"] = min(calls, key=calls.get)
        emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("sweep", "filtered", "plain", "sq8", "sq8-ab", "exact", "through"), default="sweep")
    ap.add_argument("--space", choices=("f32", "sq8"), default="f32",
                    help="exact leg: f32 = GIST-shaped L2 rows; sq8 = config 5's text-like IP rows with SQ8 codes")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=0, help="0 = 960 (768 for the sq8 legs)")
    ap.add_argument("--ef", type=int, default=0, help="0 = 387 (the sq8 legs: found on --ef-ladder)")
    ap.add_argument("--ef-ladder", default="40,60,80,100,120,160,200,260,340,440")
    ap.add_argument("--shares", default="", help="default 1,0.5,0.1,0.01 (exact leg: 0.001,0.01,0.05,0.1,0.2,0.5,1)")
    ap.add_argument("--hop-ladder", default="10,16,24,32,48,64,96,128,192,256", help="through leg: the short ef sweep")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.leg == "exact":
        args.shares = args.shares or "0.001,0.01,0.05,0.1,0.2,0.5,1"
        args.dim = args.dim or (768 if args.space == "sq8" else 960)
        args.ef = args.ef or (200 if args.space == "sq8" else 387)
        return exact_leg(args)
    if args.leg == "through":
        args.shares = args.shares or "1,0.5,0.2,0.1,0.05,0.02,0.01"
        args.dim = args.dim or 960
        args.ef = args.ef or 387
        return through_leg(args)
    args.shares = args.shares or "1,0.5,0.1,0.01"
    if args.leg in ("sq8", "sq8-ab"):
        args.dim = args.dim or 768
        return sq8_legs(args)
    args.dim = args.dim or 960
    args.ef = args.ef or 387
    import torch
    from alayalite_amd import _native
    from workloads.datasets import gist_like

    ext = _native._ext
    st = torch.cuda.current_stream()
    base, queries = gist_like(args.n, args.nq, dim=args.dim)
    dev = ext.DeviceIndex(0)
    dev.set_base(base, 0)
    dev.build_graph(32, 100, 100, 0, 0, 2)
    nq, ef = args.nq, args.ef
    qd = torch.from_numpy(np.ascontiguousarray(queries)).cuda()
    ids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    dd = torch.empty((nq, K), dtype=torch.float32, device="cuda")
    cnt = torch.empty((nq, 4), dtype=torch.int32, device="cuda")

    def emit(rec):
        rec.update(n=args.n, nq=nq, dim=args.dim, k=K, ef=ef, build="saved" if os.environ.get("ALAYA_AB_ROOT") else "tree")
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

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

    def plain():
        dev.search_device(qd.data_ptr(), nq, K, ef, ids.data_ptr(), dd.data_ptr(), cnt.data_ptr(), st.cuda_stream)

    if args.leg == "plain":
        ms = timed(plain)
        groups, waves = dev.last_launch()
        emit(dict(leg="plain", ms=ms, qps=nq / ms * 1e3, workgroups=groups, waves=waves,
                  n_dist=float(cnt.cpu().numpy()[:, 0].mean())))
        return

    from alayalite_amd.utils import calc_gt_device, pack_allow

    shares = [1.0] if args.leg == "filtered" else [float(s) for s in args.shares.split(",")]
    pool_ids = None
    for share in shares:
        allow = np.ones(args.n, bool) if share >= 1.0 else np.random.default_rng(100 + round(1000 * share)).random(args.n) < share
        words = torch.from_numpy(pack_allow(allow, args.n).view(np.int32)).cuda()

        def filtered():
            dev.filtered_search_device(qd.data_ptr(), nq, K, ef, words.data_ptr(), 1, 0, ids.data_ptr(), dd.data_ptr(),
                                       cnt.data_ptr(), st.cuda_stream)

        ms = timed(filtered)
        groups, waves = dev.last_launch()
        rec = dict(leg="filtered", share=share, allowed=int(allow.sum()), ms=ms, qps=nq / ms * 1e3, workgroups=groups,
                   waves=waves, n_dist=float(cnt.cpu().numpy()[:, 0].mean()))
        if args.leg == "sweep":
            got = ids.cpu().numpy().view(np.uint32)
            rows = np.flatnonzero(allow)
            gt_local, _ = calc_gt_device(base[rows], queries, K)
            gt = np.where(gt_local >= 0, rows[np.clip(gt_local, 0, len(rows) - 1)], -1)
            if pool_ids is None:  # the plain search's whole pool, once: k = ef
                wide = torch.empty((nq, ef), dtype=torch.int32, device="cuda")
                dev.search_device(qd.data_ptr(), nq, ef, ef, wide.data_ptr(), 0, 0, st.cuda_stream)
                torch.cuda.synchronize()
                pool_ids = wide.cpu().numpy().view(np.uint32)
            post = np.full((nq, K), 0xFFFFFFFF, np.uint32)
            kept = []
            for i in range(nq):
                keep = pool_ids[i][allow[pool_ids[i]]][:K]
                post[i, :len(keep)] = keep
                kept.append(len(keep))
            rec.update(recall_at_10=recall(got, gt), post_filter_recall_at_10=recall(post, gt),
                       post_filter_results_per_query=float(np.mean(kept)),
                       results_per_query=float((got != 0xFFFFFFFF).sum(1).mean()))
        emit(rec)
    ms = timed(plain)  # the same process's plain search, as the environment plans it
    groups, waves = dev.last_launch()
    emit(dict(leg="plain", ms=ms, qps=nq / ms * 1e3, workgroups=groups, waves=waves))


if __name__ == "__main__":
    main()
