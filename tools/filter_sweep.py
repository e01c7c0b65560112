"""Filtered graph search on a GIST-shaped device-built index: rate and recall per allowed share.

usage: python tools/filter_sweep.py [--leg sweep|filtered|plain] [--n 1000000] [--nq 1000] [--ef 387]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("sweep", "filtered", "plain"), default="sweep")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--ef", type=int, default=387)
    ap.add_argument("--shares", default="1,0.5,0.1,0.01")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
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
