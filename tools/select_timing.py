"""Times the selection search (DeviceIndex.flat_select_search_device, k = 1000) beside the flat search at its own
limit (flat_search_device, k = 224) on one MI355X: device events around each call, R alternated rounds after a
warm-up of both, medians and the spread.  Writes one JSON line per shape.

    python tools/select_timing.py --n 1000000 --dims 128 960 --nq 1000 --k 1000 --rounds 5 --out profiles/r27/timing.jsonl
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 960])
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("select_timing needs a GPU")
    from alayalite_amd import _native

    d0 = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(d0)
    lines = []
    for dim in a.dims:
        rng = np.random.default_rng(dim)
        base = rng.standard_normal((a.n, dim), dtype=np.float32)
        q = rng.standard_normal((a.nq, dim), dtype=np.float32)
        dev = _native._ext.DeviceIndex(0)
        dev.set_base(base, 0)
        qd = torch.from_numpy(q).to(d0)
        ids = torch.zeros((a.nq, a.k), dtype=torch.int32, device=d0)
        dd = torch.zeros((a.nq, a.k), dtype=torch.float32, device=d0)
        flags = torch.zeros((a.nq,), dtype=torch.int32, device=d0)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def select():
            return dev.flat_select_search_device(qd.data_ptr(), a.nq, a.k, ids.data_ptr(), dd.data_ptr(), stream.cuda_stream)

        def flat224():
            dev.flat_search_device(qd.data_ptr(), a.nq, 224, ids.data_ptr(), dd.data_ptr(), flags.data_ptr(), stream.cuda_stream)

        for _ in range(2):  # warm-up: code objects, the buffers, the flat search's tile records
            select()
            flat224()
        torch.cuda.synchronize()
        t_sel, t_flat = [], []
        for _ in range(a.rounds):
            t_sel.append(timed(select))
            t_flat.append(timed(flat224))
        passes, verified, redo = dev.flat_select_last()
        line = {"n": a.n, "dim": dim, "nq": a.nq, "k": a.k, "rounds": a.rounds,
                "select_ms_median": float(np.median(t_sel)), "select_ms_min": min(t_sel), "select_ms_max": max(t_sel),
                "flat224_ms_median": float(np.median(t_flat)), "flat224_ms_min": min(t_flat), "flat224_ms_max": max(t_flat),
                "full_passes": int(passes), "verified_pairs_per_query": verified / a.nq, "redo": int(redo)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del dev
    if a.out:
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
