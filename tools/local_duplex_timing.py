"""Timing of local hybridization (Context.local_duplex) on the GPU: a query against every window of a long target.

  python tools/local_duplex_timing.py [--out FILE.json] [--n 5000,20000] [--steps 1,20] [--window 200] [--query 100] [--whole-pair-n 5000]

Per (source, n, W, S), the median and the range of --repeat runs behind one warm-up run (which allocates and captures the launch
graphs): wall time of local_duplex plus the fetch of hp and log Z; device time of the chunks' computes and of the accumulate +
finish kernels (rh_local_times: the band kernels of the windowed molecule and the hp kernels together); the bytes those kernels must
move, computed from the shapes -- for hp every entry of every window once, hp_loc written once by the accumulate kernel, read and
written once more by the finish kernel; for the band what tools/local_fold_timing.py counts -- and the rate that gives.  DESIGN.md
section 5 records a copy bandwidth of 5.2 TB/s on this GPU.  Where the whole pair still fits (the duplex sources, n = --whole-pair-n)
the time of Context.duplex on the whole pair stands beside it, for orientation."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ractip_amd                      # noqa: E402
from ractip_amd import hot             # noqa: E402

COPY_TBS = 5.2


def windows(n, W, S):
    if n <= W:
        return [0]
    m = -(-(n - W) // S)
    return [k * S for k in range(m)] + [n - W]


def band_bytes(n, W, S, max_w):
    We, nw = min(W, n), len(windows(n, W, S))
    per_window = We * (We - 1) // 2 + sum(min(max_w, We - a) for a in range(We))
    return 8 * (nw * per_window + 3 * n * (We + max_w))


def hp_bytes(nq, n, W, S):
    We, nw = min(W, n), len(windows(n, W, S))
    return 8 * (nw * nq * We + 3 * (nq + 1) * (n + 1))


def spread(values):
    """[median, min, max]"""
    v = sorted(values)
    return [v[len(v) // 2], v[0], v[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", default="5000,20000")
    ap.add_argument("--steps", default="1,20")
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--query", type=int, default=100)
    ap.add_argument("--whole-pair-n", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sources", default="contrafold-duplex,vienna-duplex,vienna-cofold")
    args = ap.parse_args()
    W, nq = args.window, args.query
    query = "".join(np.random.RandomState(nq).choice(list("ACGU"), nq))
    rows = []
    for name in args.sources.split(","):
        c = ractip_amd.Context(device=0, model=hot.RH_MODEL_CONTRAFOLD if name.startswith("contrafold") else hot.RH_MODEL_VIENNA_BL)
        if name.startswith("vienna"):
            c.set_hybrid(name == "vienna-cofold")
        max_w = c.max_w
        for n in [int(x) for x in args.n.split(",")]:
            target = "".join(np.random.RandomState(n).choice(list("ACGU"), n))
            for S in [int(x) for x in args.steps.split(",")]:
                runs = []
                for _ in range(1 + args.repeat):
                    t0 = time.perf_counter()
                    hp, logz, starts = c.local_duplex(query, target, W, S)
                    wall = time.perf_counter() - t0
                    runs.append((1e3 * wall,) + c.local_times())
                wall_ms, compute_ms, acc_ms = (spread(col) for col in zip(*runs[1:]))
                nbytes = hp_bytes(nq, n, W, S) + band_bytes(n, W, S, max_w)
                row = dict(source=name, query=nq, n=n, W=W, S=S, windows=len(starts), max_w=max_w, wall_ms=wall_ms, compute_ms=compute_ms,
                           accumulate_ms=acc_ms, hp_bytes=hp_bytes(nq, n, W, S), band_bytes=band_bytes(n, W, S, max_w),
                           accumulate_TBs=nbytes / (acc_ms[0] * 1e-3) / 1e12, copy_TBs=COPY_TBS, result_bytes=8 * (hp.size + logz.size),
                           path=c.last_path(), hybrid_path=c.last_hybrid_path())
                if n == args.whole_pair_n and name != "vienna-cofold":
                    whole = []
                    for _ in range(1 + min(3, args.repeat)):
                        t0 = time.perf_counter()
                        c.duplex(query, target)
                        whole.append(1e3 * (time.perf_counter() - t0))
                    row["whole_pair_duplex_ms"] = spread(whole[1:])
                rows.append(row)
                print(json.dumps(row), flush=True)
        c.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
