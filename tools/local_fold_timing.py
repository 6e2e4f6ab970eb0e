"""Timing of local folding (Context.local_fold) on the GPU, next to the route a caller had before it: the same windows uploaded as
indexed batches in chunks, every table fetched (batch_results_all) and averaged in numpy.

  python tools/local_fold_timing.py [--out FILE.json] [--n 5000,20000] [--steps 1,20] [--window 200] [--old-route-n 5000]

Per (model, n, W, S), the median and the range of --repeat runs behind one warm-up run (which allocates and captures the launch
graphs): wall time of local_fold plus the
fetch of band, up and log Z; device time of the folds and of the accumulate + finish kernels (rh_local_times); the bytes those
kernels must move -- every table entry of every window once, the band and up written by the accumulate kernel, read and written
by the finish kernel -- and the rate that gives.  DESIGN.md section 5 records a copy bandwidth of 5.2 TB/s on this GPU
(profiles/pmc_calibration.json holds the counter factors it was measured with)."""
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


def accumulate_bytes(n, W, S, max_w):
    We, nw = min(W, n), len(windows(n, W, S))
    per_window = We * (We - 1) // 2 + sum(min(max_w, We - a) for a in range(We))
    return 8 * (nw * per_window + 3 * n * (We + max_w))


def spread(values):
    """[median, min, max]"""
    v = sorted(values)
    return [v[len(v) // 2], v[0], v[-1]]


def old_route(c, seq, W, S, chunk=512):
    """indexed uploads of the windows in chunks, all tables over the bus, numpy average in increasing window order"""
    n, We, starts, max_w = len(seq), min(W, len(seq)), windows(len(seq), W, S), c.max_w
    a, d, w = np.arange(We)[:, None], np.arange(We)[None, :], np.arange(max_w)[None, :]
    in_bp, in_up = (d >= 1) & (a + d < We), a + w < We
    idx = np.where(in_bp, (a + 1) * (2 * (We + 1) - (a + 1) - 1) // 2 + a + 1 + d, 0)   # entry 0 of a triangular table holds 0
    band, cb = np.zeros((n, We)), np.zeros((n, We))
    up, cu = np.zeros((n, max_w)), np.zeros((n, max_w))
    moved = 0
    for k0 in range(0, len(starts), chunk):
        part = starts[k0:k0 + chunk]
        c.batch_upload_indexed([seq[s:s + We] for s in part], [(0, 0)])
        c.batch_compute()
        r = c.batch_results_all()
        moved += 8 * len(part) * (((hot.tri_size(We) + 1) & ~1) + ((We + 3) & ~1) * max_w)   # the padded device layout (rh_batch_layout)
        for s, bp_k, up_k in zip(part, r["bp"], r["up"]):
            band[s:s + We] += bp_k[idx]
            cb[s:s + We] += in_bp
            up[s:s + We] += np.where(in_up, np.asarray(up_k).reshape(We, max_w), 0.0)
            cu[s:s + We] += in_up
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cb > 0, band / cb, 0.0), np.where(cu > 0, up / cu, 0.0), moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", default="5000,20000")
    ap.add_argument("--steps", default="1,20")
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--old-route-n", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    W = args.window
    rows = []
    for model, name in ((hot.RH_MODEL_CONTRAFOLD, "contrafold"), (hot.RH_MODEL_VIENNA_BL, "vienna-bl")):
        c = ractip_amd.Context(device=0, model=model)
        max_w = c.max_w
        for n in [int(x) for x in args.n.split(",")]:
            seq = "".join(np.random.RandomState(n).choice(list("ACGU"), n))
            for S in [int(x) for x in args.steps.split(",")]:
                runs = []
                for _ in range(1 + args.repeat):
                    t0 = time.perf_counter()
                    band, up, logz, starts = c.local_fold(seq, W, S)
                    wall = time.perf_counter() - t0
                    runs.append((1e3 * wall,) + c.local_times())
                wall_ms, fold_ms, acc_ms = (spread(col) for col in zip(*runs[1:]))
                nbytes = accumulate_bytes(n, W, S, max_w)
                row = dict(model=name, n=n, W=W, S=S, windows=len(starts), max_w=max_w, wall_ms=wall_ms, fold_ms=fold_ms, accumulate_ms=acc_ms,
                           accumulate_bytes=nbytes, accumulate_TBs=nbytes / (acc_ms[0] * 1e-3) / 1e12, copy_TBs=COPY_TBS,
                           result_bytes=8 * (band.size + up.size + logz.size), path=c.last_path())
                if n == args.old_route_n:
                    old = []
                    for _ in range(1 + min(3, args.repeat)):
                        t0 = time.perf_counter()
                        oband, oup, moved = old_route(c, seq, W, S)
                        old.append(1e3 * (time.perf_counter() - t0))
                    row["old_route_ms"] = spread(old[1:])
                    row["old_route_bytes_fetched"] = moved
                    row["old_route_same_bits"] = bool(np.array_equal(oband, band) and np.array_equal(oup, up))
                rows.append(row)
                print(json.dumps(row), flush=True)
        c.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
