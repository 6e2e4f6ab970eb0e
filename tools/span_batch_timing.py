"""Timing of span folds in batches (Context.span_fold_batch) on the GPU, next to the loop of single calls (rh_span_fold_acc) over the
same sequences on the same context.

  python tools/span_batch_timing.py [--out FILE.json] [--shapes 5000x1,5000x2,5000x8,5000x32,20000x2,20000x8,100000x1,100000x4]
                                    [--span 200] [--max-w 15] [--repeat 5] [--model vienna|contrafold]

Per shape n x K (K random ACGU sequences of n letters), the median and the range of --repeat runs behind one warm-up run (which
allocates).  The batch and the loop run interleaved: in every repetition first the batch, then the K single calls.  Wall time of the
compute calls alone (no fetch); device time of the batch (rh_span_batch_times: sweeps, exterior passes + finish, accessibility
stage) and of the K single calls (rh_span_times + rh_span_acc_times, summed over the loop); the ratios batch / loop; and whether
every item of the batch had the bits of its single call.
--model contrafold: on a CONTRAfold context with its span folds switched on (Context.set_span_contrafold) and, for
--max-w above 1, its region accessibility (Context.set_region_accessibility)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ractip_amd                      # noqa: E402
from ractip_amd import hot             # noqa: E402


def spread(values):
    """[median, min, max]"""
    v = sorted(values)
    return [v[len(v) // 2], v[0], v[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="5000x1,5000x2,5000x8,5000x32,20000x2,20000x8,100000x1,100000x4")
    ap.add_argument("--span", type=int, default=200)
    ap.add_argument("--max-w", type=int, default=15)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--model", default="vienna", choices=["vienna", "contrafold"])
    args = ap.parse_args()
    L, W = args.span, args.max_w
    rows = []
    if args.model == "contrafold":
        c = ractip_amd.Context(device=0, model=hot.RH_MODEL_CONTRAFOLD)
        c.set_span_contrafold(True)
        if W > 1:
            c.set_region_accessibility(True)
    else:
        c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    for shape in args.shapes.split(","):
        n, K = (int(x) for x in shape.split("x"))
        enc = ["".join(np.random.RandomState(n + 7919 * k).choice(list("ACGU"), n)).encode() for k in range(K)]
        arr = (ctypes.c_char_p * K)(*enc)
        lens = (ctypes.c_int * K)(*([n] * K))
        runs, same = [], True
        for rep in range(1 + args.repeat):
            t0 = time.perf_counter()
            c._check(c.L.rh_span_fold_batch(c.h, arr, lens, K, L, W))
            t1 = time.perf_counter()
            batch_dev = c.span_batch_times()
            loop_wall, loop_dev = 0.0, [0.0, 0.0, 0.0]
            for k in range(K):
                t2 = time.perf_counter()
                c._check(c.L.rh_span_fold_acc(c.h, enc[k], n, L, W))
                loop_wall += time.perf_counter() - t2
                sw, ex = c.span_times()
                loop_dev[0] += sw
                loop_dev[1] += ex
                loop_dev[2] += sum(c.span_acc_times()) if W > 1 else 0.0
                if rep == 0:           # (the warm-up run: the comparison is not timed)
                    one = c.local_results()
                    got = c.span_batch_results(k)
                    same = same and bool((one[0] == got[0]).all() and (one[1] == got[1]).all() and one[2][0] == got[2])
            runs.append((1e3 * (t1 - t0), 1e3 * loop_wall, sum(batch_dev), sum(loop_dev)) + tuple(batch_dev) + tuple(loop_dev))
        cols = [spread(col) for col in zip(*runs[1:])]
        row = dict(model=args.model, n=n, K=K, L=L, max_w=W, same_bits=same, batch_wall_ms=cols[0], loop_wall_ms=cols[1], batch_device_ms=cols[2], loop_device_ms=cols[3],
                   wall_ratio=cols[0][0] / cols[1][0], device_ratio=cols[2][0] / cols[3][0],
                   batch_sweeps_ms=cols[4], batch_exterior_finish_ms=cols[5], batch_acc_ms=cols[6],
                   loop_sweeps_ms=cols[7], loop_exterior_finish_ms=cols[8], loop_acc_ms=cols[9])
        rows.append(row)
        print(json.dumps(row), flush=True)
    c.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
