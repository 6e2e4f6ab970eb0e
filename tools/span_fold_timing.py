"""Timing of span-limited folding (Context.span_fold) on the GPU, next to the window route for the same sequence on the same
context: local_fold(W = L, S = 1), which folds n - W + 1 windows of W letters where the span fold fills one band of n x L cells.

  python tools/span_fold_timing.py [--out FILE.json] [--n 5000,20000,100000] [--span 200] [--repeat 5] [--no-windows] [--max-w W] [--constraint]
                                   [--model vienna|contrafold] [--window-fraction F]

Per n, the median and the range of --repeat runs behind one warm-up run (which allocates): wall time of rh_span_fold alone and of
the fetch of band, up and log Z; device time of the sweeps and of the exterior passes + finish (rh_span_times); the launches of the
sweeps (2 Le) and the device time per launch that gives; the same for local_fold (wall with its fetch, rh_local_times).
--max-w W (default 1): the span fold with region accessibilities up[i][w] of W widths (rh_span_fold_acc); for W > 1 also the device
time of the three parts of the accessibility stage (rh_span_acc_times: hairpin part, gap sums, final kernel), and local_fold runs
on the same context at max_w = W, the route to wide accessibilities that the stage replaces.
--constraint: also the same sequence under a structure constraint of scattered helices and x runs (rh_span_fold_constrained,
scattered_constraint below): its wall and device times next to the unconstrained ones, and the ratio of the sweeps.
--model contrafold: the same on a CONTRAfold context with its span folds switched on (Context.set_span_contrafold; no --constraint
there) and, for --max-w above 1, its region accessibility (Context.set_region_accessibility), local_fold(W = L, S = 1) on that same
context included.  The three parts of the stage are then: everything but the multiloop chain, the chain's S build, its links and
closes (the JSON keys stay acc_hairpin_ms, acc_gaps_ms, acc_final_ms).
--window-fraction F (default 1): local_fold runs on the first F n letters only and its times are scaled by 1 / F (stated in the row)."""
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


def spread(values):
    """[median, min, max]"""
    v = sorted(values)
    return [v[len(v) // 2], v[0], v[-1]]


PAIRS = {"GC", "CG", "AU", "UA", "GU", "UG"}


def scattered_constraint(seq, L, every=300):
    """a constraint over seq as it is: every `every` letters a helix -- the first (a, b) from there with 10 <= b - a <= min(40, L - 1)
    whose letters are complementary, grown inwards while they stay so, six brackets at the most -- and, half a period on, eight 'x'"""
    n, c = len(seq), ["."] * len(seq)
    for at in range(20, n - 60, every):
        found = next(((a, a + d) for a in range(at, at + 10) for d in range(min(40, L - 1), 9, -1) if seq[a] + seq[a + d] in PAIRS), None)
        if found:
            a, b = found
            for k in range(6):
                if b - a < 5 or seq[a] + seq[b] not in PAIRS:
                    break
                c[a], c[b] = "(", ")"
                a, b = a + 1, b - 1
        x = at + every // 2
        if x + 8 < n:
            c[x:x + 8] = "x" * 8
    return "".join(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", default="5000,20000,100000")
    ap.add_argument("--span", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-windows", action="store_true")
    ap.add_argument("--max-w", type=int, default=1)
    ap.add_argument("--constraint", action="store_true")
    ap.add_argument("--model", default="vienna", choices=["vienna", "contrafold"])
    ap.add_argument("--window-fraction", type=float, default=1.0)
    args = ap.parse_args()
    L, W = args.span, args.max_w
    rows = []
    if args.model == "contrafold":
        if args.constraint:
            ap.error("--model contrafold takes no --constraint")
        c = ractip_amd.Context(device=0, model=hot.RH_MODEL_CONTRAFOLD)
        c.set_span_contrafold(True)
        if W > 1:
            c.set_region_accessibility(True)
            c.set_max_w(W)             # for local_fold, as below
    else:
        c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
        c.set_max_w(W)                 # for local_fold; the span fold takes its widths as an argument
    for n in [int(x) for x in args.n.split(",")]:
        seq = "".join(np.random.RandomState(n).choice(list("ACGU"), n))
        enc = seq.encode()
        runs = []
        for _ in range(1 + args.repeat):
            t0 = time.perf_counter()
            c._check(c.L.rh_span_fold_acc(c.h, enc, n, L, W))
            t1 = time.perf_counter()
            band, up, logz, _ = c.local_results()
            t2 = time.perf_counter()
            runs.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)) + c.span_times() + (c.span_acc_times() if W > 1 else ()))
        call_ms, fetch_ms, sweep_ms, ext_ms = (spread(col) for col in list(zip(*runs[1:]))[:4])
        launches = 2 * min(L, n)
        row = dict(model=args.model, n=n, L=L, max_w=W, logZ=float(logz[0]), span_call_ms=call_ms, span_fetch_ms=fetch_ms, span_sweeps_ms=sweep_ms, span_exterior_finish_ms=ext_ms,
                   sweep_launches=launches, sweep_us_per_launch=1e3 * sweep_ms[0] / launches, result_bytes=8 * (band.size + up.size + 1),
                   pairs_above_half=int((band > 0.5).sum()))
        if W > 1:
            hp_ms, gap_ms, final_ms = (spread(col) for col in list(zip(*runs[1:]))[4:])
            row.update(acc_hairpin_ms=hp_ms, acc_gaps_ms=gap_ms, acc_final_ms=final_ms,
                       acc_over_sweeps=(hp_ms[0] + gap_ms[0] + final_ms[0]) / sweep_ms[0])
        if args.constraint:
            cons = scattered_constraint(seq, L)
            cenc, runs = cons.encode(), []
            for _ in range(1 + args.repeat):
                t0 = time.perf_counter()
                c._check(c.L.rh_span_fold_constrained(c.h, enc, n, cenc, L, W))
                t1 = time.perf_counter()
                _, _, clogz, _ = c.local_results()
                runs.append((1e3 * (t1 - t0),) + c.span_times() + (c.span_acc_times() if W > 1 else ()))
            cols = [spread(col) for col in zip(*runs[1:])]
            row.update(cons_brackets=cons.count("("), cons_x=cons.count("x"), cons_logZ=float(clogz[0]), cons_call_ms=cols[0], cons_sweeps_ms=cols[1],
                       cons_exterior_finish_ms=cols[2], cons_sweeps_over_plain=cols[1][0] / sweep_ms[0], cons_call_over_plain=cols[0][0] / call_ms[0])
            if W > 1:
                row.update(cons_acc_ms=[sum(x) for x in zip(*cols[3:6])])
        if not args.no_windows:
            runs = []
            frac = args.window_fraction
            cut = seq if frac >= 1.0 else seq[:max(L, int(n * frac))]
            scale = (n - L + 1) / max(1, len(cut) - L + 1)     # windows of the whole sequence per window folded
            for _ in range(1 + args.repeat):
                t0 = time.perf_counter()
                wband, wup, wlogz, starts = c.local_fold(cut, L, 1)
                runs.append(tuple(scale * t for t in (1e3 * (time.perf_counter() - t0),) + c.local_times()))
            wall_ms, fold_ms, acc_ms = (spread(col) for col in zip(*runs[1:]))
            row.update(windows=len(starts), window_scale=scale, window_wall_ms=wall_ms, window_folds_ms=fold_ms, window_accumulate_ms=acc_ms,
                       window_over_span_device=(fold_ms[0] + acc_ms[0]) / (sweep_ms[0] + ext_ms[0] + (hp_ms[0] + gap_ms[0] + final_ms[0] if W > 1 else 0.0)))
            if frac >= 1.0:
                row.update(max_abs_band_difference=float(np.abs(wband - band).max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    c.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
