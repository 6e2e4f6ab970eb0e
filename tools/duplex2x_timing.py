"""Device time of the pf_duplex phase under the ViennaRNA-2.x loop energies: log-space kernels against the scaled linear
ones (rh_set_duplex_mode), with the 1.8 context's linear duplex time on the same batch as the yardstick.

    python tools/duplex2x_timing.py [--pairs 256] [--n 500] [--reps 5] [--seed 1]

BL* tables, semantics = 2 (zero-filled 2.x slots), set_hybrid(DUPLEX), rh_set_overlap(ctx, 0): rh_batch_timings ms[2] is the
duplex phase alone on the device.  After a warm-up of each mode, `reps` computes per mode, interleaved.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import ractip_amd
    from ractip_amd import hot
    rng = np.random.default_rng(args.seed)
    seq = lambda: "".join("ACGU"[k] for k in rng.integers(0, 4, args.n))
    pairs = [(seq(), seq()) for _ in range(args.pairs)]
    c20 = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL, vienna=dict(semantics=2))
    c18 = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    out = {"pairs": args.pairs, "n": args.n, "reps": args.reps}
    try:
        for c in (c20, c18):
            c.set_hybrid(False)
            c.set_overlap(False)
            c.batch_upload(pairs)

        def duplex_ms(c, mode):
            c.set_duplex_mode(mode)
            c.batch_compute()
            return c.batch_timings()[0][2], c.last_hybrid_path(), c.batch_kernels()[2][0]

        for mode in (hot.RH_MODE_LOG, hot.RH_MODE_AUTO):   # warm-up: graph capture, first touch of the tables
            duplex_ms(c20, mode)
        duplex_ms(c18, hot.RH_MODE_INHERIT)
        series = {"2x_log": [], "2x_auto": [], "18_linear": []}
        seen = {}
        for _ in range(args.reps):
            for name, c, mode in (("2x_log", c20, hot.RH_MODE_LOG), ("2x_auto", c20, hot.RH_MODE_AUTO), ("18_linear", c18, hot.RH_MODE_INHERIT)):
                ms, path, kern = duplex_ms(c, mode)
                series[name].append(round(ms, 3))
                seen[name] = {"hybrid_path": path, "kernel": kern}
        med = {k: float(np.median(v)) for k, v in series.items()}
        out.update(duplex_ms=series, median_ms=med, ran=seen,
                   ratio_2x_auto_to_2x_log=med["2x_auto"] / med["2x_log"], ratio_2x_auto_to_18_linear=med["2x_auto"] / med["18_linear"])
    finally:
        c20.close()
        c18.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
