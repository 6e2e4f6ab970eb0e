"""What an indexed batch saves on a screen: a 32 x 32 cross product at n = 500 (CONTRAfold model) as ONE indexed batch of 1024 pairs
over 64 distinct sequences, against the same 1024 pairs as four plain batches of 256 pairs (2048 folds).  Five computes each,
interleaved; per-phase device times of rh_batch_timings (ms: inside, outside, duplex, whole compute), summed over the four plain
batches.  Prints one JSON line.

  python tools/indexed_timing.py [--side 32] [--n 500] [--repeats 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ractip_amd  # noqa: E402
from ractip_amd import hot  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=32)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.RandomState(500)
    rnd = lambda: "".join(rng.choice(list("ACGU"), args.n))
    queries, targets = [rnd() for _ in range(args.side)], [rnd() for _ in range(args.side)]
    pairs = [(q, t) for q in queries for t in targets]
    seqs, first, second = hot.index_pairs(pairs)
    quarter = len(pairs) // 4
    blocks = [pairs[k * quarter:(k + 1) * quarter] for k in range(4)]
    ci, cp = ractip_amd.Context(device=0), ractip_amd.Context(device=0)
    indexed, plain = [], []
    check = None
    for rep in range(args.repeats + 1):           # the first round allocates tables and captures the graphs: not reported
        ci.batch_upload_indexed(seqs, list(zip(first, second)))
        ci.batch_compute()
        ms_i = ci.batch_timings()[0]
        ms_p = np.zeros(4)
        for k, b in enumerate(blocks):
            cp.batch_upload(b)
            cp.batch_compute()
            ms_p += np.array(cp.batch_timings()[0])
            if rep == 0 and k == 3:               # the last pair of both forms: same bits
                a, c = ci.batch_results(len(pairs) - 1), cp.batch_results(quarter - 1)
                check = all(np.array_equal(a[key], c[key]) for key in ("bp1", "bp2", "up1", "up2", "hp", "logZ"))
        if rep:
            indexed.append([round(float(x), 3) for x in ms_i])
            plain.append([round(float(x), 3) for x in ms_p])
    ci.close()
    cp.close()
    med = lambda rows: [round(float(x), 3) for x in np.median(np.array(rows), axis=0)]
    print(json.dumps({"pairs": len(pairs), "distinct": len(seqs), "n": args.n, "phases_ms": ["inside", "outside", "duplex", "compute"],
                      "indexed_1x%d" % len(pairs): indexed, "plain_4x%d" % quarter: plain,
                      "indexed_median": med(indexed), "plain_median": med(plain), "last_pair_same_bits": check}))


if __name__ == "__main__":
    main()
