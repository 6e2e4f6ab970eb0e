"""Timing of local hybridization of two windowed molecules (Context.local_duplex2) on the GPU: every window of s1 against every
window of s2.

  python tools/local_duplex2_timing.py [--out FILE.json] [--shapes 2000,5000,50:5000,20000,100] [--window 200] [--repeat 5]

Per (source, n1, n2, S) with W = --window on both molecules, the median and the range of --repeat runs behind one warm-up run (which
allocates and captures the launch graphs): wall time of local_duplex2 including the fetch of hp and log Z; device time of the tiles'
computes and of the row + add + finish kernels (rh_local_hp2_times); the automatic tile; the bytes those three kernels must move,
computed from the shapes over the walk of that tile -- every hp entry of every pair read once, the row buffer written once per
column tile and read again where a column's windows continue from an earlier tile, read once more by the add kernel, hp_loc2
written once per row block (read where a row continues), read and written once more by the finish kernel -- and the rate that gives.
DESIGN.md section 5 records a copy bandwidth of 5.2 TB/s on this GPU.

Beside it, on the same context, the route a caller has without this call: one local_duplex(window k of s1, s2, windowed=2) per window
of s1, each result fetched and the nw1 matrices averaged in numpy.  The tool asserts that local_duplex2 under tiles of nw1 rows gives
the same values to 1e-12 relative (the bits may differ: that route divides once per call) and the same bits as under the automatic
tile."""
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


def first_window(starts, We, n):
    """per 0-based letter the first window that contains it"""
    first = np.full(n, -1)
    for k in reversed(range(len(starts))):
        first[starts[k]:starts[k] + We] = k
    return first


def kernel_bytes(n1, n2, W, S, rows, cols):
    """bytes the row, add and finish kernels move over the walk of (rows, cols) tiles"""
    a, b, We1, We2 = windows(n1, W, S), windows(n2, W, S), min(W, n1), min(W, n2)
    f1, f2 = first_window(a, We1, n1), first_window(b, We2, n2)
    doubles = len(a) * len(b) * We1 * We2                                   # every hp entry of every pair, once
    for kA in range(0, len(a), rows):
        kB = min(len(a), kA + rows)
        for lA in range(0, len(b), cols):
            lB = min(len(b), lA + cols)
            t0, t1 = b[lA], b[lB - 1] + We2
            carried = int((f2[t0:t1] < lA).sum())                          # columns that continue from an earlier column tile
            doubles += (kB - kA) * We1 * ((t1 - t0) + carried)
        i0, i1 = a[kA], a[kB - 1] + We1
        doubles += (kB - kA) * We1 * n2                                      # the add kernel reads the block's row buffers ...
        doubles += ((i1 - i0) + int((f1[i0:i1] < kA).sum())) * n2            # ... writes its rows of hp_loc2, reads those that continue
    doubles += n1 * n2 + (n1 + 1) * (n2 + 1)                                 # finish: read, write
    return 8 * doubles


def spread(values):
    """[median, min, max]"""
    v = sorted(values)
    return [v[len(v) // 2], v[0], v[-1]]


def by_local_duplex(c, s1, s2, W, S):
    """the route without local_duplex2: a local_duplex per window of s1, averaged on the host in increasing window order"""
    a, We1 = windows(len(s1), W, S), min(W, len(s1))
    acc, cnt = np.zeros((len(s1) + 1, len(s2) + 1)), np.zeros(len(s1) + 1)
    for s in a:
        hp, _, _ = c.local_duplex(s1[s:s + We1], s2, W, S, windowed=2)
        acc[s + 1:s + We1 + 1] += hp[1:]
        cnt[s + 1:s + We1 + 1] += 1
    acc[1:] /= cnt[1:, None]
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="2000,5000,50:5000,20000,100", help="n1,n2,S per shape, shapes separated by ':'")
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sources", default="contrafold-duplex,vienna-duplex,vienna-cofold")
    args = ap.parse_args()
    W = args.window
    out = []
    for name in args.sources.split(","):
        c = ractip_amd.Context(device=0, model=hot.RH_MODEL_CONTRAFOLD if name.startswith("contrafold") else hot.RH_MODEL_VIENNA_BL)
        if name.startswith("vienna"):
            c.set_hybrid(name == "vienna-cofold")
        for shape in args.shapes.split(":"):
            n1, n2, S = (int(x) for x in shape.split(","))
            s1 = "".join(np.random.RandomState(n1).choice(list("ACGU"), n1))
            s2 = "".join(np.random.RandomState(n2 + 1).choice(list("ACGU"), n2))
            nw1, nw2 = len(windows(n1, W, S)), len(windows(n2, W, S))
            c.set_local_tile(0, 0)
            runs = []
            for _ in range(1 + args.repeat):
                t0 = time.perf_counter()
                hp, logz, _, _ = c.local_duplex2(s1, s2, W, S)
                wall = time.perf_counter() - t0
                runs.append((1e3 * wall,) + c.local_hp2_times())
            rows, cols = c.local_hp2_tile()
            wall_ms, compute_ms, acc_ms = (spread(col) for col in zip(*runs[1:]))
            nbytes = kernel_bytes(n1, n2, W, S, rows, cols)
            row = dict(source=name, n1=n1, n2=n2, W=W, S=S, windows=[nw1, nw2], pairs=nw1 * nw2, tile=[rows, cols], wall_ms=wall_ms,
                       compute_ms=compute_ms, accumulate_ms=acc_ms, kernel_bytes=nbytes, accumulate_TBs=nbytes / (acc_ms[0] * 1e-3) / 1e12,
                       copy_TBs=COPY_TBS, result_bytes=8 * (hp.size + logz.size), path=c.last_path(), hybrid_path=c.last_hybrid_path())
            # tiles of nw1 rows with about as many pairs as the automatic tile: every window of s2 is folded once
            wide = max(1, min(nw2, rows * cols // nw1, 32767 // nw1))
            c.set_local_tile(nw1, wide)
            runs = []
            for _ in range(1 + args.repeat):
                t0 = time.perf_counter()
                hp_rows = c.local_duplex2(s1, s2, W, S)[0]
                runs.append(1e3 * (time.perf_counter() - t0))
            row["tile_nw1_rows"] = [nw1, wide]
            row["wall_ms_nw1_rows"] = spread(runs[1:])
            assert np.array_equal(hp_rows, hp), "the bits depend on the tiling"
            c.set_local_tile(0, 0)
            runs = []
            for _ in range(1 + args.repeat):
                t0 = time.perf_counter()
                old = by_local_duplex(c, s1, s2, W, S)
                runs.append(1e3 * (time.perf_counter() - t0))
            row["wall_ms_by_local_duplex"] = spread(runs[1:])
            assert np.allclose(hp_rows, old, rtol=1e-12, atol=0.0), "local_duplex2 and the per-window route disagree"
            row["max_rel_difference"] = float(np.max(np.abs(hp_rows - old)[old > 0] / old[old > 0]))
            out.append(row)
            print(json.dumps(row), flush=True)
        c.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
