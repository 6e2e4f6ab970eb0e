"""What the packed float fetch saves: the dense results of one computed batch (CONTRAfold model, the sequences of
ractip_amd/seqgen.py) fetched (A) by batch_results_all_into -- padded doubles into page-locked buffers, the existing path and the
yardstick -- and (B) by batch_results_packed_f32 -- floats narrowed and packed on the device, into page-locked buffers.  After one
compute and one untimed fetch of each (buffer allocation), seven interleaved rounds A, B; host clock around each call (a call ends
in a stream synchronize).  Per path: median ms, bytes moved device-to-host, GB/s; the device time of the pack kernel from its event
pair (median over the rounds) with the bytes it reads and writes; and whether the floats of B equal np.float32 of the doubles of A.
Prints one JSON line.

  python tools/dense_f32_timing.py [pairs=256] [n=500]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ractip_amd  # noqa: E402
from ractip_amd import seqgen  # noqa: E402

ROUNDS = 7


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    ctx = ractip_amd.Context(device=0)
    ctx.batch_upload(seqgen.random_pairs(pairs, n))
    ctx.batch_compute()
    a_bufs = ctx.batch_results_all_into()
    b = ctx.batch_results_packed_f32()
    a_ms, b_ms, k_ms = [], [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        a_bufs = ctx.batch_results_all_into(a_bufs)
        t1 = time.perf_counter()
        b = ctx.batch_results_packed_f32(b["bufs"])
        t2 = time.perf_counter()
        a_ms.append((t1 - t0) * 1e3)
        b_ms.append((t2 - t1) * 1e3)
        k_ms.append(ctx.batch_pack_time())
    a_bytes = sum(x.nbytes for x in a_bufs)
    b_bytes = sum(x.nbytes for x in b["bufs"])
    # same values: every block of B against the float32 of the block of A it was narrowed from
    ts, uld, hld = a_bufs[0].shape[1], a_bufs[1].shape[1], a_bufs[2].shape[1] // (n + 2)
    same = True
    for k in range(2 * pairs):
        same &= np.array_equal(b["bp"][k].view(np.uint32), a_bufs[0][k][:b["bp"][k].size].astype(np.float32).view(np.uint32))
        same &= np.array_equal(b["up"][k].view(np.uint32), a_bufs[1][k][:n].astype(np.float32).view(np.uint32))
    for p in range(pairs):
        block = a_bufs[2][p][:(n + 1) * hld].reshape(n + 1, hld)[:, :n + 1]
        same &= np.array_equal(b["hp"][p].view(np.uint32), block.astype(np.float32).view(np.uint32))
    med = lambda v: float(np.median(v))
    kernel_bytes = 8 * (sum(x.size for x in b["bp"]) + sum(x.size for x in b["up"]) + sum(x.size for x in b["hp"])) + sum(x.nbytes for x in b["bufs"][:3])
    out = {"pairs": pairs, "n": n, "rounds": ROUNDS,
           "A_results_all_into": {"median_ms": round(med(a_ms), 2), "bytes": a_bytes, "GBps": round(a_bytes / med(a_ms) / 1e6, 2),
                                  "pairs_per_s": round(pairs * 1e3 / med(a_ms)), "ms": [round(x, 2) for x in a_ms]},
           "B_results_packed_f32": {"median_ms": round(med(b_ms), 2), "bytes": b_bytes, "GBps": round(b_bytes / med(b_ms) / 1e6, 2),
                                    "pairs_per_s": round(pairs * 1e3 / med(b_ms)), "ms": [round(x, 2) for x in b_ms]},
           "pack_kernel": {"median_ms": round(med(k_ms), 3), "bytes_read_and_written": kernel_bytes,
                           "GBps": round(kernel_bytes / med(k_ms) / 1e6, 1), "ms": [round(x, 3) for x in k_ms]},
           "B_over_A_time": round(med(b_ms) / med(a_ms), 3), "B_over_A_bytes": round(b_bytes / a_bytes, 3),
           "B_equals_float32_of_A": bool(same), "padded_layout": {"tri_stride": ts, "up_ld": uld, "hp_ld": hld}}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
