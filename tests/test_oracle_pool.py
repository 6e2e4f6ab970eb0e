"""CPU test of the thread-pooled, memoised oracles (tests/_oracle.py: OraclePool) that the GPU tests at production shapes use:
calls that run at the same time on the pool's threads return the same bits as the same calls made one after another."""
import numpy as np

from _oracle import ORACLE_WORKERS, Oracle, OraclePool, ViennaOracle


def test_threaded_oracle_calls_equal_serial_calls():
    rng = np.random.default_rng(2024)
    seqs = ["".join(rng.choice(list("ACGU"), size=n)) for n in (37, 64, 90, 121, 150, 173)]
    pairs = list(zip(seqs[0::2], seqs[1::2])) + [(seqs[5], seqs[0])]
    pool = OraclePool(workers=64)
    try:
        assert pool.pool._max_workers == ORACLE_WORKERS == 8
        # everything submitted before anything is read: the calls overlap on the pool's threads
        cf = [pool.inference(s) for s in seqs]
        dx = [pool.duplex(a, b) for a, b in pairs]
        mc = [pool.mccaskill(s) for s in seqs]
        co = [pool.cofold(a, b) for a, b in pairs]
        vd = [pool.pf_duplex(a, b) for a, b in pairs]
        assert pool.inference(seqs[0]) is cf[0] and pool.cofold(*pairs[1]) is co[1]   # memoised by the inputs
        o, vo = Oracle(), ViennaOracle()
        for s, f in zip(seqs, cf):
            got, want = f.result(), o.inference(s)
            assert got["logZ"] == want["logZ"] and np.array_equal(got["post"], want["post"]), len(s)
        for (a, b), f in zip(pairs, dx):
            got, want = f.result(), o.duplex(a, b)
            assert all(np.array_equal(got[k], want[k]) for k in ("logZ2", "post", "inside", "outside")), (len(a), len(b))
        for s, f in zip(seqs, mc):
            got, want = f.result(), vo.mccaskill(s, max_w=15)
            assert got["logZ"] == want["logZ"] and np.array_equal(got["post"], want["post"]) and np.array_equal(got["up"], want["up"])
        for (a, b), f in zip(pairs, co):
            got, want = f.result(), vo.cofold(a, b)
            assert got["logZ"] == want["logZ"] and np.array_equal(got["post"], want["post"]) and np.array_equal(got["hp"], want["hp"])
        for (a, b), f in zip(pairs, vd):
            got, want = f.result(), vo.pf_duplex(a, b)
            assert got["logZ"] == want["logZ"] and np.array_equal(got["pr"], want["pr"])
    finally:
        pool.close()
