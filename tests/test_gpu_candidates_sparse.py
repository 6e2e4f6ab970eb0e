"""The write pass of the threshold scans (candidates.hip) skips every row in which the count pass found nothing.  Records, first[],
found and the truncation at cap must stay what a numpy threshold of the dense results narrowed to float32 gives: on a ragged batch
whose rows are mostly empty, never empty (threshold 0), and all empty (threshold 1)."""
import ctypes

import numpy as np
import pytest

from _oracle import tri_offset

pytestmark = pytest.mark.gpu

LENGTHS = ((7, 40), (65, 130), (40, 7), (130, 65))
# (a) most rows empty, (b) no row empty, (c) nothing at all -- per scan: bp1, bp2, hp, up1, up2
SPARSE = (0.5, 0.5, 0.4, 0.999, 0.999)   # (hp of pairs this short is concentrated: 0.1 leaves most rows occupied)


def rnd(rng, n):
    return "".join(rng.choice(list("ACGU"), n))


@pytest.fixture(scope="module")
def batch(hotlib):
    import ractip_amd
    rng = np.random.RandomState(2024)
    pairs = [(rnd(rng, a), rnd(rng, b)) for a, b in LENGTHS]
    c = ractip_amd.Context(device=0)
    c.batch_upload(pairs)
    c.batch_compute()
    dense = [c.batch_results(p) for p in range(len(pairs))]
    yield c, pairs, dense
    c.close()


def want_records(which, pair, r, th):
    """The reference's scan order: row-major, p > threshold after narrowing to float."""
    th = np.float32(th)
    n1, n2 = len(pair[0]), len(pair[1])
    out = []
    if which <= 1:
        n, bp = (n1, r["bp1"]) if which == 0 else (n2, r["bp2"])
        for i in range(1, n + 1):
            row = bp[tri_offset(n, i):tri_offset(n, i) + n + 1].astype(np.float32)
            out += [(i, j, row[j]) for j in range(i + 1, n + 1) if row[j] > th]
    elif which == 2:
        hp = r["hp"].astype(np.float32)
        out = [(i, j, hp[i, j]) for i in range(1, n1 + 1) for j in range(1, n2 + 1) if hp[i, j] > th]
    else:
        up = np.asarray(r["up1"] if which == 3 else r["up2"]).astype(np.float32).ravel()
        out = [(i, 0, up[i]) for i in range(up.size) if up[i] > th]
    return out


def as_tuples(rec):
    return [(int(a), int(b), np.float32(p)) for a, b, p in rec.tolist()]


@pytest.mark.parametrize("kind", ["sparse", "zero", "one"])
def test_batched_scans_equal_a_numpy_threshold(batch, kind):
    c, pairs, dense = batch
    for which in range(5):
        th = {"sparse": SPARSE[which], "zero": 0.0, "one": 1.0}[kind]
        rec, first = c.batch_candidates_all(which, th)
        want = [want_records(which, pairs[p], dense[p], th) for p in range(len(pairs))]
        assert first.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist(), (kind, which)
        assert as_tuples(rec) == [t for w in want for t in w], (kind, which)
        for p in range(len(pairs)):
            mine = [tuple(t) for t in rec[first[p]:first[p + 1]].tolist()]
            assert mine == c.batch_candidates(p, which, th), (kind, which, p)
            assert c.last_candidate_count == len(want[p])
        if kind == "one":
            assert len(rec) == 0
        if kind == "sparse" and which <= 2:
            # what the skip rests on: most rows hold nothing at these thresholds (and some do hold something)
            rows = [len({i for i, _, _ in w}) for w in want]
            total = sum(len(pr[0]) if which != 1 else len(pr[1]) for pr in pairs)
            assert 0 < sum(rows) < total / 2, (which, rows, total)


def test_cap_below_found_truncates_the_copy_only(batch):
    c, pairs, dense = batch
    for which, th in ((0, 0.0), (2, 0.1), (2, 0.0), (4, 0.0)):
        want = [t for p in range(len(pairs)) for t in want_records(which, pairs[p], dense[p], th)]
        cap = max(1, len(want) // 3)
        assert cap < len(want)
        buf = np.zeros(cap + 8, dtype=c.CAND_DTYPE)   # (eight records of slack: nothing may land behind cap)
        first = np.empty(len(pairs) + 1, dtype=np.int32)
        found = c.L.rh_batch_candidates_all(c.h, which, ctypes.c_float(th), buf.ctypes.data, cap, first.ctypes.data)
        assert found == len(want) and first[-1] == found
        assert as_tuples(buf[:cap]) == want[:cap]
        assert not buf[cap:]["i"].any() and not buf[cap:]["p"].any()
        # the per-pair call: the same truncation
        p = len(pairs) - 1
        mine = want_records(which, pairs[p], dense[p], th)
        got = c.batch_candidates(p, which, th, cap=2)
        assert c.last_candidate_count == len(mine) and [(i, j, np.float32(x)) for i, j, x in got] == mine[:2]
