"""Exterior sums of the strip sweeps in one pass per direction (lin_f5i_pass / lin_f5o_pass, mccaskill_strip.hip).

The strip launches no longer carry a workgroup that computes eight entries of F5i / F5o; one kernel per direction computes all of
them, in blocks of sixteen entries whose operands are fetched ahead of the chain.  The partition of every sum is the one the serial
kernels have (thread t of 256 takes terms t, t+256, .. ascending, then the wavefront sums, then the four partial sums in order), so
the results are the same BITS as under RH_F5_PASS=0, which runs the same strips with lin_f5i_tail / lin_f5o_head over the full range.

One mixed batch: lengths around the first strips (40, 41, 47..49), the group edges at 57 (56..58), the edges of a sixteen-entry
block (F5i blocks start at 32: 47/48/49, 63/64/65; F5o blocks start at n-1), a second and a third term per thread (k >= 256: 257..259,
k >= 512: 513, 514, 530), and 7, 20, 39 letters, which are routed away from the strips.  It runs with a sequence count that is a
multiple of 8 (XCD-pinned grids) and one that is not.  Checked: bp / up / log Z against the CPU oracle at the tolerances of
tests/test_gpu_parity.py, every output as bytes against RH_F5_PASS=0, 41 / 257 / 513 letters alone against the batch as bytes, and
RH_STRIP=1 / RH_STRIP=2 (strips for one sweep only) on the 257- and 513-letter sequences.
"""
import numpy as np
import pytest

from _oracle import assert_prob_close

pytestmark = pytest.mark.gpu

REL = 1e-6
STRIP_LENS = [40, 41, 47, 48, 49, 56, 57, 58, 63, 64, 65, 97, 255, 256, 257, 258, 259, 300, 511, 512, 513, 514, 530]
ROUTED_LENS = [7, 20, 39]
ALONE = [41, 257, 513]
STRIPS = ("lin_inside_strip<8, 8, 1>", "lin_outside_strip<8, 8, 1>")
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")


def rnd(rng, n):
    return "".join("ACGU"[k] for k in rng.randint(0, 4, n))


def sequences():
    rng = np.random.RandomState(532)
    seqs = [rnd(rng, n) for n in STRIP_LENS + ROUTED_LENS]
    fill = [rnd(rng, n) for n in (60, 61, 70, 71, 80, 81)]
    return seqs, fill


def batches():
    """pinned -> pairs: 26 sequences (not a multiple of 8: group-major grids) and the same plus six fillers (32: XCD-pinned grids)"""
    seqs, fill = sequences()
    plain = [(seqs[q], seqs[q + 1]) for q in range(0, len(seqs), 2)]
    return {False: plain, True: plain + [(fill[q], fill[q + 1]) for q in range(0, len(fill), 2)]}


def compute(env, pairs, alone=()):
    """Results of one batch (and of `alone` sequences one at a time) on a context created under `env`"""
    import ractip_amd
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        c = ractip_amd.Context(device=0)
    finally:
        mp.undo()
    try:
        singles = [c.bpp(s) for s in alone]
        c.batch_upload(pairs)
        c.batch_compute()
        assert c.last_path() == 1 and c.batch_fallbacks(0) == [] and c.batch_fallbacks(2) == [], (env, c.last_path())
        return dict(res=[c.batch_results(p) for p in range(len(pairs))], kernels=c.batch_kernels(), launches=tuple(c.batch_timings()[1]), alone=singles)
    finally:
        c.close()


@pytest.fixture(scope="module")
def runs(hotlib):
    """Every GPU result of this file, computed once: the two batches under the pass kernels and under RH_F5_PASS=0"""
    seqs, _ = sequences()
    alone = [seqs[STRIP_LENS.index(n)] for n in ALONE]
    out = {}
    for pinned, pairs in batches().items():
        out["pass", pinned] = compute({}, pairs, alone if pinned else ())
        out["serial", pinned] = compute({"RH_F5_PASS": "0"}, pairs)
    return out


@pytest.fixture(scope="module")
def truth(oracle):
    seqs, fill = sequences()
    return {s: oracle.inference(s) for s in seqs + fill}


def per_sequence(pairs, res):
    for (s1, s2), r in zip(pairs, res):
        yield s1, r["bp1"], r["up1"], r["logZ"][0]
        yield s2, r["bp2"], r["up2"], r["logZ"][1]


def check_oracle(oracle, truth, pairs, res, what):
    for s, bp, up, z in per_sequence(pairs, res):
        o = truth[s]
        assert abs(z - o["logZ"]) < 1e-9, (what, len(s), z, o["logZ"])
        assert_prob_close(bp, o["post"], rel=REL, what="%s bp n=%d" % (what, len(s)))
        ref = oracle.up_float(len(s), bp.astype(np.float32))   # ractip.cpp:213-222 in float
        assert np.abs(up.astype(np.float32) - ref).max() < 2e-6, (what, len(s))


def assert_same_bytes(a, b, what):
    assert len(a) == len(b)
    for p, (r, r0) in enumerate(zip(a, b)):
        for key in KEYS:
            assert r[key].tobytes() == r0[key].tobytes(), (what, p, key)


@pytest.mark.parametrize("pinned", [True, False], ids=["multiple_of_8", "not_multiple_of_8"])
def test_pass_against_oracle(runs, oracle, truth, pinned):
    r = runs["pass", pinned]
    assert (r["kernels"][0][0], r["kernels"][1][0]) == STRIPS, r["kernels"]
    check_oracle(oracle, truth, batches()[pinned], r["res"], "pass")


@pytest.mark.parametrize("pinned", [True, False], ids=["multiple_of_8", "not_multiple_of_8"])
def test_pass_same_bytes_as_serial_kernels(runs, pinned):
    a, b = runs["pass", pinned], runs["serial", pinned]
    assert a["kernels"] == b["kernels"] and a["launches"] == b["launches"], (a["kernels"], b["kernels"], a["launches"], b["launches"])
    assert_same_bytes(a["res"], b["res"], "RH_F5_PASS=0")


def test_batch_size_does_not_matter(runs):
    """the 26 sequences of the smaller batch: the same bytes next to six more sequences and on the other grid mapping"""
    assert_same_bytes(runs["pass", True]["res"][:len(runs["pass", False]["res"])], runs["pass", False]["res"], "32 against 26 sequences")


def test_alone_same_bytes_as_in_the_batch(runs):
    seqs, _ = sequences()
    r = runs["pass", True]
    inbatch = {s: (bp, z) for s, bp, up, z in per_sequence(batches()[True], r["res"])}
    for n, (bp, z) in zip(ALONE, r["alone"]):
        s = seqs[STRIP_LENS.index(n)]
        assert bp.tobytes() == inbatch[s][0].tobytes() and z == inbatch[s][1], n


@pytest.mark.parametrize("strip", ["1", "2"], ids=["inside_strips_only", "outside_strips_only"])
def test_strips_for_one_sweep(runs, oracle, truth, strip):
    """RH_STRIP=1 runs strips (and lin_f5i_pass) for the inside sweep only, RH_STRIP=2 strips (and lin_f5o_pass) for the outside sweep only;
    the other sweep is the diagonal-pair kernels, which compute their own exterior sums.  Every output is the same bytes as the same
    organisation under RH_F5_PASS=0.  Under RH_STRIP=1 the inside sweep is that of RH_STRIP=3, so log Z (= F5i[n]) is also the same
    bytes as RH_STRIP=3 under RH_F5_PASS=0; the outside sweep of RH_STRIP=2 starts from another organisation's inside tables, so it has
    no output to compare with RH_STRIP=3 bit by bit."""
    seqs, _ = sequences()
    pairs = [(seqs[STRIP_LENS.index(257)], seqs[STRIP_LENS.index(513)])]
    got = compute({"RH_STRIP": strip}, pairs)
    ref = compute({"RH_STRIP": strip, "RH_F5_PASS": "0"}, pairs)
    assert_same_bytes(got["res"], ref["res"], "RH_STRIP=%s" % strip)
    check_oracle(oracle, truth, pairs, got["res"], "RH_STRIP=%s" % strip)
    if strip == "1":
        z3 = {s: z for s, bp, up, z in per_sequence(batches()[True], runs["serial", True]["res"])}
        for s, bp, up, z in per_sequence(pairs, got["res"]):
            assert z == z3[s], len(s)
