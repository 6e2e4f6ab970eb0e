"""GPU suite (-m gpu) at the shapes bench.py measures: the lengths of the two-level block products and of the 64-column groups,
batches of a multiple of 8 sequences (the XCD-pinned grids of the sweep and strip kernels), the n=500 bench workload itself with two
contexts on two host threads, the n=2000 batch of --full and the Vienna-BL batches of --full.  Every matrix is compared densely
with the CPU oracles (tests/_oracle.py: OraclePool runs them on a few threads while the GPU computes) or, where the oracle is too
slow, with the same problem computed in another batch: placement (pinned or not, alone or inside a batch, one context or two)
must not change a bit."""
import numpy as np
import pytest

import bench
from _oracle import (OraclePool, assert_prob_close, check_n2000_golden, check_pair_properties, threshold_scans)
from ractip_amd.seqgen import random_pair, random_pairs

pytestmark = pytest.mark.gpu

REL = 1e-6
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")


def rnd(rng, n):
    return "".join(rng.choice(list("ACGU"), n))


def hairpins(rng, n):
    """A chain of stable GC hairpins (test_vienna_bl_flagged_pairs_are_recomputed_alone): log Z ~ 0.87 per letter under Vienna-BL."""
    comp = {"G": "C", "C": "G"}
    s = ""
    while len(s) < n:
        stem = "".join(rng.choice(list("GC"), size=10))
        s += stem + "AAAA" + "".join(comp[ch] for ch in reversed(stem)) + "AA"
    return s[:n]


def assert_same_bits(r, r0, what):
    for k in KEYS:
        assert np.array_equal(np.asarray(r[k]), np.asarray(r0[k])), (what, k)


def context(model=None):
    import ractip_amd
    return ractip_amd.Context(device=0) if model is None else ractip_amd.Context(device=0, model=model)


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    yield p
    p.close()


# ---- step 1: dense parity at the production lengths
# 383 / 384 / 385 sit on the two-level threshold (a 383-letter sequence keeps the one-level form next to longer ones), 448 = 7 macro
# tiles, 577 one letter past 9, 511 / 512 / 513 on the 16-block and 64-column group edges, 1000 many macro tiles per row
LENS = (383, 384, 385, 447, 448, 449, 500, 511, 512, 513, 577, 1000)


def production_seqs():
    rng = np.random.RandomState(383)
    s = {n: rnd(rng, n) for n in LENS}
    s[500], s["500b"] = random_pair(500)   # the golden mt19937(12345) pair
    return s


def production_batches():
    s = production_seqs()
    pinned = [(s[383], s[1000]), (s[384], s[513]), (s[448], s[500]), (s[577], s[449])]   # 8 sequences: pinned grids
    unpinned = [(s[385], s[511]), (s[447], s[512]), (s[500], s["500b"])]                # 6 sequences
    return pinned, unpinned


DENSE_HP = {("pinned", 0), ("pinned", 3), ("unpinned", 2)}   # 383 x 1000, 577 x 449, 500 x 500


@pytest.mark.parametrize("mode", [0, 1], ids=["auto", "log"])
def test_production_lengths_dense_vs_oracle(hotlib, opool, mode):
    pinned, unpinned = production_batches()
    batches = (("pinned", pinned), ("unpinned", unpinned))
    for name, pairs in batches:
        for p, (s1, s2) in enumerate(pairs):
            opool.inference(s1), opool.inference(s2)
            if (name, p) in DENSE_HP:
                opool.duplex(s1, s2)
    c = context()
    try:
        c.set_mode(mode)
        got = {}
        for name, pairs in batches:
            c.batch_upload(pairs)
            c.batch_compute()
            got[name] = [c.batch_results(p) for p in range(len(pairs))]
        alone = {s: c.bpp(s) for _, pairs in batches for pr in pairs for s in pr}
    finally:
        c.close()
    for name, pairs in batches:
        for p, ((s1, s2), r) in enumerate(zip(pairs, got[name])):
            what = "%s pair %d (%d, %d) mode %d" % (name, p, len(s1), len(s2), mode)
            for s, key, kz, ukey in ((s1, "bp1", 0, "up1"), (s2, "bp2", 1, "up2")):
                o = opool.inference(s).result()
                assert abs(r["logZ"][kz] - o["logZ"]) < 1e-8, (what, key)
                assert_prob_close(r[key], o["post"], rel=REL, what="%s %s" % (key, what))
                ref = opool.cf.up_float(len(s), r[key].astype(np.float32))   # ractip.cpp:213-222 in float
                assert np.abs(r[ukey].astype(np.float32) - ref).max() < 2e-6, (what, ukey)
                # a sequence's results do not depend on the batch it runs in (alone: unpinned, one sequence)
                bp_alone, z_alone = alone[s]
                assert np.array_equal(r[key], bp_alone) and r["logZ"][kz] == z_alone, ("alone vs batch", what, key)
            if (name, p) in DENSE_HP:
                od = opool.duplex(s1, s2).result()
                assert abs(r["logZ"][2] - od["logZ2"][0]) < 1e-8, what
                assert_prob_close(r["hp"], od["post"], rel=REL, what="hp " + what)


# ---- step 2: the organisations the library selects by environment agree at production lengths on a pinned batch
# "kernels": another kernel set than the default (rh_batch_kernels), results to 1e-10; "bits": placement or launch mode only, the
# default's kernels and its bits; "far2": the kernel names are the same (the one- / two-level choice is made per sequence inside the
# block-product kernels), so the sequences that change form must change some bit and the others must keep theirs.
# (RH_SMALL=1 is left out: the batch has no sequence of 8..109 letters for the one-workgroup kernel.)
VARIANTS = [
    ({"RH_STRIP_FILT": "0"}, "kernels"),
    ({"RH_STRIP": "0"}, "kernels"),
    ({"RH_STRIP": "1"}, "kernels"),
    ({"RH_STRIP": "2"}, "kernels"),
    ({"RH_STRIP_W": "4"}, "kernels"),
    ({"RH_STRIP_XCD": "0"}, "bits"),
    ({"RH_FAR2": "1"}, "far2"),          # names cannot show it: only the 383-letter sequence changes form (to two-level)
    ({"RH_FAR2": "0"}, "far2"),          # names cannot show it: every sequence of 384 letters or more changes form (to one-level)
    ({"RH_STRIP": "0", "RH_FAR2": "1"}, "kernels"),
    ({"RH_STRIP": "0", "RH_LOOKAHEAD": "1"}, "kernels"),
    ({"RH_STRIP": "0", "RH_LOOKAHEAD": "0"}, "kernels"),
    ({"RH_FAR_PK": "0"}, "kernels"),
    ({"RH_STRIP": "0", "RH_LOOKAHEAD": "0", "RH_LIN_W": "8"}, "kernels"),
    ({"RH_STRIP": "0", "RH_LIN_W": "8"}, "kernels"),
    ({"RH_DX_W": "8"}, "kernels"),
    ({"RH_DX_QUAD": "0"}, "kernels"),
    ({"RH_FAR_MFMA": "0"}, "kernels"),
    ({"RH_LIN_BS": "0"}, "kernels"),
    ({"RH_LIN_BS": "32"}, "kernels"),
    ({"RH_STRIP": "0", "RH_LIN_W": "16"}, "kernels"),
    ({"RH_STRIP": "0", "RH_LIN_W_IN": "8"}, "kernels"),
    ({"RH_DX_STRIP": "0"}, "kernels"),
    ({"RH_NO_GRAPH": "1"}, "bits"),
]


def test_organisations_agree_on_a_pinned_production_batch(hotlib, monkeypatch):
    pairs, _ = production_batches()
    seqs = [s for pr in pairs for s in pr]

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = context()
        try:
            c.batch_upload(pairs)
            c.batch_compute()
            assert c.last_path() == 1, env
            return c.batch_kernels(), [c.batch_results(p) for p in range(len(pairs))]
        finally:
            c.close()
            for k in env:
                monkeypatch.delenv(k)

    for k in {k for env, _ in VARIANTS for k in env}:
        monkeypatch.delenv(k, raising=False)
    base_k, base = run({})
    for env, kind in VARIANTS:
        kern, got = run(env)
        if kind == "bits":
            assert kern == base_k, env
            for p, (r, r0) in enumerate(zip(got, base)):
                assert_same_bits(r, r0, (env, p))
            continue
        if kind == "kernels":
            assert kern != base_k, ("the variant ran the default kernels", env, kern)
        else:
            assert kern == base_k, env
            forced = env["RH_FAR2"] == "1"
            for q, s in enumerate(seqs):
                r, r0, key = got[q // 2], base[q // 2], ("bp1", "bp2")[q % 2]
                changes = (len(s) < 384) == forced
                assert np.array_equal(r[key], r0[key]) != changes, (env, len(s), "changed form" if changes else "kept its form")
        for p, (r, r0) in enumerate(zip(got, base)):
            what = "%r pair %d" % (env, p)
            assert np.allclose(r["logZ"], r0["logZ"], rtol=0, atol=1e-10), what
            for key in ("bp1", "bp2", "hp"):
                assert_prob_close(r[key], r0[key], rel=1e-10, what="%s %s" % (key, what))
            for key in ("up1", "up2"):
                assert np.abs(r[key] - r0[key]).max() <= 1e-10, (key, what)


# ---- steps 3 and 4: the bench workload, 512 pairs of n = 500 (CONTRAfold model)
BENCH_PAIRS, BENCH_N = 512, 500


@pytest.fixture(scope="module")
def bench_ref(hotlib):
    """The bench batch computed once on one context: host copies of every pair's dense results and of the five candidate lists."""
    pairs = random_pairs(BENCH_PAIRS, BENCH_N, seed=12345)
    c = context()
    try:
        c.batch_upload(pairs)
        c.batch_compute()
        assert c.last_path() == 1 and c.batch_fallbacks(0) == [] and c.batch_fallbacks(2) == []
        res = c.batch_results_all()
        cands = {}
        for which, th in bench.SCANS:
            rec, first = c.batch_candidates_all(which, th)
            cands[which] = (rec.copy(), first.copy())
    finally:
        c.close()
    return pairs, res, cands


def test_bench_workload_n500(hotlib, opool, bench_ref):
    pairs, ref, cands = bench_ref
    dense = (0, 1, 2, 3, 4, 7, 255, 256, 511)   # 0-4: sequences on every residue mod 8 (every XCD slot of the pinned mapping)
    for p in dense:
        opool.inference(pairs[p][0]), opool.inference(pairs[p][1]), opool.duplex(*pairs[p])
    helix = "G" * 348 + "AAAA" + "C" * 348      # test_mixed_batch_only_the_flagged_problems_fall_back
    opool.inference(helix), opool.duplex(helix, pairs[300][1])
    assert pairs[0] == random_pair(500)

    # the five lists the bench returns == the reference's scans over the float-narrowed dense results, record for record
    for which, th in bench.SCANS:
        rec, first = cands[which]
        assert len(first) == BENCH_PAIRS + 1 and first[0] == 0 and first[-1] == len(rec) and len(rec) > 0, which
        for p in range(BENCH_PAIRS):
            i, j, pr = threshold_scans(ref[p], (which, th))
            mine = rec[first[p]:first[p + 1]]
            assert len(mine) == len(i), (which, p)
            assert np.array_equal(mine["i"], i) and np.array_equal(mine["j"], j) and np.array_equal(mine["p"], pr), (which, p)

    c = context()
    try:
        # the same upload computed again, then uploaded again and computed: the bits of the first compute (another context)
        c.batch_upload(pairs)
        for again in ("compute", "compute again", "upload again"):
            if again == "upload again":
                c.batch_upload(pairs)
            c.batch_compute()
            for p, r in enumerate(c.batch_results_all()):
                assert_same_bits(r, ref[p], (again, p))
        # unpinned sub-batches of 3 pairs (the last one of 2): every matrix of every pair bit-identical to the pinned batch
        for k in range(0, BENCH_PAIRS, 3):
            sub = pairs[k:k + 3]
            c.batch_upload(sub)
            c.batch_compute()
            for q, r in enumerate(c.batch_results_all()):
                assert_same_bits(r, ref[k + q], ("sub-batch", k + q))
        assert len(sub) == 2
        # one perfect GC helix in pair 300: only that sequence leaves the double range (held by the third scale exponent of the
        # linear path), at most the duplex of its pair with it; every other problem keeps its bits
        mixed = list(pairs)
        mixed[300] = (helix, pairs[300][1])
        c.batch_upload(mixed)
        c.batch_compute()
        assert c.last_path() == 3 and c.batch_fallbacks(2) == [600] and c.batch_fallbacks(0) == []
        assert set(c.batch_fallbacks(1) + c.batch_fallbacks(3)) <= {300}
        got = c.batch_results_all()
    finally:
        c.close()
    for p, r in enumerate(got):
        if p != 300:
            assert_same_bits(r, ref[p], ("pair next to the helix", p))
    r = got[300]
    assert np.array_equal(r["bp2"], ref[300]["bp2"]) and np.array_equal(r["up2"], ref[300]["up2"]) and r["logZ"][1] == ref[300]["logZ"][1]
    o1, od = opool.inference(helix).result(), opool.duplex(helix, pairs[300][1]).result()
    assert abs(r["logZ"][0] - o1["logZ"]) < 1e-7 * abs(o1["logZ"])
    assert_prob_close(r["bp1"], o1["post"], rel=REL, what="helix bp1 inside the bench batch")
    assert abs(r["logZ"][2] - od["logZ2"][0]) < 1e-7 * abs(od["logZ2"][0])
    assert_prob_close(r["hp"], od["post"], rel=REL, what="helix duplex inside the bench batch")

    for p in dense:
        s1, s2 = pairs[p]
        r = ref[p]
        o1, o2, od = (f.result() for f in (opool.inference(s1), opool.inference(s2), opool.duplex(s1, s2)))
        what = "bench pair %d" % p
        assert np.abs(r["logZ"] - np.array([o1["logZ"], o2["logZ"], od["logZ2"][0]])).max() < 1e-8, what
        assert_prob_close(r["bp1"], o1["post"], rel=REL, what="bp1 " + what)
        assert_prob_close(r["bp2"], o2["post"], rel=REL, what="bp2 " + what)
        assert_prob_close(r["hp"], od["post"], rel=REL, what="hp " + what)
        for s, key, ukey in ((s1, "bp1", "up1"), (s2, "bp2", "up2")):
            ref_up = opool.cf.up_float(len(s), r[key].astype(np.float32))
            assert np.abs(r[ukey].astype(np.float32) - ref_up).max() < 2e-6, (what, ukey)


def test_two_contexts_two_threads_as_the_bench_runs(hotlib, bench_ref):
    """bench.py's timed loop: two contexts on one GPU, steps alternating between them on two host threads.  Both contexts' candidate
    lists of their last step and their dense results are the bits of the single-context computation."""
    pairs, ref, cands = bench_ref
    ctxs = []
    try:
        ctxs = [context() for _ in range(2)]
        for c in ctxs:
            c.batch_upload(pairs)   # tables allocated, launch graphs captured: outside the loop, as bench.py does
            c.batch_compute()
        last = [{}, {}]

        def body(c, p, k):
            bench.step_candidates(c, p, keep=last[ctxs.index(c)])   # each thread keeps its own last step's lists

        bench.timed_steps(ctxs, pairs, 4, body, lambda: None)
        for t, c in enumerate(ctxs):
            for which, name in enumerate(bench.SCAN_NAMES):
                rec, first = last[t][name]
                rec0, first0 = cands[which]
                assert np.array_equal(first, first0) and np.array_equal(rec, rec0), (t, name)
            for p, r in enumerate(c.batch_results_all()):
                assert_same_bits(r, ref[p], ("context %d" % t, p))
    finally:
        for c in ctxs:
            c.close()


# ---- step 5: n = 2000, the --full shape (64 pairs, 128 pinned sequences)
def test_n2000_batch_of_64(hotlib, golden):
    pairs = random_pairs(64, 2000, seed=12345)
    assert pairs[0] == random_pair(2000)
    alone = (0, 1, 3, 4, 63)
    c = context()
    try:
        c.batch_upload(pairs)
        c.batch_compute()
        assert c.last_path() == 1
        kept = {}
        for p, (s1, s2) in enumerate(pairs):
            r = c.batch_results(p)
            if p == 0:
                check_n2000_golden(r, golden)
            check_pair_properties(s1, s2, r)
            if p in alone:
                kept[p] = r
        for p in alone:
            c.batch_upload([pairs[p]])
            c.batch_compute()
            assert_same_bits(c.batch_results(0), kept[p], ("alone", p))
    finally:
        c.close()


# ---- step 6: Vienna-BL at the --full shapes (256 pairs of n = 500; hp from co_pf_fold or from pf_duplex)
@pytest.mark.parametrize("cofold", [True, False], ids=["cofold", "duplex"])
def test_vienna_bl_full_batch(hotlib, opool, cofold):
    import ractip_amd
    pairs = random_pairs(256, 500, seed=12345)
    dense = (0, 1, 2, 3, 4, 255)
    for p in dense:
        s1, s2 = pairs[p]
        opool.mccaskill(s1), opool.mccaskill(s2), (opool.cofold if cofold else opool.pf_duplex)(s1, s2)
    c = context(ractip_amd.hot.RH_MODEL_VIENNA_BL)
    try:
        c.set_hybrid(cofold)
        assert c.max_w == 15
        c.batch_upload(pairs)
        c.batch_compute()
        ref = c.batch_results_all()
        # unpinned sub-batches of 3 pairs (the last one of 1): the same longest length, the same bits
        for k in range(0, len(pairs), 3):
            c.batch_upload(pairs[k:k + 3])
            c.batch_compute()
            for q, r in enumerate(c.batch_results_all()):
                assert_same_bits(r, ref[k + q], ("sub-batch", cofold, k + q))
    finally:
        c.close()
    for p in dense:
        s1, s2 = pairs[p]
        r = ref[p]
        o1, o2 = opool.mccaskill(s1).result(), opool.mccaskill(s2).result()
        what = "vienna pair %d (%s)" % (p, "cofold" if cofold else "duplex")
        for o, key, ukey, kz in ((o1, "bp1", "up1", 0), (o2, "bp2", "up2", 1)):
            assert abs(r["logZ"][kz] - o["logZ"]) < 1e-9 * abs(o["logZ"]), (what, key)
            assert_prob_close(r[key], o["post"], rel=REL, what="%s %s" % (key, what))
            assert_prob_close(r[ukey], o["up"], rel=REL, abs_floor=1e-11, what="%s %s" % (ukey, what))
        if cofold:
            oc = opool.cofold(s1, s2).result()
            zh, hp = oc["logZ"], oc["hp"]
        else:
            od = opool.pf_duplex(s1, s2).result()
            zh, hp = od["logZ"], od["pr"]
        assert abs(r["logZ"][2] - zh) < 1e-9 * abs(zh), what
        assert_prob_close(r["hp"], hp, rel=REL, what="hp " + what)


def test_vienna_bl_default_helper_threshold(hotlib, monkeypatch):
    """The per-pair route of the scale-exponent ladder under its DEFAULT threshold (a helper context recomputes the flagged pairs when
    at most one pair in 16 is flagged): one chain of stable hairpins among 32 pinned pairs of n = 500.  Only its pair is flagged,
    the other 31 keep the bits of a batch that holds a random 900-mer in the same slot (the same longest length), and the chain's
    pair equals the whole-batch route's (RH_PAIR_HELPER=0)."""
    import ractip_amd
    monkeypatch.delenv("RH_PAIR_HELPER", raising=False)
    rng = np.random.default_rng(9)
    plain = random_pairs(32, 500, seed=12345)
    K = 13
    base = list(plain)
    base[K] = (rnd(rng, 900), plain[K][1])
    mixed = list(plain)
    mixed[K] = (hairpins(rng, 900), plain[K][1])

    def run(pairs, env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = context(ractip_amd.hot.RH_MODEL_VIENNA_BL)
        try:
            c.set_hybrid(True)
            c.batch_upload(pairs)
            c.batch_compute()
            return c.last_path(), c.batch_fallbacks(2), c.batch_fallbacks(0), c.batch_results_all()
        finally:
            c.close()
            for k in env:
                monkeypatch.delenv(k)

    path0, resc0, logd0, b = run(base, {})
    assert path0 == 1 and resc0 == [] and logd0 == []
    path, resc, logd, res = run(mixed, {})
    assert path == 3 and sorted(resc + logd) == [2 * K, 2 * K + 1]   # the one pair, whichever mechanism held it on the helper
    _, _, _, whole = run(mixed, {"RH_PAIR_HELPER": "0"})
    for p in range(len(plain)):
        if p != K:
            assert_same_bits(res[p], b[p], ("pair next to the chain", p))
    r, r0 = res[K], whole[K]
    assert np.allclose(r["logZ"], r0["logZ"], rtol=1e-9, atol=0)
    for key in ("bp1", "bp2", "hp"):
        assert_prob_close(r[key], r0[key], rel=REL, what="%s of the recomputed pair" % key)
    for key in ("up1", "up2"):
        assert_prob_close(r[key], r0[key], rel=REL, abs_floor=1e-11, what="%s of the recomputed pair" % key)
