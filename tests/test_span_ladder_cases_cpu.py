"""What tests/test_gpu_span_ladder.py rests on, from the plain double-precision oracles alone (no GPU): the zone of every case's
designated cell against both thresholds (1e-280 and the smallest double) on every exponent its ladder meets, that each length is
the smallest that meets its condition, the enumeration against the DP oracle on shortened copies of each family, the factorised
identities the expected values use, and what each reference of a GPU test costs."""
import math
import time

import numpy as np
import pytest

import _contrafold_weights as cw
import _span_acc_cases as ac
import _span_cases as sc
import _span_ladder_cases as lc
from _oracle import Oracle, tri_offset

TOL = 1e-12


def lone_ln_q(d):
    return lc.ln_q(sc.masked(lc.lone(d), d + 1, bruteforce=True), d)


# ---- Vienna-BL: zones
def test_the_zones_do_not_touch():
    assert lc.LN_ZERO - lc.HOLE_MARGIN < lc.LN_ZERO + lc.MARGIN < lc.LN_TINY - lc.MARGIN < lc.LN_TINY + lc.MARGIN < lc.LN_HUGE - lc.MARGIN
    assert [lc.zone(x) for x in (700.0, 0.0, -690.0, -770.0)] == ["huge", "in range", "flagged-tiny", "hole"]
    assert [lc.zone(x) for x in (650.0, -650.0, -720.0, -750.0)] == [None] * 4
    assert 5e-324 > 0.0 and 5e-324 / 2.0 == 0.0 and math.exp(lc.LN_ZERO - lc.HOLE_MARGIN) == 0.0


def test_lone_flag_is_flagged_tiny_on_the_default_exponent_and_held_by_zero():
    c = lc.LONE_FLAG
    q = lone_ln_q(c.d)
    print("LONE_FLAG d = %d: ln Q %.4f, scaled %s" % (c.d, q, [round(q - s * c.d, 1) for s in lc.BL_LADDER]))
    assert c.L == len(c.seq) == c.d + 1
    assert lc.zones(q, c.d, lc.BL_LADDER) == ("flagged-tiny", "hole", "hole", "in range")
    assert lc.zone(lone_ln_q(c.d - 1) - 0.28 * (c.d - 1)) is None, "one letter less is not flagged-tiny by the margin"


def test_lone_hole_is_a_hole_on_every_positive_exponent():
    c = lc.LONE_HOLE
    q = lone_ln_q(c.d)
    print("LONE_HOLE d = %d: ln Q %.4f, scaled %s" % (c.d, q, [round(q - s * c.d, 1) for s in lc.BL_LADDER]))
    assert lc.zones(q, c.d, lc.BL_LADDER) == ("hole", "hole", "hole", "in range")
    assert lc.zone(lone_ln_q(c.d - 1) - 0.28 * (c.d - 1)) is None


def test_multi_hole_closes_a_multiloop_that_holds_all_the_weight():
    c = lc.MULTI_HOLE
    n = len(c.seq)
    whole, below = sc.masked(c.seq, n, bruteforce=True), sc.masked(c.seq, n - 1, bruteforce=True)
    less = sc.masked(lc.multi(lc.TAIL_MULTI_HOLE - 100), n - 100, bruteforce=True)
    b = lc.multi_bonus(less["logZ"], lc.TAIL_MULTI_HOLE - 100, whole["logZ"], lc.TAIL_MULTI_HOLE)
    q = lc.ln_q(whole, c.d)
    print("MULTI_HOLE n = %d: log Z %.6f (L = n), %.6f (L = n - 1), P(closing) %.12f, bonus %.6f a letter, scaled %s"
          % (n, whole["logZ"], below["logZ"], whole["band"][0, c.d], b, [round(q - s * c.d, 1) for s in lc.BL_LADDER]))
    assert whole["band"][0, c.d] > 1.0 - 1e-9 and whole["logZ"] - below["logZ"] > 80.0
    assert 0.03 < b < 0.035, "an unpaired multiloop letter has a bonus under BL*"
    assert lc.zones(q, c.d, lc.BL_LADDER) == ("hole", "hole", "hole", "in range")
    assert lc.zone(q + (0.28 - b) - 0.28 * c.d) is None, "one tail letter less is not a hole by the margin"
    # at L = n - 1 the last C still pairs with the G's of the hairpins, tail and more apart: hairpin-only cells, holes on 0.28
    far = below["band"][10:20, lc.TAIL_MULTI_HOLE:]
    assert far.max() > 1e-9, "pairs a first attempt that passes for clean would drop, above the floor of 1e-12"
    assert 1.0 < below["logZ"] < 2.0


def test_the_far_cell_of_the_exhaustion_cases():
    """the lone pair behind the chain: its cell is the lone sequence's (the same letters enclosed).  The chain itself is pinned by
    the GPU test against Context.fold, as the existing ladder tests do (the DP takes 25 s at 1300 letters); here an estimate from a
    fifth of it."""
    for c, want in ((lc.EXHAUST_FLAG, ("in range", "flagged-tiny", "hole", "in range")), (lc.EXHAUST_HOLE, ("in range", "hole", "hole", "in range"))):
        q = lone_ln_q(c.d)
        print("%s d = %d: ln Q %.4f, scaled %s" % (c.name, c.d, q, [round(q - s * c.d, 1) for s in lc.BL_LADDER]))
        assert lc.zones(q, c.d, lc.BL_LADDER) == want
        assert lc.zone(lone_ln_q(c.d - 1) - 0.7 * (c.d - 1)) is None
        assert c.L == lc.BL_CHAIN > c.d + 1 and c.seq.endswith("AAAAA" + lc.lone(c.d)) and len(c.seq) == lc.BL_CHAIN + 5 + c.d + 1
    z260 = sc.masked(lc.hairpin_chain(260), None)["logZ"]
    print("chain: log Z %.3f at 260 letters, %.3f a letter" % (z260, z260 / 260))
    assert 5 * z260 - 0.28 * lc.BL_CHAIN > lc.LN_HUGE + 50.0


def test_the_constrained_twin_is_the_empty_ensemble():
    seq = lc.LONE_FLAG.seq
    assert len(lc.TWIN_CONSTRAINT) == len(seq) and lc.TWIN_CONSTRAINT.count("x") == 1 and seq[-1] == "C"
    r = sc.oracle().fold_bruteforce(seq, 1, constraint=lc.TWIN_CONSTRAINT)
    assert r["logZ"] == 0.0 and not r["post"].any() and (r["up"] == 1.0).all()


# ---- identities and the enumeration against the DP
@pytest.mark.parametrize("d", [lc.D_EXHAUST_FLAG, lc.D_LONE_HOLE])
def test_the_lone_pair_factorises(d):
    r = ac.masked_acc(lc.lone(d), d + 1, lc.ACC_W, bruteforce=True)
    p = r["band"][0, d]
    w = p / (1.0 - p)
    assert abs(r["logZ"] - math.log1p(w)) < TOL and abs(lc.ln_q(r, d) - math.log(w)) < 1e-9
    band = np.zeros((d + 1, d + 1))
    band[0, d] = p
    assert (r["band"] == band).all()
    up = np.ones((d + 1, lc.ACC_W))
    for k in range(lc.ACC_W):
        up[0, k] = up[d - k, k] = 1.0 - p                    # the runs that hold the first or the last letter
        up[d + 1 - k:, k] = 0.0                              # ... and those that pass the end
    assert np.abs(r["up"] - up).max() < TOL


@pytest.mark.parametrize("seq", [lc.lone(300), lc.multi(300)], ids=["lone", "multi"])
def test_enumeration_equals_the_dp_oracle_on_shortened_copies(seq):
    n = len(seq)
    for L in (n, n - 1):
        e, o = ac.masked_acc(seq, L, lc.ACC_W, bruteforce=True), ac.masked_acc(seq, L, lc.ACC_W)
        assert abs(e["logZ"] - o["logZ"]) < TOL * max(1.0, abs(o["logZ"]))
        assert np.abs(e["band"] - o["band"]).max() < TOL and np.abs(e["up"] - o["up"]).max() < TOL
        e1 = sc.masked(seq, L, bruteforce=True)
        assert e1["logZ"] == e["logZ"] and (e1["band"] == e["band"]).all() and np.abs(e1["up"][:, 0] - e["up"][:, 0]).max() < TOL
    assert sc.masked(lc.multi(300), 321, bruteforce=True)["band"][0, 320] > 0.9, "the multiloop already holds most of the weight"


def test_what_the_references_of_the_gpu_tests_cost():
    """under 2 s each: CPU time of this process, the best of up to three runs, since a busy machine slows a run down and never
    speeds it up (the values themselves are computed once per session and shared)"""
    vo = sc.oracle()
    for c in lc.DESCENT:
        mask = sc.band_mask(len(c.seq), c.L)
        for max_w in (1, lc.ACC_W):
            best = float("inf")
            for _ in range(3):
                vo.L.vo_set_allow_mask(mask.ctypes.data)
                try:
                    t = time.process_time()
                    vo._fold_bruteforce(c.seq, max_w)
                    best = min(best, time.process_time() - t)
                finally:
                    vo.L.vo_set_allow_mask(None)
                if best < 2.0:
                    break
            print("%s max_w %d: %.2f s" % (c.name, max_w, best))
            assert best < 2.0


# ---- CONTRAfold
@pytest.fixture(scope="module")
def custom(tmp_path_factory):
    return Oracle(cw.write(tmp_path_factory.mktemp("ladder") / "custom.params", lc.cf_custom_rows()))


def test_the_custom_file_case_is_a_hole_on_the_default_exponent_and_held_by_zero(custom):
    c = lc.CF_HOLE
    S = lc.cf_pair_weight(custom)
    print("CF_HOLE d = %d: S %.4f, scaled %s" % (c.d, S, [round(S - s * c.d, 1) for s in lc.CF_LADDER]))
    assert lc.zones(S, c.d, lc.CF_LADDER) == ("hole", "hole", "hole", "in range")
    assert lc.zone(S - 0.12 * (c.d - 1)) is None
    # S does not depend on d from 31 on, and it is linear in the changed row
    for d in (31, 40, 77):
        n = d + 1
        r = custom.inference(lc.lone(d))
        assert abs(r["logZ"] + math.log(r["post"][tri_offset(n, 1) + n]) - S) < 1e-9
    rows = [(name, v - 100.0 if name == "hairpin_length_at_least_30" else v) for name, v in lc.cf_custom_rows()]
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert abs(lc.cf_pair_weight(Oracle(cw.write(tmp + "/moved.params", rows))) - (S - 100.0)) < 1e-9


def test_the_closed_form_is_the_oracle_at_full_length(custom):
    c = lc.CF_HOLE
    n = len(c.seq)
    want = lc.cf_closed_form(lc.cf_pair_weight(custom), c.d)
    t = time.process_time()
    r = custom.inference(c.seq)
    print("cfo_inference at %d letters: %.1f s; log Z %.6f, P %.6f" % (n, time.process_time() - t, r["logZ"], want["band"][0, c.d]))
    assert abs(r["logZ"] - want["logZ"]) < 1e-9 * abs(want["logZ"])
    band = sc.tri_to_band(r["post"], n, n)
    assert np.abs(band - want["band"]).max() < 1e-9 and 0.9 < want["band"][0, c.d] < 0.99, "a probability that is neither 0 nor 1"
    up = 1.0 - band.sum(axis=1) - np.array([sum(band[i - d, d] for d in range(1, i + 1)) for i in range(n)])
    assert np.abs(up - want["up"][:, 0]).max() < 1e-9


def test_the_contrafold_exhaustion_cases():
    o = Oracle()
    S = lc.cf_pair_weight(o)
    for c, want in ((lc.CF_EXHAUST_FLAG, ("in range", "flagged-tiny", "hole", "in range")), (lc.CF_EXHAUST_HOLE, ("in range", "hole", "hole", "in range"))):
        print("%s d = %d: S %.4f, scaled %s" % (c.name, c.d, S, [round(S - s * c.d, 1) for s in lc.CF_LADDER]))
        assert lc.zones(S, c.d, lc.CF_LADDER) == want
        assert lc.zone(S - 0.45 * (c.d - 1)) is None
        assert c.L >= lc.CF_CHAIN and c.L > c.d and len(c.seq) == lc.CF_CHAIN + 5 + c.d + 1
    # the chain: an estimate from a sixth of it (the DP takes 46 s at 1560 letters: 949.697); the GPU test asserts it on Context.fold
    z260 = o.inference(lc.hairpin_chain(260))["logZ"]
    print("chain: log Z %.3f at 260 letters, %.3f a letter" % (z260, z260 / 260))
    assert 6 * z260 - 0.12 * lc.CF_CHAIN > lc.LN_HUGE + 50.0, "huge on 0.12 and on 0.0"
    assert lc.zone(6 * z260 - 0.45 * lc.CF_CHAIN) == "in range", "the chain alone answers from 0.45"
