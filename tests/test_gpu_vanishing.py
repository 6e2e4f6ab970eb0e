"""GPU suite: the scale-exponent ladders driven DOWNWARDS.  Every other test of the ladders makes Z~ overflow (chains of hairpins, GC
helices, complementary strands); here Z~ VANISHES: a short structured insert in long poly-A flanks (tests/_vanishing_cases.py), whose
reference is the plain double-precision oracle on a 96-letter sequence (identities and the position of every case relative to the
flag threshold: tests/test_vanishing_cases_cpu.py).  Duplex cases are compared with the oracle on the full pair.
Bars: bp / hp 1e-6 relative above 1e-12; log Z 1e-9 * max(1, |log Z|); CONTRAfold up: the float restatement at 2e-6; Vienna-BL up:
1e-6 relative above 1e-11; "keeps its bits": np.array_equal.
Every batch is computed once, by a module fixture; the tests each check one aspect of it."""
import contextlib
import os
import sys

import numpy as np
import pytest

import _vanishing_cases as vc
from _oracle import NEG, OraclePool, assert_prob_close
from ractip_amd.seqgen import random_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import vienna2x as v2  # noqa: E402

pytestmark = pytest.mark.gpu
REL = 1e-6
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")
L = len(vc.INSERT)
SHORT2 = vc.short_of(vc.INSERT2)


@contextlib.contextmanager
def switches(env):
    """environment switches a context reads when it is created or computes"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    yield p
    p.close()


@pytest.fixture(scope="module")
def refs(opool):
    """the short sequences' oracle results every embedded reference is made of"""
    s = vc.short_of(vc.INSERT)
    return dict(cf=opool.inference(s).result(), bl=opool.mccaskill(s, vc.MAX_W).result(), bl2=opool.mccaskill(SHORT2, vc.MAX_W).result(),
                co=opool.cofold(s, SHORT2).result(), B=vc.cf_flank_letter(opool.cf), n=len(s))


def logz_close(z, ref):
    return abs(z - ref) <= 1e-9 * max(1.0, abs(ref))


def rnd(rng, n):
    return "".join(rng.choice(list("ACGU"), n))


def ordinary_pairs():
    return random_pairs(6, 300, seed=4242)        # the shapes of test_after_an_overflow


def compute(c, pairs, keep=None):
    c.batch_upload(pairs)
    c.batch_compute()
    return {p: c.batch_results(p) for p in (range(len(pairs)) if keep is None else keep)}


def run_on(c, pairs, keep=None, then=None):
    """the batch on context c (closed here), then -- reused tables -- the batch `then` on the same context"""
    try:
        res = compute(c, pairs, keep)
        out = dict(res=res, path=c.last_path(), hpath=c.last_hybrid_path(), fb=[c.batch_fallbacks(w) for w in range(4)])
        if then is not None:
            out["then"] = compute(c, then)
        return out
    finally:
        c.close()


def run_cf(pairs, env, keep=None, then=None):
    import ractip_amd
    with switches(env):
        return run_on(ractip_amd.Context(device=0), pairs, keep, then)


def vbl(hybrid, mode=0):
    import ractip_amd
    c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL)
    c.set_mode(mode)
    c.set_hybrid(hybrid)
    c.set_max_w(vc.MAX_W)
    return c


def run_bl(pairs, env, hybrid, then=None, mode=0):
    with switches(env):
        return run_on(vbl(hybrid, mode), pairs, None, then)


def assert_same_bits(got, want, what):
    for p in want:
        for k in KEYS:
            assert np.array_equal(got[p][k], want[p][k]), (what, p, k)


def check_fold_bp(r, which, case, ref, what):
    bp = r[("bp1", "bp2")[which]]
    assert_prob_close(bp, vc.embed_bp(ref["post"], L, case.f5, case.f3), rel=REL, what="bp " + what)
    assert bp[~vc.insert_block_mask(L, case.f5, case.f3)].max() <= 1e-12, what       # nothing outside the insert
    return bp


def check_cf_fold(r, which, case, refs, oracle):
    """one CONTRAfold fold case against the embedded reference"""
    what = "cf %s %s n = %d" % (case.label, case.where, case.n)
    z, want_z = r["logZ"][which], refs["cf"]["logZ"] + refs["B"] * (case.n - refs["n"])
    assert logz_close(z, want_z), (what, z, want_z)
    bp = check_fold_bp(r, which, case, refs["cf"], what)
    up = np.asarray(r[("up1", "up2")[which]]).ravel()
    assert np.abs(up.astype(np.float32) - oracle.up_float(case.n, bp.astype(np.float32))).max() < 2e-6, what
    flank = np.r_[0:case.f5, case.f5 + L:case.n]
    assert np.abs(up[flank] - 1.0).max() < 2e-6 and up[case.f5:case.f5 + L].min() < 0.9, what


def check_bl_fold(r, which, case, refs):
    what = "bl %s %s n = %d" % (case.label, case.where, case.n)
    assert logz_close(r["logZ"][which], refs["bl"]["logZ"]), (what, r["logZ"][which], refs["bl"]["logZ"])
    check_fold_bp(r, which, case, refs["bl"], what)
    up, want = np.asarray(r[("up1", "up2")[which]]), vc.embed_up(refs["bl"]["up"], L, case.f5, case.f3)
    assert_prob_close(up, want, rel=REL, abs_floor=1e-11, what="up " + what)
    far = max(0, case.f5 - vc.FLANK - vc.MAX_W)
    assert (want[:far] == 1.0).all() and (far == 0 or np.abs(up[:far] - 1.0).max() <= REL), what   # up is 1 in the flanks


def check_bl_short(r, which, seq, opool, what):
    o = opool.mccaskill(seq, vc.MAX_W).result()
    assert logz_close(r["logZ"][which], o["logZ"]), what
    assert_prob_close(r[("bp1", "bp2")[which]], o["post"], rel=REL, what="bp " + what)
    assert_prob_close(r[("up1", "up2")[which]], o["up"], rel=REL, abs_floor=1e-11, what="up " + what)


def check_against_the_log_space_context(r, r0, what):
    assert np.allclose(r["logZ"], r0["logZ"], rtol=1e-9, atol=0), what
    for k in ("bp1", "bp2", "hp"):
        assert_prob_close(r[k], r0[k], rel=REL, what="%s of %s against the log-space context" % (k, what))
    for k in ("up1", "up2"):
        assert_prob_close(r[k], r0[k], rel=REL, abs_floor=1e-11, what="%s of %s against the log-space context" % (k, what))


# =================================================================================== CONTRAfold folds
# Three n = 3950 sequences (insert at the 5' end, in the middle, at the 3' end: ln Z~ = -505 on s = 0.12) and one n = 3200 sequence
# (-408: inside) among ordinary short ones, in one batch
CF_VANISHING = {"5'": 0, "mid": 5, "3'": 8}       # where the insert sits -> sequence index (2p = s1 of pair p)
CF_INSIDE = 10
CF_ORDINARY = (1, 3, 6, 7)                        # pairs of ordinary short sequences
CF_RUNS = ("ladder", "log")


def cf_fold_batch(with_the_long_ones=True):
    rng = np.random.RandomState(31)
    short = [rnd(rng, n) for n in (90, 120, 60, 100)]
    ordinary = [(rnd(rng, a), rnd(rng, b)) for a, b in ((300, 280), (64, 65), (150, 97), (41, 200))]
    if with_the_long_ones:
        van = {w: vc.fold_case("cf", "vanishing", w, vc.CF_N_VANISHING) for w in vc.POSITIONS}
        longs = [van["5'"].seq, van["mid"].seq, van["3'"].seq, vc.fold_case("cf", "inside", "mid", vc.CF_N_INSIDE).seq]
    else:                                         # random letters of the same lengths: the same nmax, nothing vanishes
        longs = [rnd(rng, n) for n in (vc.CF_N_VANISHING,) * 3 + (vc.CF_N_INSIDE,)]
    return [(longs[0], short[0]), ordinary[0], (short[1], longs[1]), ordinary[1], (longs[2], short[2]), (longs[3], short[3]), ordinary[2], ordinary[3]]


@pytest.fixture(scope="module")
def cf_fresh_ordinary(hotlib):
    return run_cf(ordinary_pairs(), {})["res"]


@pytest.fixture(scope="module")
def cf_ladder(hotlib, opool):
    for s1, s2 in cf_fold_batch():          # (queued here, the oracle runs beside the GPU)
        opool.duplex(s1, s2)
        for s in (s1, s2):
            if len(s) < vc.CF_N_INSIDE:
                opool.inference(s)
    return run_cf(cf_fold_batch(), {}, then=ordinary_pairs())


@pytest.fixture(scope="module")
def cf_log(hotlib):
    return run_cf(cf_fold_batch(), {"RH_SCALE_LADDER": "0"}, then=ordinary_pairs())


@pytest.fixture(scope="module")
def cf_without(hotlib):
    return run_cf(cf_fold_batch(False), {}, keep=CF_ORDINARY)


@pytest.fixture(params=CF_RUNS)
def cf_run(request):
    return request.getfixturevalue("cf_" + request.param)


def test_contrafold_folds_that_vanish_are_held_by_the_exponent_zero(cf_ladder):
    """the vanishing sequences are recomputed on the linear kernels with s = 0 (rh_batch_fallbacks which = 2); nothing goes to log
    space; the n = 3200 sequence is in neither list"""
    assert cf_ladder["path"] == 3 and cf_ladder["fb"][2] == sorted(CF_VANISHING.values()) and cf_ladder["fb"][0] == []


def test_contrafold_folds_that_vanish_without_the_ladder_go_to_log_space(cf_log):
    assert cf_log["path"] == 3 and cf_log["fb"][0] == sorted(CF_VANISHING.values()) and cf_log["fb"][2] == []


@pytest.mark.parametrize("where", vc.POSITIONS)
def test_contrafold_vanishing_fold_equals_the_embedded_reference(cf_run, refs, opool, where):
    sq = CF_VANISHING[where]
    check_cf_fold(cf_run["res"][sq // 2], sq % 2, vc.fold_case("cf", "vanishing", where, vc.CF_N_VANISHING), refs, opool.cf)


def test_contrafold_fold_inside_the_range_equals_the_embedded_reference(cf_run, refs, opool):
    check_cf_fold(cf_run["res"][CF_INSIDE // 2], CF_INSIDE % 2, vc.fold_case("cf", "inside", "mid", vc.CF_N_INSIDE), refs, opool.cf)


@pytest.mark.parametrize("p", range(len(cf_fold_batch())))
def test_contrafold_short_sequences_and_duplexes_next_to_the_vanishing_folds(cf_run, opool, p):
    """every other dense result of the batch against the oracle; the duplexes of the long sequences (L1 + L2 about 4000) vanish on
    every exponent but 0"""
    s1, s2 = cf_fold_batch()[p]
    r, od = cf_run["res"][p], opool.duplex(s1, s2).result()
    assert logz_close(r["logZ"][2], od["logZ2"][0]), p
    assert_prob_close(r["hp"], od["post"], rel=REL, what="hp of pair %d" % p)
    for which, s in enumerate((s1, s2)):
        if len(s) < vc.CF_N_INSIDE:
            o = opool.inference(s).result()
            assert logz_close(r["logZ"][which], o["logZ"]), (p, which)
            assert_prob_close(r[("bp1", "bp2")[which]], o["post"], rel=REL, what="bp of sequence %d" % (2 * p + which))


def test_contrafold_ordinary_pairs_keep_their_bits_next_to_vanishing_folds(cf_run, cf_without):
    """... the bits of a batch of the same nmax without the long ones"""
    assert_same_bits(cf_run["res"], cf_without["res"], "ordinary pairs next to the vanishing sequences")


def test_contrafold_tables_are_reusable_after_vanishing_folds(cf_run, cf_fresh_ordinary):
    assert_same_bits(cf_run["then"], cf_fresh_ordinary, "ordinary batch after the vanishing one")


# ---- both directions in one batch: one vanishing sequence (held by s = 0) and one chain of stable hairpins (overflow on s = 0.12,
# held by s = 0.45)
def both_directions_batch():
    rng = np.random.default_rng(5)
    comp = {"G": "C", "C": "G"}

    def hairpins(n):
        s = ""
        while len(s) < n:
            stem = "".join(rng.choice(list("GC"), size=10))
            s += stem + "AAAA" + "".join(comp[ch] for ch in reversed(stem)) + "AA"
        return s[:n]
    rs = np.random.RandomState(32)
    case = vc.fold_case("cf", "vanishing", "mid", vc.CF_N_VANISHING)
    return case, [(case.seq, rnd(rs, 80)), (hairpins(1100), rnd(rs, 70)), (rnd(rs, 200), rnd(rs, 210)), (rnd(rs, 150), rnd(rs, 100))]


@pytest.fixture(scope="module")
def both_directions(hotlib, opool):
    pairs = both_directions_batch()[1]
    for p in (2, 3):
        opool.inference(pairs[p][0]), opool.inference(pairs[p][1])
    return run_cf(pairs, {}, then=ordinary_pairs())


def test_contrafold_both_directions_each_held_by_its_own_rung(both_directions, refs, opool, cf_fresh_ordinary):
    assert both_directions["path"] == 3 and both_directions["fb"][2] == [0, 2] and both_directions["fb"][0] == []
    assert_same_bits(both_directions["then"], cf_fresh_ordinary, "ordinary batch after both directions")
    check_cf_fold(both_directions["res"][0], 0, both_directions_batch()[0], refs, opool.cf)


def test_contrafold_both_directions_the_chain_equals_the_log_space_path(both_directions):
    """as in test_scale_exponent_ladder"""
    log = run_cf(both_directions_batch()[1][1:2], {"RH_SCALE_LADDER": "0"})
    assert log["fb"][0] == [0] and log["fb"][2] == []
    r, r0 = both_directions["res"][1], log["res"][0]
    assert abs(r["logZ"][0] - r0["logZ"][0]) < 1e-9 * abs(r0["logZ"][0]) and r0["logZ"][0] - vc.CF_S * 1100 > vc.LN_HI
    assert_prob_close(r["bp1"], r0["bp1"], rel=REL, what="the chain of hairpins next to a vanishing sequence")
    assert np.abs(r["up1"] - r0["up1"]).max() < 1e-9


def test_contrafold_both_directions_the_ordinary_sequences(both_directions, opool):
    pairs = both_directions_batch()[1]
    for p in (2, 3):
        for which in (0, 1):
            o = opool.inference(pairs[p][which]).result()
            assert logz_close(both_directions["res"][p]["logZ"][which], o["logZ"])
            assert_prob_close(both_directions["res"][p][("bp1", "bp2")[which]], o["post"], rel=REL, what="ordinary sequence of pair %d" % p)


# =================================================================================== CONTRAfold duplex
# a + b = 1100 (ln Z~ = -647 on s = 0.65, -262 on 0.3), a + b = 2000 (-540 on 0.3, held by 0) and one U in poly-A against poly-A
# (terms exist and their sum underflows) walk through 1.3 and 2.2, where every value is exactly 0, down to the rung that holds them;
# the a + b = 700 pair (-384) stays; a pair without a complementary letter keeps the sentinel
DX_INSIDE, DX_BY_03, DX_BY_0, DX_ONE, DX_NONE = 1, 3, 5, 6, 8
DX_RESCALED = [DX_BY_03, DX_BY_0, DX_ONE]


def cf_duplex_batch(with_the_vanishing_ones=True):
    rng = np.random.RandomState(33)
    ordinary = [(rnd(rng, a), rnd(rng, b)) for a, b in ((300, 280), (120, 400), (64, 64), (200, 210))]
    cases = {c.label: (c.s1, c.s2) for c in vc.duplex_cases() if c.model == "cf"}
    pairs = [ordinary[0], cases["inside"], ordinary[1], cases[0.3], ordinary[2], cases[0.0], vc.DX_ONE_PAIR, ordinary[3], vc.DX_NO_PAIR]
    if not with_the_vanishing_ones:               # random letters of the same lengths (log Z 0.6 per unit of a + b: inside)
        for p in DX_RESCALED:
            pairs[p] = (rnd(rng, len(pairs[p][0])), rnd(rng, len(pairs[p][1])))
    return pairs


@pytest.fixture(scope="module")
def dx_run(hotlib, opool):
    pairs = cf_duplex_batch()
    for s1, s2 in pairs:
        opool.duplex(s1, s2)
    return run_cf(pairs, {}, then=ordinary_pairs())


def test_contrafold_duplex_pairs_that_vanish_walk_down_the_ladder(dx_run):
    """rh_batch_fallbacks which = 3, not 1; the inside pair and the pair without a complementary letter are not flagged"""
    assert dx_run["fb"][3] == DX_RESCALED and dx_run["fb"][1] == [] and dx_run["hpath"] == 3


@pytest.mark.parametrize("p", range(len(cf_duplex_batch())))
def test_contrafold_duplex_equals_the_oracle_on_the_full_pair(dx_run, opool, p):
    s1, s2 = cf_duplex_batch()[p]
    od, r = opool.duplex(s1, s2).result(), dx_run["res"][p]
    if p == DX_NONE:      # no complementary letter: the -2e20 sentinel and a zero hp
        assert r["logZ"][2] <= NEG / 2 and od["logZ2"][0] <= NEG / 2 and not r["hp"].any()
        return
    assert logz_close(r["logZ"][2], od["logZ2"][0]), (r["logZ"][2], od["logZ2"][0])
    assert_prob_close(r["hp"], od["post"], rel=REL, what="hp of duplex pair %d" % p)


def test_contrafold_duplex_pairs_keep_their_bits_next_to_vanishing_ones(dx_run):
    others = [p for p in range(len(cf_duplex_batch())) if p not in DX_RESCALED]
    assert_same_bits(dx_run["res"], run_cf(cf_duplex_batch(False), {}, keep=others)["res"], "pairs next to the vanishing duplexes")


def test_contrafold_tables_are_reusable_after_vanishing_duplexes(dx_run, cf_fresh_ordinary):
    assert_same_bits(dx_run["then"], cf_fresh_ordinary, "ordinary batch after the vanishing duplexes")


# =================================================================================== Vienna-BL folds and accessibility
@pytest.fixture(scope="module")
def bl_fresh_ordinary(hotlib):
    return {hybrid: run_bl(ordinary_pairs(), {}, hybrid)["res"] for hybrid in (False, True)}


# ---- whole-batch route: three n = 1900 sequences (ln Z~ = -514 on s = 0.28) in fewer than four pairs.  The whole batch runs again
# on 0.7 and 1.8 (where it vanishes altogether) and then on s = 0, over the tables the underflowed attempts left behind.  hp is
# pf_duplex, which has no ladder: its Z~ vanishes with these lengths and the pairs are recomputed in log space.
def bl_whole_batch():
    rs = np.random.RandomState(34)
    van = [vc.fold_case("bl", "vanishing", w, vc.BL_N_VANISHING) for w in vc.POSITIONS]
    return van, [(van[0].seq, SHORT2), (rnd(rs, 70), van[1].seq), (van[2].seq, rnd(rs, 50))]


@pytest.fixture(scope="module")
def bl_whole(hotlib, opool):
    pairs = bl_whole_batch()[1]
    for s1, s2 in pairs:
        opool.pf_duplex(s1, s2)
    return run_bl(pairs, {}, False, then=ordinary_pairs())


def test_vienna_bl_folds_that_vanish_whole_batch_route(bl_whole, bl_fresh_ordinary):
    assert bl_whole["path"] == 3 and bl_whole["fb"][2] == [0, 3, 4] and bl_whole["fb"][0] == []
    assert_same_bits(bl_whole["then"], bl_fresh_ordinary[False], "ordinary Vienna-BL batch after the vanishing one")


@pytest.mark.parametrize("p", range(3), ids=vc.POSITIONS)
def test_vienna_bl_vanishing_fold_equals_the_embedded_reference(bl_whole, refs, opool, p):
    """bp, up at fifteen widths and log Z; the partner against the oracle; hp against pf_duplex on the full pair"""
    van, pairs = bl_whole_batch()
    which = 1 if p == 1 else 0
    check_bl_fold(bl_whole["res"][p], which, van[p], refs)
    check_bl_short(bl_whole["res"][p], 1 - which, pairs[p][1 - which], opool, "partner of pair %d" % p)
    od = opool.pf_duplex(*pairs[p]).result()
    assert logz_close(bl_whole["res"][p]["logZ"][2], od["logZ"]), p
    assert_prob_close(bl_whole["res"][p]["hp"], od["pr"], rel=REL, what="pf_duplex of pair %d" % p)
    assert p != 0 or od["pr"].max() > 0.1


def test_vienna_bl_folds_inside_the_range_stay_on_the_first_pass(hotlib, refs):
    """n = 1500 (ln Z~ = -402), the three insert positions; the partner has no letter that pairs, so no sweep is flagged"""
    cases = [vc.fold_case("bl", "inside", w, vc.BL_N_INSIDE) for w in vc.POSITIONS]
    run = run_bl([(c.seq, "A" * 20) for c in cases], {}, False)
    assert run["path"] == 1 and run["fb"] == [[], [], [], []]
    for p, c in enumerate(cases):
        check_bl_fold(run["res"][p], 0, c, refs)
        assert not run["res"][p]["hp"].any()


# ---- per-pair route (RH_PAIR_HELPER=2, four pairs, hp from the two-molecule ensemble): only the pair that holds the vanishing
# sequence is recomputed.  Its second molecule is the short one itself, so hp is the short pair's, shifted.
def bl_helper_batches():
    rs = np.random.RandomState(35)
    case = vc.fold_case("bl", "vanishing", "3'", vc.BL_N_VANISHING)
    assert (case.seq, SHORT2) == vc.cofold_pair(case.f5, vc.FLANK)
    plain = [(rnd(rs, 300), rnd(rs, 260)), (rnd(rs, 150), rnd(rs, 333)), (rnd(rs, vc.BL_N_VANISHING), rnd(rs, len(SHORT2))), (rnd(rs, 128), rnd(rs, 127))]
    mixed = list(plain)
    mixed[2] = (case.seq, SHORT2)
    return case, plain, mixed


@pytest.fixture(scope="module")
def bl_helper(hotlib):
    return run_bl(bl_helper_batches()[2], {"RH_PAIR_HELPER": "2"}, True, then=ordinary_pairs())


def test_vienna_bl_vanishing_pair_is_recomputed_alone(bl_helper, bl_fresh_ordinary):
    """... and every other pair keeps the bits of a batch without it"""
    base = run_bl(bl_helper_batches()[1], {}, True)
    assert base["path"] == 1
    assert bl_helper["path"] == 3 and sorted(bl_helper["fb"][2] + bl_helper["fb"][0]) == [4, 5]
    assert_same_bits({p: bl_helper["res"][p] for p in (0, 1, 3)}, {p: base["res"][p] for p in (0, 1, 3)}, "pairs next to the recomputed one")
    assert_same_bits(bl_helper["then"], bl_fresh_ordinary[True], "ordinary batch after the per-pair route")


def test_vienna_bl_pair_recomputed_alone_equals_the_embedded_references(bl_helper, refs):
    case, r = bl_helper_batches()[0], bl_helper["res"][2]
    check_bl_fold(r, 0, case, refs)
    assert logz_close(r["logZ"][1], refs["bl2"]["logZ"])
    assert_prob_close(r["bp2"], refs["bl2"]["post"], rel=REL, what="bp2 of the recomputed pair")
    assert_prob_close(r["up2"], refs["bl2"]["up"], rel=REL, abs_floor=1e-11, what="up2 of the recomputed pair")
    assert logz_close(r["logZ"][2], refs["co"]["logZ"])
    assert_prob_close(r["hp"], vc.embed_hp(refs["co"]["hp"], case.n, len(SHORT2), case.f5 - vc.FLANK, 0), rel=REL, what="hp of the recomputed pair")
    assert r["hp"].max() > 0.1


# ---- no exponent fits: one vanishing sequence and one ordinary random 1900-mer (log Z 0.28 per letter: it overflows on s = 0)
def bl_no_fit_batch():
    rs = np.random.RandomState(36)
    case = vc.fold_case("bl", "vanishing", "mid", vc.BL_N_VANISHING)
    return case, [(case.seq, rnd(rs, 60)), (rnd(rs, vc.BL_N_VANISHING), rnd(rs, 80))]


@pytest.fixture(scope="module")
def bl_no_fit(hotlib):
    return run_bl(bl_no_fit_batch()[1], {}, False, then=ordinary_pairs())


@pytest.fixture(scope="module")
def bl_no_fit_log(hotlib):
    return run_bl(bl_no_fit_batch()[1], {}, False, mode=1)


def test_vienna_bl_no_exponent_fits_the_batch_ends_in_log_space(bl_no_fit, refs, bl_fresh_ordinary):
    assert bl_no_fit["path"] == 3 and bl_no_fit["fb"][2] == []
    assert_same_bits(bl_no_fit["then"], bl_fresh_ordinary[False], "ordinary batch after the batch no exponent held")
    check_bl_fold(bl_no_fit["res"][0], 0, bl_no_fit_batch()[0], refs)


def test_vienna_bl_no_exponent_fits_the_log_space_context(bl_no_fit_log, refs):
    """the reference of the random 1900-mer, itself against the embedded reference where there is one"""
    assert bl_no_fit_log["path"] == 2 and bl_no_fit_log["res"][1]["logZ"][0] > vc.LN_HI
    check_bl_fold(bl_no_fit_log["res"][0], 0, bl_no_fit_batch()[0], refs)


@pytest.mark.parametrize("p", range(2))
def test_vienna_bl_no_exponent_fits_equals_the_log_space_context(bl_no_fit, bl_no_fit_log, p):
    check_against_the_log_space_context(bl_no_fit["res"][p], bl_no_fit_log["res"][p], "pair %d" % p)


# ---- 1010 + 1010 letters: each fold is inside (ln Z~ = -265) and the joint ensemble is not (-505); the inserts sit on both sides of
# the cut, so hp is not zero.  The batch runs again down to s = 0.
@pytest.fixture(scope="module")
def bl_joint(hotlib):
    c = vc.cofold_case()
    return run_bl([(c.s1, c.s2)], {}, True, then=ordinary_pairs())


def test_vienna_bl_two_molecule_ensemble_vanishes_while_its_folds_do_not(bl_joint, refs):
    c, r = vc.cofold_case(), bl_joint["res"][0]
    assert bl_joint["path"] == 3 and bl_joint["hpath"] == 3 and bl_joint["fb"][0] == [] and bl_joint["fb"][1] == []
    for z, ref in zip(r["logZ"], (refs["bl"]["logZ"], refs["bl2"]["logZ"], refs["co"]["logZ"])):
        assert logz_close(z, ref), (r["logZ"], ref)
    assert_prob_close(r["hp"], vc.embed_hp(refs["co"]["hp"], len(c.s1), len(c.s2), c.k1 - vc.FLANK, 0), rel=REL, what="hp of the vanishing ensemble")
    assert r["hp"].max() > 0.1


def test_vienna_bl_folds_of_the_vanishing_two_molecule_ensemble(bl_joint, refs, bl_fresh_ordinary):
    c, r = vc.cofold_case(), bl_joint["res"][0]
    n2, l2 = len(c.s2), len(vc.INSERT2)
    assert_prob_close(r["bp1"], vc.embed_bp(refs["bl"]["post"], L, c.k1, vc.FLANK), rel=REL, what="bp1 of the vanishing ensemble")
    assert_prob_close(r["bp2"], vc.embed_bp(refs["bl2"]["post"], l2, vc.FLANK, n2 - l2 - vc.FLANK), rel=REL, what="bp2 of the vanishing ensemble")
    assert_prob_close(r["up1"], vc.embed_up(refs["bl"]["up"], L, c.k1, vc.FLANK), rel=REL, abs_floor=1e-11, what="up1 of the vanishing ensemble")
    assert_prob_close(r["up2"], vc.embed_up(refs["bl2"]["up"], l2, vc.FLANK, n2 - l2 - vc.FLANK), rel=REL, abs_floor=1e-11, what="up2 of the vanishing ensemble")
    assert_same_bits(bl_joint["then"], bl_fresh_ordinary[True], "ordinary two-molecule batch after the vanishing one")


# =================================================================================== Vienna-BL pf_duplex
BL_DX = {c.label: c for c in vc.duplex_cases() if c.model == "bl"}


@pytest.mark.parametrize("label,path", [("inside", 1), ("vanishing", 3)])
def test_vienna_bl_pf_duplex_that_vanishes_goes_to_log_space(hotlib, opool, bl_fresh_ordinary, label, path):
    """pf_duplex has no ladder: 1025 x 1025 (ln Z~ = -503 on s = 0.27) is flagged and recomputed in log space, 700 x 700 (-328)
    stays on dxvl_sweep4<false>; an ordinary batch on the same context afterwards has the bits of a fresh context"""
    s1, s2 = BL_DX[label].s1, BL_DX[label].s2
    o = opool.pf_duplex(s1, s2).result()
    c = vbl(False)
    try:
        hp, z = c.duplex(s1, s2)
        assert c.last_hybrid_path() == path
        assert path != 1 or c.batch_kernels()[2][0] == "dxvl_sweep4<false>"
        assert logz_close(z, o["logZ"]), (z, o["logZ"])
        assert_prob_close(hp, o["pr"], rel=REL, what="pf_duplex " + label)
        assert_same_bits(compute(c, ordinary_pairs()), bl_fresh_ordinary[False], "ordinary batch after the pf_duplex call")
    finally:
        c.close()


@pytest.fixture(scope="module")
def ctx20(hotlib, tmp_path_factory):
    import ractip_amd
    T = v2.random_tables(23)
    path = str(tmp_path_factory.mktemp("par") / "synthetic_v20.par")
    v2.write_par_v20(path, T)
    c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL, param_file=path, vienna=dict(use_bl_param=False))
    c.set_duplex_mode(0)
    yield T, c
    c.close()


@pytest.mark.parametrize("label", ["inside", "vanishing"])
def test_vienna_2x_pf_duplex_on_the_same_pairs(ctx20, label):
    """The same two pairs under the ViennaRNA-2.x energies (synthetic tables) with rh_set_duplex_mode(AUTO), against the loop-for-loop
    restatement of oracle/vienna2x.py; on these tables the longer pair's ln Z~ is -456, five nats INSIDE the flag threshold."""
    T, c = ctx20
    assert c.vienna_semantics() == 2
    s1, s2 = BL_DX[label].s1, BL_DX[label].s2
    efw, ebk, pr = v2.pf_duplex(T, s1, s2)
    hp, z = c.duplex(s1, s2)
    print("2.x pf_duplex %s: ln Z~ %.1f, path %d" % (label, efw - vc.VDX_S * (len(s1) + len(s2) + 2), c.last_hybrid_path()))
    assert c.last_hybrid_path() in (1, 3)
    assert logz_close(z, efw) and abs(efw - ebk) <= 1e-10 * abs(efw), (z, efw, ebk)
    assert_prob_close(hp, pr, rel=REL, what="2.x pf_duplex " + label)
    assert pr.max() > 0.1
