"""GPU suite: the exponent ladder of the span folds (span_ladder in ractip_amd/csrc/mccaskill_span.hip) DOWNWARDS and off its end.
The other span tests drive it upwards only, with the chain of GC hairpins that overflows the default exponent.  The inputs and their
cheap references are tests/_span_ladder_cases.py; tests/test_span_ladder_cases_cpu.py pins where every designated cell lies
against 1e-280 and against the smallest double on every exponent, without a GPU.

  1  descent, single calls: a lone pair 2395 letters apart (below 1e-280 on 0.28, exactly 0 on 0.7 and 1.8), one 2679 apart and a
     multiloop over 3064 letters (exactly 0 on every positive exponent) answer from 0.0 with the enumeration's band, up and log Z;
     the same at max_w = 5: the accessibility stage on the 0.0 model.  The context's fold bits stay
  2  descent in a batch: one item climbs to 0.7 while another goes down to 0.0; under any chunking
  3  exhaustion, single call: no exponent holds both the chain (huge on 0.0 and 0.28) and a lone pair behind it (tiny or 0 on
     0.7 and 1.8): RH_ERR_UNSUPPORTED, no local result, everything else the context holds is what it was
  4  exhaustion in a batch: the call returns RH_OK, the item has its status, the fetches of that item are refused by name, the
     other items have the bits of their single calls; Context.span_fold_batch raises and names the item
  5  the constrained twin: 'x' on the far letter leaves no pairable cell and the empty ensemble
  6  CONTRAfold: the descent on a custom weight file (one possible pair, closed form), both exhaustion inputs
  7  a structured sequence of 2800 letters at L = n, whose far rows have hairpin weight 0, answers as before

Bars: band rel 1e-6 above 1e-12; Vienna-BL up the same with the floor 1e-11; log Z 1e-9 * max(1, |log Z|); "the bits": ==.

Why the "hole" cases pass without a test for 0 in the inside sweep: the outside sweep stores FCo^ = (outside weight
/ Z) * exp(+s d), and FC~ * FCo^ = P.  A closed cell whose true value lies below the smallest double therefore has an outside cell
above P * 2e323, which the outside sweep flags (> 1e300) for every pair with P > 5e-24; for the cells designated here the
exterior term alone, exp(gi + go - log Z + s d) with s d > 745, is infinite.

GPU time: a descent costs four attempts over 2 * Le launches whose cells sum over up to Le terms; Le = n is set by the zone
conditions (d >= 2395, 2679, 3063), so the descents take 6 to 12 s each on the MI355X, a batch with a descent 19 s.  The single calls
are computed once per module (single()) and shared."""
import ctypes

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot
import _cf_span_ref as cfref
import _contrafold_weights as cw
import _span_acc_cases as ac
import _span_cases as sc
import _span_ladder_cases as lc
from _oracle import Oracle, assert_prob_close
from _span_ladder_cases import RH_ERR_ARG, RH_ERR_UNSUPPORTED, RH_OK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def v1(hotlib):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bl_chain(v1):
    """(the 1300-letter chain, its log Z from Context.fold, which takes its own ladder): huge on 0.28 and so on 0.0"""
    seq = lc.hairpin_chain(lc.BL_CHAIN)
    z = v1.fold(seq)[2]
    assert z - 0.28 * len(seq) > lc.LN_HUGE + 50.0
    assert lc.zone(z - 0.7 * len(seq)) == "in range"
    return seq, z


def make_cf(param_file=None):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_CONTRAFOLD, param_file=param_file)
    c.set_span_contrafold(True)
    return c


@pytest.fixture(scope="module")
def cf(hotlib):
    c = make_cf()
    yield c
    c.close()


@pytest.fixture(scope="module")
def cf_custom(hotlib, tmp_path_factory):
    """(context on the custom weight file, the file, S of lone(d) from the oracle on that file)"""
    path = cw.write(tmp_path_factory.mktemp("ladder") / "custom.params", lc.cf_custom_rows())
    c = make_cf(path)
    yield c, path, lc.cf_pair_weight(Oracle(path))
    c.close()


def err(c):
    return c.L.rh_last_error(c.h).decode()


def equal(a, b):
    return a[0].shape == b[0].shape and a[1].shape == b[1].shape and (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]


def check(got, ref, what, up_floor=1e-11):
    band, up, logz = got
    assert band.shape == ref["band"].shape and up.shape == ref["up"].shape, what
    print("%s: log Z %.12g (reference %.12g)" % (what, logz, ref["logZ"]))
    assert abs(logz - ref["logZ"]) <= 1e-9 * max(1.0, abs(ref["logZ"])), "%s: log Z %r, reference %r" % (what, logz, ref["logZ"])
    assert_prob_close(band, ref["band"], what=what + " band")
    assert_prob_close(up, ref["up"], abs_floor=up_floor, what=what + " up")
    n, ld = band.shape
    i, d = np.arange(n)[:, None], np.arange(ld)[None, :]
    assert not band[(d == 0) | (i + d >= n)].any(), what + ": column 0 and the entries past the end hold 0"


_singles = {}


def single(c, seq, L, max_w=1):
    """span_fold(seq, L, max_w) on the module's Vienna-BL context, called once (a repeated call gives the same bits:
    tests/test_gpu_span_fold.py) and left unchanged"""
    key = (seq, L, max_w)
    if key not in _singles:
        got = c.span_fold(seq, L, max_w)
        got[0].setflags(write=False)
        got[1].setflags(write=False)
        _singles[key] = got
    return _singles[key]


def run_batch(c, seqs, L, max_w=1):
    """rh_span_fold_batch itself: the return code (Context.span_fold_batch raises where an item has no result)"""
    enc = [s.encode() for s in seqs]
    arr, lens = (ctypes.c_char_p * len(enc))(*enc), (ctypes.c_int * len(enc))(*[len(s) for s in seqs])
    return c.L.rh_span_fold_batch(c.h, arr, lens, len(enc), L, max_w)


def statuses(c, count):
    out = []
    for k in range(count):
        st = ctypes.c_int(99)
        assert c.L.rh_span_batch_item(c.h, k, None, None, ctypes.byref(st)) == RH_OK
        out.append(st.value)
    return out


def item_bytes(n, L, max_w, tables=13):
    """the plan formula: the band tables of Le * ldn doubles plus, at widths above one, the gap sums of 2 * 32 rows"""
    Le, ldn = min(n, L), -(-(n + 1) // 16) * 16
    return tables * Le * ldn * 8 + (2 * 32 * ldn * 8 if max_w > 1 else 0)


# ---- 1
@pytest.mark.parametrize("case", lc.DESCENT, ids=lambda c: c.name)
def test_descent_to_the_zero_exponent(v1, case):
    a = sc.random_seq(130)
    bp0, up0, z0 = v1.fold(a)
    ref = sc.masked(case.seq, case.L, bruteforce=True)
    assert ref["band"][0, case.d] > 1e-7, "the designated pair stands far above the floor of 1e-12"
    got = single(v1, case.seq, case.L)
    print("%s: P(designated) %.9g (reference %.9g)" % (case.name, got[0][0, case.d], ref["band"][0, case.d]))
    check(got, ref, case.name)
    bp1, up1, z1 = v1.fold(a)
    assert (bp0 == bp1).all() and (np.asarray(up0) == np.asarray(up1)).all() and z0 == z1


@pytest.mark.parametrize("case", lc.DESCENT, ids=lambda c: c.name)
def test_descent_with_the_accessibility_stage(v1, case):
    ref = ac.masked_acc(case.seq, case.L, lc.ACC_W, bruteforce=True)
    got = v1.span_fold(case.seq, case.L, lc.ACC_W)
    print("%s: P(designated) %.9g (reference %.9g)" % (case.name, got[0][0, case.d], ref["band"][0, case.d]))
    assert (ref["up"][:, 1:] < 0.5).any() and (ref["up"][:, 1:] > 0.5).any()
    check(got, ref, case.name + " max_w %d" % lc.ACC_W)


def test_the_multiloop_sequence_one_letter_below_its_length(v1):
    """L = n - 1 excludes the closing pair and log Z falls from 92.96 to 1.41.  The last C still pairs with the G's of the hairpins,
    3044 letters and more apart: hairpin-only cells that are exactly 0 on 0.28, with probabilities near 1e-7, so this call goes
    down the ladder as well"""
    c = lc.MULTI_HOLE
    ref = sc.masked(c.seq, c.L - 1, bruteforce=True)
    assert 1.0 < ref["logZ"] < 2.0 and ref["band"][10:20, lc.TAIL_MULTI_HOLE:].max() > 1e-9
    check(v1.span_fold(c.seq, c.L - 1), ref, "MULTI_HOLE at L = n - 1")


# ---- 2
def test_descent_in_a_batch_while_another_item_climbs(v1, bl_chain):
    hole, L = lc.LONE_HOLE, lc.LONE_HOLE.L
    seqs = [sc.random_seq(64, seed=1), hole.seq, bl_chain[0], sc.random_seq(257, seed=2)]
    singles = [single(v1, s, L) for s in seqs]
    assert abs(singles[2][2] - bl_chain[1]) <= 1e-9 * bl_chain[1], "the chain answers, from a larger exponent"
    try:
        for budget in (0, 1):                                    # one chunk; one item per chunk
            v1.set_span_batch_bytes(budget)
            assert run_batch(v1, seqs, L) == RH_OK
            assert statuses(v1, 4) == [RH_OK] * 4
            got = [v1.span_batch_results(k) for k in range(4)]
            for k in range(4):
                assert equal(got[k], singles[k]), "item %d, chunk budget %d" % (k, budget)
            check(got[1], sc.masked(hole.seq, L, bruteforce=True), "LONE_HOLE as item 1, chunk budget %d" % budget)
    finally:
        v1.set_span_batch_bytes(0)
    check(singles[0], sc.masked(seqs[0], L), "the ordinary item")


# ---- 3
@pytest.mark.parametrize("case", [lc.EXHAUST_FLAG, lc.EXHAUST_HOLE], ids=lambda c: c.name)
def test_no_exponent_holds_single_call(v1, bl_chain, case):
    assert case.seq.startswith(bl_chain[0]) and case.L == len(bl_chain[0])
    q, t = sc.random_seq(12, seed=1), sc.random_seq(60, seed=2)
    hp2 = v1.local_duplex2(q, t, 12, 1, 30, 10)
    v1.batch_upload([(q, t)])
    v1.batch_compute()
    uploaded = v1.batch_results(0)
    small = [sc.random_seq(n, seed=n) for n in (65, 13, 90)]
    sb = v1.span_fold_batch(small, 20, 3)
    v1.span_fold(small[0], 20)
    assert v1.L.rh_local_layout(v1.h, None, None, None, None, None) == RH_OK
    assert v1.L.rh_span_fold(v1.h, case.seq.encode(), len(case.seq), case.L) == RH_ERR_UNSUPPORTED
    assert "max_span %d" % case.L in err(v1) and "exponent" in err(v1)
    assert v1.L.rh_local_layout(v1.h, None, None, None, None, None) == RH_ERR_ARG, "the call leaves no local result"
    after = v1.batch_results(0)
    assert all((np.asarray(uploaded[key]) == np.asarray(after[key])).all() for key in ("bp1", "bp2", "hp", "up1", "up2", "logZ"))
    assert all(equal(a, v1.span_batch_results(k)) for k, a in enumerate(sb))
    assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(hp2[:2], v1.local_hp2_results()[:2]))
    seq = sc.random_seq(90)
    check(v1.span_fold(seq, 33), sc.masked(seq, 33), "the next span fold")


# ---- 4
def test_no_exponent_holds_for_one_item_of_a_batch(v1, bl_chain):
    bad, L, W = lc.EXHAUST_FLAG, lc.EXHAUST_FLAG.L, lc.ACC_W
    others = [sc.random_seq(40, seed=1), sc.random_seq(300, seed=2), bl_chain[0], sc.random_seq(129, seed=3)]
    alone = {s: v1.span_fold(s, L, W) for s in others}
    seqs = [others[0], bad.seq] + others[1:]
    sizes = [item_bytes(len(s), L, W) for s in seqs]
    assert sizes[1] == max(sizes) and sizes[0] + sizes[1] > sizes[1] >= sum(sizes[2:])      # budget sizes[1]: chunks 1 | 1 | 3

    def served(order, at, what):
        assert statuses(v1, 5) == [RH_ERR_UNSUPPORTED if k == at else RH_OK for k in range(5)], what
        n, ld, st = (ctypes.c_int() for _ in range(3))
        assert v1.L.rh_span_batch_item(v1.h, at, ctypes.byref(n), ctypes.byref(ld), ctypes.byref(st)) == RH_OK
        assert (n.value, ld.value, st.value) == (len(bad.seq), L, RH_ERR_UNSUPPORTED), what
        assert v1.L.rh_span_batch_results(v1.h, at, None, None, None) == RH_ERR_UNSUPPORTED
        assert "rh_span_batch_results: item %d:" % at in err(v1) and "max_span %d" % L in err(v1), what
        assert v1.L.rh_span_batch_candidates(v1.h, at, 0, ctypes.c_float(0.5), None, 0) == RH_ERR_UNSUPPORTED
        assert "rh_span_batch_candidates: item %d:" % at in err(v1), what
        for k, s in enumerate(order):
            if k != at:
                assert equal(v1.span_batch_results(k), alone[s]), "%s: item %d" % (what, k)
                assert v1.span_batch_candidates(k, 1, 0.5)[1] > 0

    with pytest.raises(ractip_amd.RhError, match="item 1: no scale exponent"):
        v1.span_fold_batch(seqs, L, W)
    served(seqs, 1, "one chunk")                                 # (the batch the wrapper refused to fetch from is the context's)
    try:
        v1.set_span_batch_bytes(sizes[1])
        assert run_batch(v1, seqs, L, W) == RH_OK
        served(seqs, 1, "the failed item alone in its chunk")
    finally:
        v1.set_span_batch_bytes(0)
    last = others + [bad.seq]
    assert run_batch(v1, last, L, W) == RH_OK
    served(last, 4, "the failed item last")
    assert abs(alone[bl_chain[0]][2] - bl_chain[1]) <= 1e-9 * bl_chain[1]


# ---- 5
def test_the_constrained_twin_is_the_empty_ensemble(v1):
    c = lc.LONE_FLAG
    single(v1, c.seq, c.L)                                       # the context has been down to 0.0 and back
    got = v1.span_fold(c.seq, c.L, 1, lc.TWIN_CONSTRAINT)
    assert not got[0].any() and (got[1] == 1.0).all() and got[2] == 0.0
    fresh = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    try:
        assert equal(fresh.span_fold(c.seq, c.L, 1, lc.TWIN_CONSTRAINT), got)
    finally:
        fresh.close()


# ---- 6
def test_contrafold_descent_on_the_custom_weight_file(cf_custom):
    c, path, S = cf_custom
    case = lc.CF_HOLE
    want = lc.cf_closed_form(S, case.d)
    assert lc.zones(S, case.d, lc.CF_LADDER) == ("hole", "hole", "hole", "in range") and 0.9 < want["band"][0, case.d] < 0.99
    single = c.span_fold(case.seq, case.L)
    print("CF_HOLE: P(designated) %.9g (reference %.9g)" % (single[0][0, case.d], want["band"][0, case.d]))
    check(single, want, "CF_HOLE", up_floor=1e-12)
    seqs = [sc.random_seq(64, seed=1), case.seq, sc.random_seq(257, seed=2)]
    singles = [c.span_fold(seqs[0], case.L), single, c.span_fold(seqs[2], case.L)]
    got = c.span_fold_batch(seqs, case.L)
    assert statuses(c, 3) == [RH_OK] * 3
    for k in range(3):
        assert equal(got[k], singles[k]), "item %d" % k
    check(got[0], cfref.span_ref(seqs[0], case.L, path), "an ordinary item under the custom file", up_floor=1e-12)


@pytest.mark.parametrize("case", [lc.CF_EXHAUST_FLAG, lc.CF_EXHAUST_HOLE], ids=lambda c: c.name)
def test_contrafold_no_exponent_holds(cf, case):
    chain = lc.hairpin_chain(lc.CF_CHAIN)
    z = cf.fold(chain)[2]
    assert case.seq.startswith(chain) and case.L >= len(chain)
    assert z - 0.12 * len(chain) > lc.LN_HUGE + 50.0 and lc.zone(z - 0.45 * len(chain)) == "in range"
    assert cf.L.rh_span_fold(cf.h, case.seq.encode(), len(case.seq), case.L) == RH_ERR_UNSUPPORTED
    assert "max_span %d" % case.L in err(cf)
    assert cf.L.rh_local_layout(cf.h, None, None, None, None, None) == RH_ERR_ARG
    seqs = [sc.random_seq(64, seed=1), case.seq, sc.random_seq(129, seed=3)]
    assert run_batch(cf, seqs, case.L) == RH_OK
    assert statuses(cf, 3) == [RH_OK, RH_ERR_UNSUPPORTED, RH_OK]
    assert cf.L.rh_span_batch_results(cf.h, 1, None, None, None) == RH_ERR_UNSUPPORTED and "item 1:" in err(cf)
    for k in (0, 2):
        assert equal(cf.span_batch_results(k), cf.span_fold(seqs[k], case.L)), "item %d" % k


# ---- 7
def test_a_structured_long_sequence_still_answers(v1):
    """random_seq(2800) at L = n: the rows past d = 2661 have hairpin weight exp(-0.28 d) = 0 and their pairable cells are not 0 (the
    loops inside them carry weight), so nothing is flagged; a sweep that flagged on the hairpin weight alone would send the call down
    the ladder, to 0.0 in the end, where a sequence with log Z above 645 overflows, and refuse it"""
    seq = sc.random_seq(2800)
    n = len(seq)
    bp, fup, z = v1.fold(seq)
    print("random_seq(2800): log Z %.6f" % z)
    assert lc.zone(z - 0.28 * n) == "in range"
    assert v1.L.rh_span_fold(v1.h, seq.encode(), n, n) == RH_OK
    band, up, logz, _ = v1.local_results()
    assert abs(logz[0] - z) <= 1e-9 * max(1.0, abs(z))
    assert_prob_close(up[:, 0], np.asarray(fup).reshape(n, -1)[:, 0], abs_floor=1e-11, what="up against Context.fold")
    assert band[:100, 2662:].max() > 0.0, "pairs in the rows whose hairpin weight is 0"
