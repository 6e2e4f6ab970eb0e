"""GPU suite: pf_duplex under the ViennaRNA-2.x loop energies (RH_VIENNA_SEM_20, the HAVE_VIENNA20 branch of
/root/reference/src/pf_duplex.c:128-206) on the SCALED LINEAR kernels, switched on by rh_set_duplex_mode -- the path of the
pf_duplex sweeps alone, independent of rh_set_mode.  PARITY UNPINNED like the rest of the Vienna model: the kernels are
compared with oracle/vienna2x.py (pf_duplex restated loop for loop, and enumeration of every duplex) on the synthetic
all-distinct tables of random_tables(23), and with the log-space kernels of the same context.
Tolerances are those of tests/test_gpu_vienna2x.py: log Z rel 1e-9; hp rtol 1e-8, atol 1e-12."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import vienna2x as v2  # noqa: E402

pytestmark = pytest.mark.gpu
REL = 1e-9
HP = dict(rtol=1e-8, atol=1e-12)
INHERIT, AUTO, LOG, LINEAR = -1, 0, 1, 2
SWEEP_2X = "dxvl_sweep4<true>"


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    T = v2.random_tables(23)
    path = str(tmp_path_factory.mktemp("par") / "synthetic_v20.par")
    v2.write_par_v20(path, T)
    return T, path


def new_ctx20(path):
    import ractip_amd
    return ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL, param_file=path, vienna=dict(use_bl_param=False))


@pytest.fixture(scope="module")
def ctx20(hotlib, synth):
    c = new_ctx20(synth[1])
    yield c
    c.close()


def rand_seq(rng, n):
    return "".join("ACGU"[k] for k in rng.integers(0, 4, n))


def same_logz(a, b):
    return (a < -1e18 and b < -1e18) or a == pytest.approx(b, rel=REL)


def batch(c, pairs):
    c.batch_upload(pairs)
    c.batch_compute()
    return [c.batch_results(p) for p in range(len(pairs))]


def assert_bits(res, want):
    for r, w in zip(res, want):
        for k in ("hp", "bp1", "bp2", "up1", "up2", "logZ"):
            assert np.array_equal(r[k], w[k]), k


# ---- 1. the linear path against the loop-for-loop restatement
# part one: the eight pairs of the existing 2.x duplex test (long 1xn, 2x3, long-bulge and asymmetric loops, N letters, 1x7, 33x2);
# part two: random pairs whose first length sits at the edges of the kernel's 62-column groups (62|63, 124|125; 130 = three groups)
def oracle_cases():
    rng = np.random.default_rng(7)
    cases = [(rand_seq(rng, a), rand_seq(rng, b)) for a, b in ((12, 9), (25, 31), (40, 38), (1, 7), (33, 2))]
    cases.append(("GGAAAAAAAAAAAAAAAAAAAAAAAAAGCAAAGG", "CCUUUGUUC"))
    cases.append(("GCAG", "CAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAGUUUGC"))
    cases.append(("GANNCUG", "CAGNUC"))
    rng = np.random.default_rng(11)
    cases += [(rand_seq(rng, a), rand_seq(rng, b)) for a, b in ((61, 9), (62, 9), (63, 9), (64, 9), (66, 20), (70, 36), (130, 12))]
    return cases


@pytest.mark.parametrize("s1,s2", oracle_cases(), ids=lambda s: "%d" % len(s))
def test_linear_pf_duplex_2x_against_the_loop_for_loop_restatement(ctx20, synth, s1, s2):
    T, _ = synth
    ctx20.set_duplex_mode(LINEAR)
    assert ctx20.get_duplex_mode() == LINEAR
    hp, logz = ctx20.duplex(s1, s2)
    assert ctx20.last_hybrid_path() == 1
    efw, ebk, pr = v2.pf_duplex(T, s1, s2)
    print("logZ gpu %.15g oracle fw %.15g bk %.15g  max|hp - pr| %.3g" % (logz, efw, ebk, np.abs(hp - pr).max()))
    if efw == -math.inf:
        assert logz < -1e18 and not hp.any()
        return
    assert logz == pytest.approx(efw, rel=REL) and efw == pytest.approx(ebk, rel=1e-10)
    assert np.allclose(hp, pr, **HP), np.abs(hp - pr).max()


def test_linear_pf_duplex_2x_without_a_complementary_letter(ctx20):
    ctx20.set_duplex_mode(LINEAR)
    hp, logz = ctx20.duplex("AAGAAGGA", "GAGGAAG")
    assert ctx20.last_hybrid_path() == 1
    assert logz < -1e18 and not hp.any()


# ---- 2. against enumeration
def test_linear_pf_duplex_2x_against_enumeration_of_all_duplexes(ctx20, synth):
    T, _ = synth
    rng = np.random.default_rng(9)
    ctx20.set_duplex_mode(LINEAR)
    for _ in range(6):
        s1, s2 = rand_seq(rng, int(rng.integers(3, 8))), rand_seq(rng, int(rng.integers(3, 8)))
        lz, prb = v2.brute_duplex(T, s1, s2)
        hp, logz = ctx20.duplex(s1, s2)
        assert ctx20.last_hybrid_path() == 1
        if lz == -math.inf:
            assert logz < -1e18 and not hp.any()
            continue
        assert logz == pytest.approx(lz, rel=REL), (s1, s2)
        assert np.allclose(hp, prb, **HP), (s1, s2)


# ---- 3. linear equals log-space on one context, ragged batch
def test_linear_equals_log_space_on_a_ragged_batch(ctx20):
    rng = np.random.default_rng(31)
    shapes = [(200, 180), (1, 23), (37, 1), (63, 125), (124, 62), (5, 5), (190, 17), (16, 171), (62, 63), (90, 90), (125, 40), (2, 3)]
    pairs = [(rand_seq(rng, a), rand_seq(rng, b)) for a, b in shapes]
    ctx20.set_duplex_mode(LINEAR)
    lin = batch(ctx20, pairs)
    assert ctx20.last_hybrid_path() == 1 and ctx20.last_path() == 2
    assert ctx20.batch_kernels()[2][0] == SWEEP_2X
    ctx20.set_duplex_mode(LOG)
    log = batch(ctx20, pairs)
    assert ctx20.last_hybrid_path() == 2 and ctx20.last_path() == 2
    assert ctx20.batch_kernels()[2][0] == "dxv_sweep_diag"
    for p, (a, b) in enumerate(zip(lin, log)):
        print("pair %d %s: logZ lin %.15g log %.15g  max|dhp| %.3g" % (p, shapes[p], a["logZ"][2], b["logZ"][2], np.abs(a["hp"] - b["hp"]).max()))
    for p, (a, b) in enumerate(zip(lin, log)):
        assert same_logz(a["logZ"][2], b["logZ"][2]), p
        assert np.allclose(a["hp"], b["hp"], **HP), (p, np.abs(a["hp"] - b["hp"]).max())
        for k in ("bp1", "bp2", "up1", "up2"):     # the McCaskill sweeps do not see the duplex mode
            assert np.array_equal(a[k], b[k]), (p, k)
        assert np.array_equal(a["logZ"][:2], b["logZ"][:2]), p


# ---- 4. AUTO falls back
def test_auto_recomputes_in_log_space_what_leaves_the_double_range(ctx20):
    """The linear sweeps store Z * exp(-0.27 (L1+L2+2)) and flag a pair whose value leaves 1e-200 .. 1e200, i.e. whose
    |log Z - 0.27 (L1+L2+2)| exceeds 460.5.  Under the synthetic tables log Z of G^n / C^n grows by 5.128 per letter pair
    (oracle: 48.42 at n = 12, 89.44 at n = 20), the scale by 0.54: n >= 104 leaves the range; n = 120 (log of the scaled
    value: about 537) does so with a margin and stays below the largest double."""
    rng = np.random.default_rng(41)
    pairs = [(rand_seq(rng, 40), rand_seq(rng, 33)), ("G" * 120, "C" * 120), (rand_seq(rng, 70), rand_seq(rng, 64))]
    ctx20.set_duplex_mode(LOG)
    log = batch(ctx20, pairs)
    assert ctx20.last_hybrid_path() == 2 and ctx20.batch_fallbacks(1) == []
    ctx20.set_duplex_mode(AUTO)
    auto = batch(ctx20, pairs)
    assert ctx20.batch_fallbacks(1) == [1]          # the first pass flagged the G/C pair and nothing else
    assert ctx20.last_hybrid_path() == 3 and ctx20.last_path() == 2
    assert_bits(auto, log)                          # the whole batch went to the log-space kernels
    ctx20.batch_upload(pairs[::2])                  # the ordinary pairs alone stay on the linear kernels
    ctx20.batch_compute()
    assert ctx20.last_hybrid_path() == 1 and ctx20.batch_fallbacks(1) == []
    for p, q in ((0, 0), (1, 2)):
        r = ctx20.batch_results(p)
        assert same_logz(r["logZ"][2], log[q]["logZ"][2]) and np.allclose(r["hp"], log[q]["hp"], **HP)


# ---- 5. nothing changes unasked
def test_nothing_changes_for_a_context_that_does_not_ask(hotlib, synth):
    from ractip_amd.hot import RhError
    rng = np.random.default_rng(51)
    pairs = [(rand_seq(rng, 45), rand_seq(rng, 38)), (rand_seq(rng, 20), rand_seq(rng, 66))]
    c = new_ctx20(synth[1])
    try:
        assert c.get_duplex_mode() == INHERIT
        first = batch(c, pairs)
        assert c.last_hybrid_path() == 2 and c.last_path() == 2
        c.set_duplex_mode(LINEAR)
        lin = batch(c, pairs)
        assert c.last_hybrid_path() == 1
        for a, b in zip(lin, first):
            assert same_logz(a["logZ"][2], b["logZ"][2]) and np.allclose(a["hp"], b["hp"], **HP)
        c.set_duplex_mode(INHERIT)
        again = batch(c, pairs)
        assert c.last_hybrid_path() == 2
        assert_bits(again, first)
        with pytest.raises(RhError, match="log-space"):
            c.set_mode(2)
        with pytest.raises(RhError, match="duplex mode"):
            c.set_duplex_mode(3)
        # the two-molecule sweeps follow set_mode, whatever the duplex mode says
        c.set_hybrid(True)
        co = batch(c, pairs)
        assert c.last_hybrid_path() == 2
        c.set_duplex_mode(LINEAR)
        co_lin = batch(c, pairs)
        assert c.last_hybrid_path() == 2
        assert_bits(co_lin, co)
    finally:
        c.close()


# ---- 6. independence on a 1.8 context
def test_duplex_mode_is_independent_of_the_mode_on_a_1_8_context(hotlib):
    import ractip_amd
    M = ractip_amd.hot.RH_MODEL_VIENNA_BL
    rng = np.random.default_rng(61)
    pairs = [(rand_seq(rng, 64), rand_seq(rng, 50)), (rand_seq(rng, 30), rand_seq(rng, 41)), (rand_seq(rng, 9), rand_seq(rng, 70))]
    c, plain = ractip_amd.Context(device=0, model=M), ractip_amd.Context(device=0, model=M)
    try:
        want = batch(plain, pairs)
        assert plain.last_path() == 1 and plain.last_hybrid_path() == 1
        assert plain.batch_kernels()[2][0] == "dxvl_sweep4<false>"
        c.set_duplex_mode(LOG)
        got = batch(c, pairs)
        assert c.last_path() == 1 and c.last_hybrid_path() == 2
        for a, b in zip(got, want):
            assert same_logz(a["logZ"][2], b["logZ"][2]) and np.allclose(a["hp"], b["hp"], **HP)
            assert np.array_equal(a["bp1"], b["bp1"]) and np.array_equal(a["up2"], b["up2"])
        c.set_duplex_mode(INHERIT)
        assert_bits(batch(c, pairs), want)
        assert c.last_path() == 1 and c.last_hybrid_path() == 1
        c.set_mode(LOG)                      # and the other way round: log-space folds, linear duplex
        c.set_duplex_mode(AUTO)
        got = batch(c, pairs)
        assert c.last_path() == 2 and c.last_hybrid_path() == 1
        for a, b in zip(got, want):
            assert np.array_equal(a["hp"], b["hp"]) and a["logZ"][2] == b["logZ"][2]
    finally:
        c.close()
        plain.close()


# ---- 7. BL* tables under forced semantics = 2 (zero-filled 2.x slots)
def test_bl_tables_under_forced_2x_semantics_linear_equals_log(hotlib):
    import ractip_amd
    M = ractip_amd.hot.RH_MODEL_VIENNA_BL
    c20 = ractip_amd.Context(device=0, model=M, vienna=dict(semantics=2))
    c18 = ractip_amd.Context(device=0, model=M)
    try:
        s1, s2 = "GGGAAAUCCCGAGCGAAAGCUC", "GAGCUUUCGCUCGGGAUUUCCC"
        hlog, zlog = c20.duplex(s1, s2)
        assert c20.last_hybrid_path() == 2
        c20.set_duplex_mode(LINEAR)
        hlin, zlin = c20.duplex(s1, s2)
        assert c20.last_hybrid_path() == 1
        _, z18 = c18.duplex(s1, s2)
        print("logZ 2.x linear %.15g log %.15g, 1.8 %.15g" % (zlin, zlog, z18))
        assert zlin == pytest.approx(zlog, rel=REL) and np.allclose(hlin, hlog, **HP)
        assert abs(zlin - z18) > 1e-6 and abs(zlog - z18) > 1e-6
    finally:
        c20.close()
        c18.close()


# ---- 8. reused tables: the four 2.x tables leave nothing stale
def test_reused_tables_give_the_bits_of_a_fresh_context(ctx20, synth):
    rng = np.random.default_rng(81)
    big = [(rand_seq(rng, 130), rand_seq(rng, 60)), (rand_seq(rng, 97), rand_seq(rng, 58))]
    # the same table layout as `big` (no clear in between), other letters, a short pair in the corner of the tables
    same = [(rand_seq(rng, 130), rand_seq(rng, 60)), (rand_seq(rng, 40), rand_seq(rng, 35))]
    small = [(rand_seq(rng, 40), rand_seq(rng, 35)), (rand_seq(rng, 12), rand_seq(rng, 30))]
    ctx20.set_duplex_mode(LINEAR)
    used = []
    for pairs in (big, same, small):
        used.append(batch(ctx20, pairs))
        assert ctx20.last_hybrid_path() == 1
    for pairs, got in zip((big, same, small), used):
        fresh = new_ctx20(synth[1])
        try:
            fresh.set_duplex_mode(LINEAR)
            assert_bits(got, batch(fresh, pairs))
        finally:
            fresh.close()


# ---- 9. a change of mode takes effect at the next compute, without a new upload
def test_mode_change_without_a_new_upload_gives_the_bits_of_a_fresh_context(ctx20, synth, hotlib):
    """the linear and the log-space kernels share the pair's tables, and the linear ones read zero pad columns: a compute that
    follows a log-space compute on the same upload (another mode, or an AUTO fallback) must not see what that one left"""
    import ractip_amd
    rng = np.random.default_rng(91)
    pairs = [(rand_seq(rng, 130), rand_seq(rng, 60)), (rand_seq(rng, 40), rand_seq(rng, 35)), (rand_seq(rng, 63), rand_seq(rng, 9))]
    results = lambda c: [c.batch_results(p) for p in range(len(pairs))]
    fresh = new_ctx20(synth[1])
    try:
        want = {}
        for mode in (LINEAR, LOG):
            fresh.set_duplex_mode(mode)
            want[mode] = batch(fresh, pairs)
    finally:
        fresh.close()
    ctx20.set_duplex_mode(LOG)
    assert_bits(batch(ctx20, pairs), want[LOG])
    for mode, path in ((LINEAR, 1), (LOG, 2), (AUTO, 1), (LOG, 2), (LINEAR, 1)):
        ctx20.set_duplex_mode(mode)
        ctx20.batch_compute()                      # (no upload in between)
        assert ctx20.last_hybrid_path() == path, mode
        assert_bits(results(ctx20), want[LINEAR if path == 1 else LOG])
    # after an AUTO fallback the tables hold log-space values: the next linear compute on that upload clears them
    over = [pairs[0], ("G" * 120, "C" * 120)]
    ctx20.set_duplex_mode(AUTO)
    ctx20.batch_upload(over)
    ctx20.batch_compute()
    assert ctx20.last_hybrid_path() == 3
    ctx20.set_duplex_mode(LINEAR)
    ctx20.batch_compute()
    assert ctx20.last_hybrid_path() == 1
    assert np.array_equal(ctx20.batch_results(0)["hp"], want[LINEAR][0]["hp"])
    # the same promise on a 1.8 context and under the CONTRAfold model (rh_set_mode inherited)
    for kw in (dict(model=ractip_amd.hot.RH_MODEL_VIENNA_BL), dict()):
        a, b = ractip_amd.Context(device=0, **kw), ractip_amd.Context(device=0, **kw)
        try:
            lin = batch(b, pairs)
            a.set_duplex_mode(LOG)
            batch(a, pairs)
            assert a.last_hybrid_path() == 2
            a.set_duplex_mode(INHERIT)
            a.batch_compute()
            assert a.last_hybrid_path() == 1
            assert_bits(results(a), lin)
        finally:
            a.close()
            b.close()
