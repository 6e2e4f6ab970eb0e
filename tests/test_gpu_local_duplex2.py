"""GPU suite: local hybridization of two windowed molecules (rh_local_duplex2) -- both models, the three hybridization sources, both
arithmetic paths (the `ctx` fixture; the Vienna-BL contexts follow its path).

The definition, restated here: s1 is cut into windows (W1, S1) with starts a_k, s2 into (W2, S2) with starts b_l, by the rule of local
folding (starts 0, S, .. and a last window that ends the sequence); h_kl is the hybridization matrix of (window k of s1, window l of
s2); hp_loc2(i, j) is the sum over the windows k that contain i, in increasing k, of the ROW SUMS over the windows l that contain j,
in increasing l, of h_kl at the translated coordinates, divided once by the product of the two window counts.  Kinds of check:
  * against the CPU oracles, each window pair from the oracle and averaged in numpy (rel 1e-6, log Z 1e-9);
  * bit for bit against the numpy restatement over what the SAME context returns for all windows of s1 followed by all windows of
    s2, uploaded as one indexed batch with all nw1 x nw2 pairs, under six tilings;
  * one window of either molecule = local_duplex, one window pair = Context.duplex; zeros, candidates, reuse, rejection and the
    independence of the 1-D local results; the pipeline with a planted site in two windowed molecules.
Shapes (n1, W1, S1; n2, W2, S2), the smallest that reach every edge:
  A (23, 16, 5; 41, 16, 5)   3 x 6   off-grid last window of s1; joint length 32 < kStripMinN
  B (41, 16, 1; 23, 16, 5)  26 x 3   S = 1: many windows per letter
  C (50, 33, 33; 43, 33, 5)  2 x 3   S = W with an off-grid last window; joint 66
  D (70, 65, 1; 70, 65, 5)   6 x 2   windows wider than one 58 / 64-column duplex group; joint 130
  E (9, 16, 1; 41, 16, 1)    1 x 26  n1 < W1, one window of s1
  F (16, 16, 1; 16, 16, 1)   1 x 1   one window pair
  G (41, 16, 1; 9, 16, 1)   26 x 1   the mirror of E: n2 < W2, one window of s2
E, G and F take the routes of the scheduler on which a level of the sum has one term and is skipped."""
import os

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot, pipeline
from _oracle import Oracle, ViennaOracle, assert_prob_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-6
MODE = {"auto": hot.RH_MODE_AUTO, "log": hot.RH_MODE_LOG}
VIENNA_W = 5
SHAPES = {"A": (23, 16, 5, 41, 16, 5), "B": (41, 16, 1, 23, 16, 5), "C": (50, 33, 33, 43, 33, 5), "D": (70, 65, 1, 70, 65, 5),
          "E": (9, 16, 1, 41, 16, 1), "F": (16, 16, 1, 16, 16, 1), "G": (41, 16, 1, 9, 16, 1)}
WINDOWS = {"A": (3, 6), "B": (26, 3), "C": (2, 3), "D": (6, 2), "E": (1, 26), "F": (1, 1), "G": (26, 1)}
SOURCES = ["contrafold", "pf_duplex", "cofold"]


def seq_of(n, salt=0):
    return "".join(np.random.RandomState(20261020 + n + 1000 * salt).choice(list("ACGU"), n))


def molecules(case):
    n1, _, _, n2, _, _ = SHAPES[case]
    return seq_of(n1, 1), seq_of(n2)


# ---- the definition, restated
def windows(n, W, S):
    if n <= W:
        return [0]
    m = -(-(n - W) // S)
    return [k * S for k in range(m)] + [n - W]


def window_grid(s1, s2, shape):
    """(windows of s1, windows of s2, starts1, starts2)"""
    _, W1, S1, _, W2, S2 = shape
    a, b = windows(len(s1), W1, S1), windows(len(s2), W2, S2)
    We1, We2 = min(W1, len(s1)), min(W2, len(s2))
    return [s1[s:s + We1] for s in a], [s2[s:s + We2] for s in b], a, b


def average2(shape, h):
    """hp_loc2 (n1+1, n2+1) from h[k][l], each (We1+1, We2+1), 1-based: per window of s1 the row sum over the windows of s2 in
    increasing l, the row sums added in increasing k, one division by the product of the counts"""
    n1, W1, S1, n2, W2, S2 = shape
    a, b, We1, We2 = windows(n1, W1, S1), windows(n2, W2, S2), min(W1, n1), min(W2, n2)
    acc, c1, c2 = np.zeros((n1 + 1, n2 + 1)), np.zeros(n1 + 1), np.zeros(n2 + 1)
    for k, sa in enumerate(a):
        row = np.zeros((We1, n2 + 1))
        for l, sb in enumerate(b):
            hkl = np.asarray(h[k][l])
            assert hkl.shape == (We1 + 1, We2 + 1)
            row[:, sb + 1:sb + We2 + 1] += hkl[1:, 1:]
        acc[sa + 1:sa + We1 + 1] += row
        c1[sa + 1:sa + We1 + 1] += 1
    for sb in b:
        c2[sb + 1:sb + We2 + 1] += 1
    assert c1[1:].min() >= 1 and c2[1:].min() >= 1              # every letter lies in a window: no holes
    acc[1:, 1:] /= c1[1:, None] * c2[None, 1:]
    return acc


# ---- contexts
@pytest.fixture(scope="module")
def vctx(ctx):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    c.set_mode(MODE[ctx.path_name])
    c.set_max_w(VIENNA_W)
    yield c
    c.close()


def fresh_like(c, model, cofold=False):
    """a new context of `model` on the arithmetic path of the `ctx` fixture c"""
    f = ractip_amd.Context(device=0, model=model)
    f.set_mode(MODE[c.path_name])
    if model == hot.RH_MODEL_VIENNA_BL:
        f.set_max_w(VIENNA_W)
        f.set_hybrid(cofold)
    return f


def context_of(source, ctx, vctx):
    if source == "contrafold":
        return ctx
    vctx.set_hybrid(source == "cofold")
    return vctx


# ---- oracle references, once per window pair
_oracles, _memo = {}, {}


def oracle_pair(source, a, b):
    """(hp, log Z) of one pair from the CPU oracle of the source"""
    key = (source, a, b)
    if key not in _memo:
        if source == "contrafold":
            o = _oracles.setdefault("cf", Oracle()).duplex(a, b)
            _memo[key] = (o["post"], o["logZ2"][0])
        elif source == "pf_duplex":
            o = _oracles.setdefault("vo", ViennaOracle()).pf_duplex(a, b)
            _memo[key] = (o["pr"], o["logZ"])
        else:
            o = _oracles.setdefault("vo", ViennaOracle()).cofold(a, b)
            _memo[key] = (o["hp"], o["logZ"])
    return _memo[key]


def oracle_average2(source, s1, s2, shape):
    w1, w2, a, b = window_grid(s1, s2, shape)
    ref = [[oracle_pair(source, x, y) for y in w2] for x in w1]
    want = average2(shape, [[r[0] for r in row] for row in ref])
    return want, np.array([[r[1] for r in row] for row in ref]), a, b


def check_parity(c, source, case, what):
    shape = SHAPES[case]
    s1, s2 = molecules(case)
    want, want_z, a, b = oracle_average2(source, s1, s2, shape)
    hp, logz, starts1, starts2 = c.local_duplex2(s1, s2, shape[1], shape[2], shape[4], shape[5])
    assert list(starts1) == a and list(starts2) == b and (len(a), len(b)) == WINDOWS[case]
    assert hp.shape == (len(s1) + 1, len(s2) + 1) and logz.shape == (len(a), len(b))
    print("%s: max |log Z - oracle| = %.3e, max |hp - oracle| = %.3e" % (what, np.abs(logz - want_z).max(), np.abs(hp - want).max()))
    assert np.abs(logz - want_z).max() < 1e-9, what
    assert_prob_close(hp, want, rel=REL, what="hp " + what)


# ---- 1. against the CPU oracles
@pytest.mark.parametrize("case", ["A", "C", "D", "E"])
@pytest.mark.parametrize("source", SOURCES)
def test_against_the_oracle(ctx, vctx, source, case):
    c = context_of(source, ctx, vctx)
    check_parity(c, source, case, "%s %s %s" % (source, ctx.path_name, case))


def test_vienna_duplex_under_its_own_duplex_mode(ctx, vctx):
    """rh_set_duplex_mode(RH_MODE_AUTO): the pf_duplex sweeps on the scaled linear kernels whatever the folds run on"""
    c = context_of("pf_duplex", ctx, vctx)
    c.set_duplex_mode(hot.RH_MODE_AUTO)
    try:
        check_parity(c, "pf_duplex", "A", "pf_duplex, duplex mode auto, folds %s" % ctx.path_name)
        assert c.last_hybrid_path() == 1
    finally:
        c.set_duplex_mode(hot.RH_MODE_INHERIT)


# ---- 2. the bits do not depend on the tiling
def per_window_pair(c, s1, s2, shape):
    """what the context itself returns for all windows of s1 followed by all windows of s2, one indexed batch with all pairs.  A grid of
    one window pair is defined to have the bits of Context.duplex, whose two-molecule sweeps are not seeded from folds (DESIGN.md 5.1j,
    "One window"; a batch with folds differs from it in the last bits under cofold on the scaled linear path): there h_00 is that."""
    w1, w2, _, _ = window_grid(s1, s2, shape)
    if len(w1) == len(w2) == 1:
        hp, z = c.duplex(w1[0], w2[0])
        return [[np.array(hp)]], np.array([[z]])
    c.batch_upload_indexed(w1 + w2, [(k, len(w1) + l) for k in range(len(w1)) for l in range(len(w2))])
    c.batch_compute()
    r = c.batch_results_all()
    h = [[np.array(r["hp"][k * len(w2) + l]) for l in range(len(w2))] for k in range(len(w1))]
    return h, r["logZ"][:, 2].reshape(len(w1), len(w2)).copy()


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "G", "F"])
@pytest.mark.parametrize("source", SOURCES)
def test_hp_is_the_ordered_sum_of_row_sums_under_every_tiling(ctx, vctx, source, case):
    c = context_of(source, ctx, vctx)
    shape = SHAPES[case]
    nw1, nw2 = WINDOWS[case]
    s1, s2 = molecules(case)
    h, logz = per_window_pair(c, s1, s2, shape)
    want = average2(shape, h)
    try:
        for rows, cols in ((1, 1), (2, 3), (3, 2), (nw1, 1), (1, nw2), (0, 0)):
            what = "%s %s %s tile %d x %d" % (source, ctx.path_name, case, rows, cols)
            c.set_local_tile(rows, cols)
            hp, lz, _, _ = c.local_duplex2(s1, s2, shape[1], shape[2], shape[4], shape[5])
            assert c.local_hp2_tile() == ((min(rows, nw1), min(cols, nw2)) if rows else (nw1, nw2)), what   # (these grids fit one automatic tile)
            assert np.array_equal(hp, want), what + ": hp"
            assert np.array_equal(lz, logz), what + ": log Z"
    finally:
        c.set_local_tile(0, 0)


# ---- 3. one window of a molecule, one window pair
@pytest.mark.parametrize("source", SOURCES)
def test_one_window_of_a_molecule_has_the_bits_of_local_duplex(ctx, vctx, source):
    c = context_of(source, ctx, vctx)
    n1, W1, S1, n2, W2, S2 = SHAPES["E"]
    s1, s2 = molecules("E")
    want, want_z, want_starts = c.local_duplex(s1, s2, W2, S2, windowed=2)
    hp, logz, starts1, starts2 = c.local_duplex2(s1, s2, W1, S1, W2, S2)
    assert list(starts1) == [0] and list(starts2) == list(want_starts) and logz.shape == (1, len(want_starts))
    assert np.array_equal(hp, want) and np.array_equal(logz[0], want_z)
    # mirrored: s2 has one window
    want, want_z, want_starts = c.local_duplex(s2, s1, W2, S2, windowed=1)
    hp, logz, starts1, starts2 = c.local_duplex2(s2, s1, W2, S2, W1, S1)
    assert list(starts2) == [0] and list(starts1) == list(want_starts) and logz.shape == (len(want_starts), 1)
    assert np.array_equal(hp, want) and np.array_equal(logz[:, 0], want_z)


@pytest.mark.parametrize("source", SOURCES)
def test_one_window_pair_has_the_bits_of_rh_duplex(ctx, vctx, source):
    """nw1 x nw2 = 1: the one compute runs unseeded, like rh_duplex / rh_cofold_constrained, which stage the pair without its folds"""
    c = context_of(source, ctx, vctx)
    n1, W1, S1, n2, W2, S2 = SHAPES["F"]
    s1, s2 = molecules("F")
    want, z = c.duplex(s1, s2)                                 # (under the context's hybrid source)
    if source == "cofold":
        also, also_z = c.cofold(s1, s2)
        assert np.array_equal(also, want) and also_z == z
    hp, logz, starts1, starts2 = c.local_duplex2(s1, s2, W1, S1, W2, S2)
    assert list(starts1) == [0] and list(starts2) == [0] and logz.shape == (1, 1)
    print("one pair %s %s: max |local - duplex| = %.3e, log Z %.3e" % (source, ctx.path_name, np.abs(hp - want).max(), abs(logz[0, 0] - z)))
    assert np.array_equal(hp, want) and logz[0, 0] == z


# ---- 4. zeros and holes
COMPLEMENT = {"A": "U", "U": "A", "C": "G", "G": "C"}


def planted(case):
    """the molecules of a case with a stretch of s2 made the reverse complement of a stretch of s1"""
    s1, s2 = molecules(case)
    site = "".join(COMPLEMENT[ch] for ch in reversed(s1[8:18]))
    return s1, s2[:20] + site + s2[30:]


@pytest.mark.parametrize("source", SOURCES)
def test_zeros_and_no_holes(ctx, vctx, source):
    c = context_of(source, ctx, vctx)
    shape = SHAPES["A"]
    s1, s2 = planted("A")
    assert (len(s1), len(s2)) == (shape[0], shape[3]) and set(s1) == set(s2) == set("ACGU")
    hp, logz, _, _ = c.local_duplex2(s1, s2, shape[1], shape[2], shape[4], shape[5])
    assert not hp[0].any() and not hp[:, 0].any()
    assert np.isfinite(hp).all() and hp.min() >= 0.0 and np.isfinite(logz).all()
    assert (hp[1:, 1:].max(axis=1) > 0.0).all() and (hp[1:, 1:].max(axis=0) > 0.0).all()   # every row and column carries a positive entry
    print("planted %s %s: largest row sum %.4f, over the planted columns %.4f" % (
        source, ctx.path_name, hp.sum(axis=1).max(), hp[9:19, 21:31].sum(axis=1).min()))


# ---- 5. candidates
def scan_hp(hp, th):
    """row-major numpy scan over 1..n1 x 1..n2: float narrowing, then p > th"""
    v32 = hp.astype(np.float32)
    return [(i, j, v32[i, j]) for i in range(1, hp.shape[0]) for j in range(1, hp.shape[1]) if v32[i, j] > np.float32(th)]


def test_candidates_equal_a_numpy_scan_of_the_fetched_matrix(ctx, vctx):
    shape = SHAPES["A"]
    s1, s2 = planted("A")
    for source, th in (("contrafold", 0.01), ("pf_duplex", 0.003), ("cofold", 1e-4)):
        c = context_of(source, ctx, vctx)
        hp = c.local_duplex2(s1, s2, shape[1], shape[2], shape[4], shape[5])[0]
        want = scan_hp(hp, th)
        assert len(want) > 8, source
        rec, total = c.local_hp2_candidates(th)
        assert total == len(want)
        assert [(int(r["i"]), int(r["j"]), r["p"]) for r in rec] == want
        rec, total = c.local_hp2_candidates(th, cap=5)         # too small: the first records, the whole count
        assert total == len(want) and [(int(r["i"]), int(r["j"]), r["p"]) for r in rec] == want[:5]
        p0 = float(want[0][2])                                 # an entry exactly at the threshold is not reported
        rec, total = c.local_hp2_candidates(p0)
        assert total == sum(1 for r in want if r[2] > np.float32(p0)) and total < len(want)


# ---- 6. reuse, rejection, independence of the other local results
def same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("source", SOURCES)
def test_reuse_rejection_and_independence(ctx, source):
    model = hot.RH_MODEL_CONTRAFOLD if source == "contrafold" else hot.RH_MODEL_VIENNA_BL
    calls = []
    for case in ("D", "A"):                                     # a big, then a small one
        sh = SHAPES[case]
        calls.append(molecules(case) + (sh[1], sh[2], sh[4], sh[5]))
    want = []
    for args in calls:
        f = fresh_like(ctx, model, source == "cofold")
        want.append(f.local_duplex2(*args))
        f.close()
    big, small = calls
    c = fresh_like(ctx, model, source == "cofold")
    try:
        with pytest.raises(ractip_amd.RhError, match="no local hybridization result of two windowed molecules"):
            c.local_hp2_results()
        with pytest.raises(ractip_amd.RhError, match="no local hybridization result of two windowed molecules"):
            c.local_hp2_candidates(0.1)
        # the 1-D local calls before any 2-D one: what they give on their own
        fold0 = c.local_fold(small[1], 16, 5)
        dup0 = c.local_duplex(small[0], small[1], 16, 5, 2) + c.local_results()
        assert same(c.local_duplex2(*big), want[0])
        assert same(c.local_hp_results() + (dup0[2],) + c.local_results(), dup0)      # the 2-D call left the 1-D results alone
        c.set_local_tile(2, 4)
        assert same(c.local_duplex2(*small), want[1])                                # not polluted by the big one
        # the last tile is an ordinary computed indexed batch: windows 2 of s1 with windows 4, 5 of s2
        ns, index = c.batch_index()
        assert ns == 3 and index == [(0, 1), (0, 2)]
        hp0 = c.batch_results(0)["hp"]
        assert hp0.shape == (17, 17)
        one = fresh_like(ctx, model, source == "cofold")
        ref0 = (one.cofold if source == "cofold" else one.duplex)(small[0][7:23], small[1][20:36])[0]
        one.close()
        assert_prob_close(hp0, ref0, rel=REL, what="pair 0 of the last tile")
        for bad in (("", small[1], 16, 5, 16, 5), (small[0], "", 16, 5, 16, 5), (small[0], small[1], 1, 1, 16, 5), (small[0], small[1], 16, 5, 16, 0),
                    (small[0], small[1], 16, 17, 16, 5)):
            with pytest.raises(ractip_amd.RhError, match="local duplex2"):
                c.local_duplex2(*bad)
        assert same(c.local_hp2_results(), want[1])                                  # a rejected call leaves hp2 ...
        assert same(c.local_hp_results() + (dup0[2],) + c.local_results(), dup0)      # ... the 1-D local results ...
        assert np.array_equal(c.batch_results(0)["hp"], hp0)                         # ... and the batch in place
        assert same(c.local_fold(small[1], 16, 5), fold0)
        assert same(c.local_hp2_results(), want[1])
        assert same(c.local_duplex(small[0], small[1], 16, 5, 2) + c.local_results(), dup0)
        assert same(c.local_hp2_results(), want[1])
        ms = c.local_hp2_times()
        assert ms[0] > 0.0 and ms[1] > 0.0
    finally:
        c.close()


# ---- 7. pipeline
@pytest.mark.parametrize("model", ["vienna", "contrafold"])
def test_predict_with_a_window_no_shorter_than_the_molecules(hotlib, model):
    fa = [l.strip() for l in open(os.path.join(ROOT, "ractip_amd", "data", "config5_OxyS_fhlA.fa")) if not l.startswith(">")]
    s1, s2 = fa[0], fa[1]
    W = max(len(s1), len(s2))
    whole = pipeline.predict(s1, s2, model=model)
    local = pipeline.predict(s1, s2, model=model, window=W, step=10, local_hp_both=True)
    assert local[0] == whole[0] and local[1] == whole[1]
    assert set(whole[0]) > {"."} or set(whole[1]) > {"."}      # (a prediction with structure in it)
    r = pipeline.local_duplex2(s1[:50], s2[:60], 40, step1=4, window2=30, step2=7, model=model)
    assert r["hp"].shape == (51, 61) and r["logz_pair"].shape == (len(r["starts1"]), len(r["starts2"]))
    assert list(r["starts1"]) == windows(50, 40, 4) and list(r["starts2"]) == windows(60, 30, 7)


QUERY = "AAUAGGUUACGAUGAGCUACGGCC"
TARGET = "GCUGGAAGUACAAUUAUAUUGAGUGGACUGACGGAGCCGAUCGACUUAACGUGAGCGAACGUCGUGGACUGUAGCUCAUCGUAACCAUUUGACCUGCCUUUUGCGGGCUUAUUGAUGAGA"
LONG1 = "GGUCCUGGCCCUAAGCAGUGUUAAGUUGACGGUCGCGUAAUAGGUUACGAUGAGCUACGGCCCAAUCGACCAAACUGUAGAGCGGGUAUAUCCCUCGGGA"


def test_predict_finds_a_planted_site_in_two_windowed_molecules(hotlib):
    """Vienna model, default (cofold) source, (W, S) = (40, 10) on both molecules: letters 43-58 of s1 are query letters 5-20 of
    tests/test_gpu_local_duplex.py, and their reverse complement is s2 letters 71-86.  On the CPU-oracle 2-D average the hp row sums of
    the planted letters of s1 over the planted columns are at least 0.822; the predicted joint structure must carry an interaction
    bracket on at least 12 of the 16 planted letters of each side (with oracle local folds the ILP gives 15 of 16)."""
    W, S = 40, 10
    assert len(LONG1) == 100 and LONG1[42:58] == QUERY[4:20]
    assert TARGET[70:86] == "".join(COMPLEMENT[ch] for ch in reversed(LONG1[42:58]))
    want, _, _, _ = oracle_average2("cofold", LONG1, TARGET, (len(LONG1), W, S, len(TARGET), W, S))
    sums = want[43:59, 71:87].sum(axis=1)
    print("planted site, W = %d, S = %d: oracle row sums min %.3f, largest whole row sum %.3f" % (W, S, sums.min(), want.sum(axis=1).max()))
    assert sums.min() > 0.7
    r1, r2, _ = pipeline.predict(LONG1, TARGET, model="vienna", window=W, step=S, local_hp_both=True)
    on_s1, on_s2 = sum(ch == "[" for ch in r1[42:58]), sum(ch == "]" for ch in r2[70:86])
    print(r1, r2, on_s1, on_s2, sep="\n")
    assert on_s1 >= 12 and on_s2 >= 12
