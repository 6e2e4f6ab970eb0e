"""GPU suite: local hybridization (rh_local_duplex) -- the window-averaged hp of a query on a longer target, both models, the three
hybridization sources, both arithmetic paths (the `ctx` fixture; the Vienna-BL contexts follow its path).

The definition, restated here: one molecule (`windowed` = 1 or 2) is cut into the windows of local folding (starts 0, S, .. and a last
window that ends the sequence), the other one -- the query -- is whole; hp_k is the hybridization matrix of (query, window k) or
(window k, query); hp_loc(i, j) is the plain sum, in increasing window order, of hp_k at the translated coordinates over the windows
that contain the windowed molecule's letter, divided once by their number.  Kinds of check:
  * against the CPU oracles, each window pair from the oracle and averaged in numpy (rel 1e-6, log Z 1e-9);
  * bit for bit against the numpy average of what the SAME context returns for query + windows uploaded as an indexed batch, under
    chunks of 1, 3 and the automatic size, with the fold part equal to a plain local_fold of the windowed molecule;
  * one window = Context.duplex, zeros, candidates, reuse and rejection, the pipeline with a planted site.
Shapes: queries of 7, 23, 60 letters (60 crosses the 58-column duplex group), windows of 16, 33, 65, windowed molecules of 9 .. 70
letters, steps 1, 5 and S = W, off-grid last windows, joint lengths of 23, 56 and 125 (both sides of kStripMinN = 40 and of one
64-column group), both roles."""
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
# (nq, n, W, S, windowed): joint lengths 23, 56, 125; S = 1, 5, W; off-grid last windows (43, 16, 5) and (50, 33, 33); n < W, n = W
PARITY = [(7, 41, 16, 1, 2), (23, 43, 16, 5, 1), (23, 50, 33, 33, 2), (60, 70, 65, 1, 2), (60, 70, 65, 1, 1), (60, 9, 16, 1, 1), (7, 16, 16, 1, 2)]
IDENTITY = [(7, 41, 16, 1, 2), (23, 43, 16, 5, 1), (23, 50, 33, 33, 1), (60, 70, 65, 1, 2), (23, 43, 33, 5, 2)]


def seq_of(n, salt=0):
    return "".join(np.random.RandomState(20261020 + n + 1000 * salt).choice(list("ACGU"), n))


def molecules(nq, n, windowed):
    """(s1, s2): the query of nq letters and the windowed molecule of n letters in their roles"""
    q, t = seq_of(nq, 1), seq_of(n)
    return (q, t) if windowed == 2 else (t, q)


# ---- the definition, restated
def windows(n, W, S):
    if n <= W:
        return [0]
    m = -(-(n - W) // S)
    return [k * S for k in range(m)] + [n - W]


def window_pairs(s1, s2, W, S, windowed):
    """the pairs (a_k, b_k) whose hp_k the definition averages, and the starts"""
    t = s2 if windowed == 2 else s1
    We, starts = min(W, len(t)), windows(len(t), W, S)
    return [(s1, t[s:s + We]) if windowed == 2 else (t[s:s + We], s2) for s in starts], starts


def average_hp(n1, n2, W, S, windowed, hps):
    """hp_loc (n1+1, n2+1) from the per-window matrices: the sum in increasing window order, one division by the count"""
    n = n2 if windowed == 2 else n1
    We, starts = min(W, n), windows(n, W, S)
    acc, cnt = np.zeros((n1 + 1, n2 + 1)), np.zeros(n + 1)
    for s, h in zip(starts, hps):
        h = np.asarray(h)
        if windowed == 2:
            assert h.shape == (n1 + 1, We + 1)
            acc[1:, s + 1:s + We + 1] += h[1:, 1:]
        else:
            assert h.shape == (We + 1, n2 + 1)
            acc[s + 1:s + We + 1, 1:] += h[1:, 1:]
        cnt[s + 1:s + We + 1] += 1
    assert cnt[1:].min() >= 1                                   # every letter lies in a window: no holes
    if windowed == 2:
        acc[1:, 1:] /= cnt[None, 1:]
    else:
        acc[1:, 1:] /= cnt[1:, None]
    return acc, cnt


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


SOURCES = ["contrafold", "pf_duplex", "cofold"]


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


def oracle_average(source, s1, s2, W, S, windowed):
    pairs, starts = window_pairs(s1, s2, W, S, windowed)
    ref = [oracle_pair(source, a, b) for a, b in pairs]
    want, _ = average_hp(len(s1), len(s2), W, S, windowed, [r[0] for r in ref])
    return want, np.array([r[1] for r in ref]), starts


def check_parity(c, source, nq, n, W, S, windowed, what):
    s1, s2 = molecules(nq, n, windowed)
    want, want_z, starts = oracle_average(source, s1, s2, W, S, windowed)
    hp, logz, got_starts = c.local_duplex(s1, s2, W, S, windowed)
    assert list(got_starts) == starts and hp.shape == (len(s1) + 1, len(s2) + 1) and logz.shape == (len(starts),)
    assert np.abs(logz - want_z).max() < 1e-9, what
    assert_prob_close(hp, want, rel=REL, what="hp " + what)


# ---- 1. against the CPU oracles
@pytest.mark.parametrize("nq,n,W,S,windowed", PARITY)
@pytest.mark.parametrize("source", SOURCES)
def test_against_the_oracle(ctx, vctx, source, nq, n, W, S, windowed):
    c = context_of(source, ctx, vctx)
    check_parity(c, source, nq, n, W, S, windowed, "%s %s %r" % (source, ctx.path_name, (nq, n, W, S, windowed)))


def test_vienna_duplex_under_its_own_duplex_mode(ctx, vctx):
    """rh_set_duplex_mode(RH_MODE_AUTO): the pf_duplex sweeps on the scaled linear kernels whatever the folds run on"""
    c = context_of("pf_duplex", ctx, vctx)
    c.set_duplex_mode(hot.RH_MODE_AUTO)
    try:
        check_parity(c, "pf_duplex", 23, 43, 16, 5, 2, "pf_duplex, duplex mode auto, folds %s" % ctx.path_name)
        assert c.last_hybrid_path() == 1
    finally:
        c.set_duplex_mode(hot.RH_MODE_INHERIT)


# ---- 2. accumulation identity, bit for bit
def per_window(c, s1, s2, W, S, windowed):
    """what the context itself returns for query + windows, uploaded as one indexed batch"""
    pairs, starts = window_pairs(s1, s2, W, S, windowed)
    query = s1 if windowed == 2 else s2
    wins = [p[1] if windowed == 2 else p[0] for p in pairs]
    index = [(0, 1 + k) if windowed == 2 else (1 + k, 0) for k in range(len(wins))]
    c.batch_upload_indexed([query] + wins, index)
    c.batch_compute()
    r = c.batch_results_all()
    return [np.array(h) for h in r["hp"]], r["logZ"][:, 2].copy()


@pytest.mark.parametrize("nq,n,W,S,windowed", IDENTITY)
@pytest.mark.parametrize("source", SOURCES)
def test_hp_is_the_ordered_sum_of_its_windows(ctx, vctx, source, nq, n, W, S, windowed):
    c = context_of(source, ctx, vctx)
    what = "%s %s %r" % (source, ctx.path_name, (nq, n, W, S, windowed))
    s1, s2 = molecules(nq, n, windowed)
    hps, logz = per_window(c, s1, s2, W, S, windowed)
    want, _ = average_hp(len(s1), len(s2), W, S, windowed, hps)
    fold = c.local_fold(s2 if windowed == 2 else s1, W, S)
    try:
        for chunk in (1, 3, 0):
            c.set_local_chunk(chunk)
            hp, lz, _ = c.local_duplex(s1, s2, W, S, windowed)
            assert np.array_equal(hp, want), "%s chunk %d: hp" % (what, chunk)
            assert np.array_equal(lz, logz), "%s chunk %d: log Z" % (what, chunk)
            for got, ref, name in zip(c.local_results(), fold, ("band", "up", "log Z", "starts")):
                assert np.array_equal(got, ref), "%s chunk %d: %s of the windowed molecule" % (what, chunk, name)
    finally:
        c.set_local_chunk(0)


# ---- 3. a window no shorter than the windowed molecule
@pytest.mark.parametrize("nq,n,W", [(7, 9, 16), (23, 16, 16), (60, 50, 65), (60, 70, 100)])
@pytest.mark.parametrize("source", SOURCES)
def test_one_window_has_the_bits_of_rh_duplex(ctx, vctx, source, nq, n, W):
    """With W >= n the result has the bits of Context.duplex(s1, s2) under the same settings, in both roles.  Under the cofold source on
    the scaled linear path that takes a rule of its own: rh_duplex stages the pair without its folds, so its two-molecule sweeps
    compute their one-strand cells themselves, while a batch with folds copies them from the folds (vlin_co_seed), and the two orders
    of summation differ in the last bits (up to 2.2e-16 on these shapes).  A call with one window therefore runs its one compute
    unseeded, like rh_duplex; with two windows or more every chunk is seeded, like any batch (test 2).  DESIGN.md 5.1j."""
    c = context_of(source, ctx, vctx)
    for windowed in (1, 2):
        s1, s2 = molecules(nq, n, windowed)
        hp, z = c.duplex(s1, s2)
        got, logz, starts = c.local_duplex(s1, s2, W, 3, windowed)
        assert list(starts) == [0] and logz.shape == (1,)
        print("one window %s %s %r windowed %d: max |local - duplex| = %.3e, log Z %.3e" % (
            source, ctx.path_name, (nq, n, W), windowed, np.abs(got - hp).max(), abs(logz[0] - z)))
        assert np.array_equal(got, hp) and logz[0] == z


@pytest.mark.parametrize("nq,n,W", [(7, 9, 16), (23, 16, 16), (60, 50, 65), (60, 70, 100)])
@pytest.mark.parametrize("source", SOURCES)
def test_one_window_has_the_bits_of_the_pair_batch(ctx, vctx, source, nq, n, W):
    """... and the fold part has the bits of the pair as a plain batch of one (what pipeline.probabilities computes); so has hp, except
    under the cofold source, where the batch's sweeps are seeded from its folds and the one window's are not (see above): there
    the two agree to the project's tolerance, and bit for bit on the log-space path, which never seeds"""
    c = context_of(source, ctx, vctx)
    for windowed in (1, 2):
        s1, s2 = molecules(nq, n, windowed)
        c.batch_upload([(s1, s2)])
        c.batch_compute()
        r = c.batch_results(0)
        got, logz, starts = c.local_duplex(s1, s2, W, 3, windowed)
        assert list(starts) == [0]
        if source == "cofold" and ctx.path_name == "auto":
            assert_prob_close(got, r["hp"], rel=REL, what="hp, seeded against unseeded")
            assert abs(logz[0] - r["logZ"][2]) < 1e-9
        else:
            assert np.array_equal(got, r["hp"]) and logz[0] == r["logZ"][2]
        band, up, lz, _ = c.local_results()
        assert np.array_equal(hot.band_to_tri(band), r["bp%d" % windowed]) and lz[0] == r["logZ"][windowed - 1]
        assert np.array_equal(up, np.asarray(r["up%d" % windowed]).reshape(up.shape))


# ---- 4. zeros and counts
@pytest.mark.parametrize("nq,n,W,S,windowed", [(23, 43, 16, 5, 2), (23, 50, 16, 16, 1)])
def test_zeros_and_positive_entries(ctx, vctx, nq, n, W, S, windowed):
    s1, s2 = molecules(nq, n, windowed)
    pairable = {"AU", "UA", "CG", "GC", "GU", "UG"}
    for source in SOURCES:
        c = context_of(source, ctx, vctx)
        hp, _, _ = c.local_duplex(s1, s2, W, S, windowed)
        assert not hp[0].any() and not hp[:, 0].any()
        assert np.isfinite(hp).all() and hp.min() >= 0.0 and hp.max() <= 1.0 + 1e-12
        _, cnt = average_hp(len(s1), len(s2), W, S, windowed, [np.zeros((len(a) + 1, len(b) + 1)) for a, b in window_pairs(s1, s2, W, S, windowed)[0]])
        assert cnt[1:].min() >= 1 and cnt[1:].max() > 1
        if source == "cofold":
            # interior = not next to the cut: co_pf_fold keeps TURN = 3 letters between the partners of a pair in the concatenation, so
            # in the pair (a, b) the entry (ia, jb) is 0 by construction iff (len(a) - ia) + jb <= 3; an entry of hp_loc is interior
            # if some window that contains its letter holds it further from the cut than that
            We, starts = min(W, n), windows(n, W, S)
            interior = np.zeros(hp.shape, dtype=bool)
            i, j = np.arange(1, len(s1) + 1)[:, None], np.arange(1, len(s2) + 1)[None, :]
            for st in starts:
                if windowed == 2:
                    interior[1:, 1:] |= (j > st) & (j <= st + We) & ((len(s1) - i) + (j - st) > 3)
                else:
                    interior[1:, 1:] |= (i > st) & (i <= st + We) & ((st + We - i) + j > 3)
            comp = np.array([[a + b in pairable for b in s2] for a in s1])
            assert (interior[1:, 1:] & comp).sum() > 100 and (~interior[1:, 1:] & comp).any()
            assert (hp[1:, 1:][interior[1:, 1:] & comp] > 0.0).all()
            assert not hp[1:, 1:][~comp].any()


# ---- 5. candidates
def scan_hp(hp, th):
    """row-major numpy scan over 1..n1 x 1..n2: float narrowing, then p > th"""
    v32 = hp.astype(np.float32)
    return [(i, j, v32[i, j]) for i in range(1, hp.shape[0]) for j in range(1, hp.shape[1]) if v32[i, j] > np.float32(th)]


@pytest.mark.parametrize("windowed", [1, 2])
def test_candidates_equal_a_numpy_scan_of_the_fetched_matrix(ctx, vctx, windowed):
    s1, s2 = molecules(23, 43, windowed)
    for source, th in (("contrafold", 0.01), ("pf_duplex", 0.003), ("cofold", 1e-4)):
        c = context_of(source, ctx, vctx)
        hp, _, _ = c.local_duplex(s1, s2, 16, 5, windowed)
        want = scan_hp(hp, th)
        assert len(want) > 8, source
        rec, total = c.local_candidates(2, th)
        assert total == len(want)
        assert [(int(r["i"]), int(r["j"]), r["p"]) for r in rec] == want
        rec, total = c.local_candidates(2, th, cap=5)          # too small: the first records, the whole count
        assert total == len(want) and [(int(r["i"]), int(r["j"]), r["p"]) for r in rec] == want[:5]
        p0 = float(want[0][2])                                 # an entry exactly at the threshold is not reported
        rec, total = c.local_candidates(2, p0)
        assert total == sum(1 for r in want if r[2] > np.float32(p0)) and total < len(want)
        # the fold part of the same call still serves what = 0
        band = c.local_results()[0]
        assert c.local_candidates(0, 0.01)[1] == int((band.astype(np.float32) > np.float32(0.01)).sum())


# ---- 6. reuse and rejection
@pytest.mark.parametrize("source", SOURCES)
def test_reuse_and_rejection(ctx, source):
    model = hot.RH_MODEL_CONTRAFOLD if source == "contrafold" else hot.RH_MODEL_VIENNA_BL
    big = molecules(60, 70, 2) + (65, 1, 2)
    small = molecules(23, 43, 1) + (16, 5, 1)
    want = []
    for args in (big, small):
        f = fresh_like(ctx, model, source == "cofold")
        want.append(f.local_duplex(*args) + f.local_results())
        f.close()
    c = fresh_like(ctx, model, source == "cofold")
    try:
        def same(got, k):
            return len(got) == len(want[k]) and all(np.array_equal(a, b) for a, b in zip(got, want[k]))
        with pytest.raises(ractip_amd.RhError, match="no local hybridization result"):
            c.local_hp_results()
        assert same(c.local_duplex(*big) + c.local_results(), 0)
        assert same(c.local_duplex(*small) + c.local_results(), 1)
        # the last chunk is an ordinary computed indexed batch: pair 0 = (window 0, query)
        r = c.batch_results(0)
        first_window = small[0][:16]
        assert r["hp"].shape == (17, 24)
        one = fresh_like(ctx, model, source == "cofold")
        hp0 = (one.cofold if source == "cofold" else one.duplex)(first_window, small[1])[0]
        one.close()
        assert_prob_close(r["hp"], hp0, rel=REL, what="pair 0 of the last chunk")
        hp0 = r["hp"]
        ns, index = c.batch_index()
        assert ns == 1 + len(want[1][2]) and index == [(1 + k, 0) for k in range(ns - 1)]
        for bad in ((small[0], small[1], 1, 1, 1), (small[0], small[1], 16, 0, 1), (small[0], small[1], 16, 17, 1), (small[0], small[1], 16, 5, 3),
                    ("", small[1], 16, 5, 1), (small[0], "", 16, 5, 2)):
            with pytest.raises(ractip_amd.RhError, match="local duplex"):
                c.local_duplex(*bad)
        assert same(c.local_hp_results() + (want[1][2],) + c.local_results(), 1)   # a rejected call leaves local hp, local bp ...
        assert np.array_equal(c.batch_results(0)["hp"], hp0)                       # ... and the batch in place
        fold = c.local_fold(small[0], 16, 5)
        assert all(np.array_equal(a, b) for a, b in zip(fold, want[1][3:]))
        with pytest.raises(ractip_amd.RhError, match="no local hybridization result"):
            c.local_hp_results()
        with pytest.raises(ractip_amd.RhError, match="no local hybridization result"):
            c.local_candidates(2, 0.1)
        assert same(c.local_duplex(*small) + c.local_results(), 1)
        ms = c.local_times()
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
    local = pipeline.predict(s1, s2, model=model, window=W, step=10, local_hp=True)
    assert local[0] == whole[0] and local[1] == whole[1]
    assert set(whole[0]) > {"."} or set(whole[1]) > {"."}      # (a prediction with structure in it)
    with pytest.raises(ValueError, match="local_hp"):
        pipeline.predict(s1, s2, model=model, local_hp=True)
    r = pipeline.local_duplex(s1[:30], s2, 40, step=4, model=model)
    assert r["hp"].shape == (31, len(s2) + 1) and r["bp_band"].shape == (len(s2), 40) and r["starts"][-1] == len(s2) - 40


QUERY = "AAUAGGUUACGAUGAGCUACGGCC"
TARGET = "GCUGGAAGUACAAUUAUAUUGAGUGGACUGACGGAGCCGAUCGACUUAACGUGAGCGAACGUCGUGGACUGUAGCUCAUCGUAACCAUUUGACCUGCCUUUUGCGGGCUUAUUGAUGAGA"
COMPLEMENT = {"A": "U", "U": "A", "C": "G", "G": "C"}


@pytest.mark.parametrize("W,S", [(40, 10), (33, 7)])
def test_predict_finds_a_planted_site_on_a_windowed_target(hotlib, W, S):
    """Vienna model, default (cofold) source: target letters 71-86 are the reverse complement of query letters 5-20.  On the CPU-oracle
    average the hp row sums of those query letters over those target columns are all > 0.7 (0.960 at (40, 10), 0.785 at (33, 7) at
    the least); the predicted joint structure must carry an interaction bracket on at least 12 of the 16 planted letters of each side."""
    assert TARGET[70:86] == "".join(COMPLEMENT[ch] for ch in reversed(QUERY[4:20]))
    want, _, _ = oracle_average("cofold", QUERY, TARGET, W, S, 2)
    sums = want[5:21, 71:87].sum(axis=1)
    print("planted site, W = %d, S = %d: oracle row sums min %.3f" % (W, S, sums.min()))
    assert sums.min() > 0.7
    r1, r2, _ = pipeline.predict(QUERY, TARGET, model="vienna", window=W, step=S, local_hp=True)
    on_query, on_target = sum(ch == "[" for ch in r1[4:20]), sum(ch == "]" for ch in r2[70:86])
    print(r1, r2, on_query, on_target, sep="\n")
    assert on_query >= 12 and on_target >= 12
