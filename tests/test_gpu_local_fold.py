"""GPU suite: local folding (rh_local_fold) -- window-averaged bp and accessibility of a long sequence, both models, both
arithmetic paths (the `ctx` fixture; the Vienna-BL and region-accessibility contexts follow its path).

The definition, restated here (windows, average): starts 0, S, .. and a last window that ends the sequence; an entry is the plain
sum, in increasing window order, of the windows that contain its run, divided once by their number.  Three kinds of check:
  * against the CPU oracles, each window folded by the oracle and averaged in numpy (rel 1e-6, log Z 1e-9);
  * bit for bit against the numpy average of what the SAME context returns for the windows uploaded as an indexed batch, under
    chunks of 1, 3 and the automatic size -- the accumulate / finish kernels add nothing but the defined arithmetic;
  * zeros, candidates, reuse of one context, the pipeline.
Shapes: W = 16 and 33 (below kStripMinN = 40), 65 and 200 (strips, two 64-column groups), n on both sides of W, steps on and off
the grid, disjoint tiles (S = W)."""
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
PARITY = [(41, 16, 1), (43, 16, 5), (17, 16, 1), (16, 16, 1), (9, 16, 1), (48, 16, 16), (50, 16, 16), (70, 65, 1), (40, 33, 2)]
IDENTITY = [(230, 200, 7), (70, 65, 1), (43, 16, 5)]
VIENNA_W = 5


def seq_of(n):
    return "".join(np.random.RandomState(20261020 + n).choice(list("ACGU"), n))


# ---- the definition, restated
def windows(n, W, S):
    if n <= W:
        return [0]
    m = -(-(n - W) // S)
    return [k * S for k in range(m)] + [n - W]


def tri_rows(tri, n):
    """(n, n) band of a triangular table of n letters: row a (0-based), column d = bp(a, a + d)"""
    band = np.zeros((n, n))
    for a in range(n):
        at = hot.tri_offset(n, a + 1) + a + 2
        band[a, 1:n - a] = tri[at:at + n - a - 1]
    return band


def average(n, W, S, bp_tris, ups, max_w):
    """bp_band (n, We) and up (n, max_w) from the per-window triangular tables and (We, max_w) accessibilities: the sum in
    increasing window order, one division by the count, 0 where no window holds the run"""
    We, starts = min(W, n), windows(n, W, S)
    band, cb = np.zeros((n, We)), np.zeros((n, We))
    up, cu = np.zeros((n, max_w)), np.zeros((n, max_w))
    a, d, w = np.arange(We)[:, None], np.arange(We)[None, :], np.arange(max_w)[None, :]
    in_bp, in_up = (d >= 1) & (a + d < We), a + w < We
    for k, s in enumerate(starts):
        band[s:s + We] += np.where(in_bp, tri_rows(np.asarray(bp_tris[k]), We), 0.0)
        cb[s:s + We] += in_bp
        up[s:s + We] += np.where(in_up, np.asarray(ups[k]).reshape(We, max_w), 0.0)
        cu[s:s + We] += in_up
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cb > 0, band / cb, 0.0), np.where(cu > 0, up / cu, 0.0), cb, cu


# ---- contexts
@pytest.fixture(scope="module")
def vctx(ctx):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    c.set_mode(MODE[ctx.path_name])
    c.set_max_w(VIENNA_W)
    yield c
    c.close()


@pytest.fixture(scope="module")
def acc(ctx):
    c = ractip_amd.Context(device=0)
    c.set_mode(MODE[ctx.path_name])
    c.set_region_accessibility(True)
    c.set_max_w(4)
    yield c
    c.close()


def fresh_like(c, model):
    """a new context of `model` on the arithmetic path of the `ctx` fixture c"""
    f = ractip_amd.Context(device=0, model=model)
    f.set_mode(MODE[c.path_name])
    if model == hot.RH_MODEL_VIENNA_BL:
        f.set_max_w(VIENNA_W)
    return f


# ---- oracle references, once per window string
_cf, _vo = {}, {}
_oracles = {}


def cf_window(s):
    if s not in _cf:
        o = _oracles.setdefault("cf", Oracle()).inference(s)
        n = len(s)
        rows = tri_rows(o["post"], n)
        full = np.zeros((n, n))
        for a in range(n):
            for d in range(1, n - a):
                full[a, a + d] = full[a + d, a] = rows[a, d]
        _cf[s] = (o["post"], np.maximum(0.0, 1.0 - full.sum(axis=1)).reshape(n, 1), o["logZ"])
    return _cf[s]


def vo_window(s):
    if s not in _vo:
        o = _oracles.setdefault("vo", ViennaOracle()).mccaskill(s, max_w=VIENNA_W)
        _vo[s] = (o["post"], o["up"], o["logZ"])
    return _vo[s]


def check_parity(c, fold_window, max_w, n, W, S, what):
    seq = seq_of(n)
    We, starts = min(W, n), windows(n, W, S)
    band, up, logz, got_starts = c.local_fold(seq, W, S)
    assert list(got_starts) == starts and band.shape == (n, We) and up.shape == (n, max_w)
    ref = [fold_window(seq[s:s + We]) for s in starts]
    want_band, want_up, _, _ = average(n, W, S, [r[0] for r in ref], [r[1] for r in ref], max_w)
    assert np.abs(logz - np.array([r[2] for r in ref])).max() < 1e-9, what
    assert_prob_close(band, want_band, rel=REL, what="bp " + what)
    assert_prob_close(up, want_up, rel=REL, what="up " + what)


@pytest.mark.parametrize("n,W,S", PARITY)
def test_contrafold_against_the_oracle(ctx, n, W, S):
    check_parity(ctx, cf_window, 1, n, W, S, "CONTRAfold %s %r" % (ctx.path_name, (n, W, S)))


@pytest.mark.parametrize("n,W,S", PARITY)
def test_vienna_against_the_oracle(vctx, ctx, n, W, S):
    check_parity(vctx, vo_window, VIENNA_W, n, W, S, "Vienna-BL %s %r" % (ctx.path_name, (n, W, S)))


# ---- accumulation identity, bit for bit
def per_window(c, seq, n, W, S):
    """what the context itself returns for the windows, uploaded as an indexed batch (pair k = window k with itself)"""
    We, starts = min(W, n), windows(n, W, S)
    wins = [seq[s:s + We] for s in starts]
    c.batch_upload_indexed(wins, [(k, k) for k in range(len(wins))])
    c.batch_compute()
    r = c.batch_results_all()
    return r["bp"], r["up"], r["logZ"][:, 0].copy()


def check_identity(c, n, W, S, what):
    seq, max_w = seq_of(n), c.max_w
    bps, ups, logz = per_window(c, seq, n, W, S)
    want_band, want_up, _, _ = average(n, W, S, bps, ups, max_w)
    try:
        for chunk in (1, 3, 0):
            c.set_local_chunk(chunk)
            band, up, lz, _ = c.local_fold(seq, W, S)
            assert np.array_equal(band, want_band), "%s chunk %d: band" % (what, chunk)
            assert np.array_equal(up, want_up), "%s chunk %d: up" % (what, chunk)
            assert np.array_equal(lz, logz), "%s chunk %d: log Z" % (what, chunk)
    finally:
        c.set_local_chunk(0)


@pytest.mark.parametrize("n,W,S", IDENTITY)
def test_contrafold_band_is_the_ordered_sum_of_its_windows(ctx, n, W, S):
    check_identity(ctx, n, W, S, "CONTRAfold %s %r" % (ctx.path_name, (n, W, S)))


@pytest.mark.parametrize("n,W,S", IDENTITY)
def test_vienna_band_is_the_ordered_sum_of_its_windows(vctx, ctx, n, W, S):
    check_identity(vctx, n, W, S, "Vienna-BL %s %r" % (ctx.path_name, (n, W, S)))


@pytest.mark.parametrize("n,W,S", [(70, 65, 1), (43, 16, 5)])
def test_region_accessibility_band_is_the_ordered_sum_of_its_windows(acc, ctx, n, W, S):
    assert acc.max_w == 4
    check_identity(acc, n, W, S, "CONTRAfold region accessibility %s %r" % (ctx.path_name, (n, W, S)))


# ---- a window no shorter than the sequence
@pytest.mark.parametrize("n,W", [(9, 16), (16, 16), (70, 100)])
def test_one_window_has_the_bits_of_rh_fold(ctx, vctx, n, W):
    seq = seq_of(n)
    for c in (ctx, vctx):
        bp, up, z = c.fold(seq)
        band, lup, logz, starts = c.local_fold(seq, W, 3)
        assert list(starts) == [0] and band.shape == (n, n)
        assert np.array_equal(band, tri_rows(bp, n))
        assert np.array_equal(lup, np.asarray(up).reshape(n, -1))
        assert logz.shape == (1,) and logz[0] == z


# ---- zeros
@pytest.mark.parametrize("n,W,S", [(50, 16, 16), (52, 16, 9)])
def test_zeros_where_the_definition_says_zero(ctx, vctx, n, W, S):
    seq, We, starts = seq_of(n), min(W, n), windows(n, W, S)

    def covered(i, ln):
        return i + ln <= n and any(s <= i and i + ln <= s + We for s in starts)

    for c in (ctx, vctx):
        band, up, _, _ = c.local_fold(seq, W, S)
        assert not band[:, 0].any()
        holes = 0
        for i in range(n):
            for d in range(1, We):
                if not covered(i, d + 1):
                    assert band[i, d] == 0.0, (i, d)
                    holes += i + d < n
            for w in range(up.shape[1]):
                if not covered(i, w + 1):
                    assert up[i, w] == 0.0, (i, w)
                elif c is vctx:
                    assert up[i, w] > 0.0, (i, w)   # (a sum of positive weights; the CONTRAfold width-1 column is clamped at 0)
        assert holes > 0   # runs inside the sequence that no window holds (pairs across a tile border)
        if S == W:
            assert band[15, 1] == 0.0 and band[31, 1] == 0.0


# ---- candidates
def scan(values, e0, last, record):
    """row-major numpy scan: float narrowing, then p > th"""
    def go(th):
        out = []
        v32 = values.astype(np.float32)
        for i in range(values.shape[0]):
            for e in range(e0, min(values.shape[1] - 1, last - i) + 1):
                if v32[i, e] > np.float32(th):
                    out.append(record(i, e) + (v32[i, e],))
        return out
    return go


def test_candidates_equal_a_numpy_scan_of_the_fetched_result(ctx, vctx):
    n, W, S = 43, 16, 5
    seq = seq_of(n)
    for c, th_bp, th_up in ((ctx, 0.01, 0.2), (vctx, 0.003, 0.05)):
        band, up, _, _ = c.local_fold(seq, W, S)
        want_bp = scan(band, 1, n - 1, lambda i, d: (i + 1, i + 1 + d))(th_bp)
        want_up = scan(up, 0, n + 64, lambda i, w: (i, w))(th_up)
        assert len(want_bp) > 8 and len(want_up) > 8
        for what, th, want in ((0, th_bp, want_bp), (1, th_up, want_up)):
            rec, total = c.local_candidates(what, th)
            assert total == len(want)
            assert [(int(r["i"]), int(r["j"]), r["p"]) for r in rec] == want
            rec, total = c.local_candidates(what, th, cap=5)       # too small: the first records, the whole count
            assert total == len(want) and [(int(r["i"]), int(r["j"]), r["p"]) for r in rec] == want[:5]
        # an entry exactly at the threshold is not reported: p > th on the narrowed value
        p0 = float(want_bp[0][2])
        rec, total = c.local_candidates(0, p0)
        assert total == sum(1 for r in want_bp if r[2] > np.float32(p0)) and total < len(want_bp)


# ---- reuse of one context
@pytest.mark.parametrize("model", [hot.RH_MODEL_CONTRAFOLD, hot.RH_MODEL_VIENNA_BL], ids=["contrafold", "vienna"])
def test_reuse_has_the_bits_of_a_fresh_context(ctx, model):
    big, small = (seq_of(230), 200, 7), (seq_of(43), 16, 5)
    want = []
    for args in (big, small):
        f = fresh_like(ctx, model)
        want.append(f.local_fold(*args))
        f.close()
    c = fresh_like(ctx, model)
    try:
        def same(got, k):
            return all(np.array_equal(a, b) for a, b in zip(got, want[k]))
        assert same(c.local_fold(*big), 0)
        assert same(c.local_fold(*small), 1)
        pair = (seq_of(41), seq_of(23))
        c.batch_upload([pair])
        c.batch_compute()
        hp = c.batch_results(0)["hp"]
        assert same(c.local_results(), 1)                       # the local result lives in buffers of its own
        for bad in ((small[0], 1, 1), (small[0], 16, 0), (small[0], 16, 17), ("", 16, 1)):
            with pytest.raises(ractip_amd.RhError, match="local fold"):
                c.local_fold(*bad)
        assert same(c.local_results(), 1)                       # a rejected call leaves the earlier result ...
        assert np.array_equal(c.batch_results(0)["hp"], hp)     # ... and the earlier batch in place
        assert same(c.local_fold(*small), 1)
        with pytest.raises(ractip_amd.RhError, match="no computed pair batch"):
            c.batch_results(0)
        with pytest.raises(ractip_amd.RhError, match="no computed pair batch"):
            c.batch_logz()
        ms = c.local_times()
        assert ms[0] > 0.0 and ms[1] > 0.0
    finally:
        c.close()


def test_no_local_result_before_the_first_local_fold(ctx):
    c = fresh_like(ctx, hot.RH_MODEL_CONTRAFOLD)
    try:
        with pytest.raises(ractip_amd.RhError, match="no local fold result"):
            c.local_results()
        with pytest.raises(ractip_amd.RhError, match="rh_set_local_chunk"):
            c.set_local_chunk(-1)
    finally:
        c.close()


# ---- pipeline
def test_band_to_tri_round_trips():
    rng = np.random.RandomState(5)
    for n, ld in ((9, 5), (16, 16), (7, 2), (1, 1)):
        band = rng.rand(n, ld)
        band[:, 0] = 0.0
        for i in range(n):
            band[i, max(1, n - i):] = 0.0
        tri = hot.band_to_tri(band)
        assert tri.shape == (hot.tri_size(n),)
        for i in range(n):
            for d in range(1, min(ld, n - i)):
                assert tri[hot.tri_offset(n, i + 1) + i + 1 + d] == band[i, d]
        assert np.count_nonzero(tri) == np.count_nonzero(band)
        assert np.array_equal(tri_rows(tri, n)[:, :ld], band)


@pytest.mark.parametrize("model", ["vienna", "contrafold"])
def test_predict_with_a_window_no_shorter_than_the_molecules(hotlib, model):
    fa = [l.strip() for l in open(os.path.join(ROOT, "ractip_amd", "data", "config5_OxyS_fhlA.fa")) if not l.startswith(">")]
    s1, s2 = fa[0], fa[1]
    W = max(len(s1), len(s2))
    whole = pipeline.predict(s1, s2, model=model)
    local = pipeline.predict(s1, s2, model=model, window=W, step=10)
    assert local[0] == whole[0] and local[1] == whole[1]
    assert set(whole[0]) > {"."} or set(whole[1]) > {"."}      # (a prediction with structure in it)
    r = pipeline.local_fold(s1, 40, step=4, model=model)
    assert r["bp_band"].shape == (len(s1), 40) and r["starts"][-1] == len(s1) - 40
