"""GPU suite: span-limited folding (rh_span_fold) -- the McCaskill ensemble of the whole sequence under the Vienna-BL model, pairs
(a, b) only with b - a < L -- against the CPU oracle under the band mask (tests/_span_cases.py; the mask is pinned against the
enumeration by tests/test_span_fold_cpu.py): band and up at rel 1e-6 above 1e-12, log Z at 1e-9.

Shapes (random ACGU with one N planted): no pair possible (L = 2, 4) and the first possible pair (L = 5); the reach of the interior
loops (L = 31..34); the wavefront edge of the multiloop rows (L = 63..65 at n = 130); the exterior passes' blocks of 64 entries
(n = 64, 65, 66 at L >= n; n = 128, 129: the last block full, and one entry in the next); two workgroup columns of 256 cells
(n = 256..258); table rows without padding (n = 47: ldn = n + 1 = 48) -- every other shape has padded rows; L >= n, also against
Context.fold of the same context; L = n - 1 on a sequence whose end pair matters.  The contexts are Vienna-BL at max_w 1 and 5: the
setting is ignored.  Then the interface: layout, candidates, what a span fold replaces and what a refusal keeps, reuse."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot, pipeline
import _span_cases as sc
from _oracle import assert_log_close, assert_prob_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RH_ERR_ARG, RH_ERR_UNSUPPORTED = -1, -5
END_PAIR = "GGGCGCGG" + sc.random_seq(54, seed=3, plant_n=False) + "CCGCGCCC"   # P(1, 70) > 1e-3
SHAPES = [(40, 2), (40, 4), (40, 5), (90, 31), (90, 32), (90, 33), (90, 34), (130, 63), (130, 64), (130, 65), (256, 20), (257, 20),
          (258, 20), (300, 60), (70, 70), (70, 500), (64, 70), (65, 70), (66, 70), (128, 40), (129, 40), (47, 20)]


@pytest.fixture(scope="module", params=[1, 5], ids=["max_w1", "max_w5"])
def vctx(hotlib, request):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    c.set_max_w(request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def v1(hotlib):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    yield c
    c.close()


def check(got, ref, what):
    band, up, logz = got
    assert band.shape == ref["band"].shape and up.shape == ref["up"].shape, what
    assert_log_close([logz], [ref["logZ"]], what=what + " log Z")
    assert_prob_close(band, ref["band"], what=what + " band")
    assert_prob_close(up, ref["up"], what=what + " up")
    n, ld = band.shape
    i, d = np.arange(n)[:, None], np.arange(ld)[None, :]
    assert not band[(d == 0) | (i + d >= n)].any(), what + ": column 0 and the entries past the end hold 0"


# ---- parity
@pytest.mark.parametrize("n,L", SHAPES)
def test_parity_with_the_masked_oracle(vctx, n, L):
    seq = sc.random_seq(n)
    assert "N" in seq
    check(vctx.span_fold(seq, L), sc.masked(seq, L), "n=%d L=%d" % (n, L))


@pytest.mark.parametrize("L", [2, 4])
def test_no_pair_is_possible(vctx, L):
    band, up, logz = vctx.span_fold(sc.random_seq(40), L)
    assert not band.any() and (up == 1.0).all() and logz == 0.0


def test_the_first_possible_pair(v1):
    seq = sc.random_seq(40)
    band, _, logz = v1.span_fold(seq, 5)
    assert logz > 0.0 and band[:, 4].any() and not band[:, :4].any()


@pytest.mark.parametrize("L", [70, 500])
def test_span_at_least_the_length_is_the_whole_fold(vctx, L):
    seq = sc.random_seq(70)
    band, up, logz = vctx.span_fold(seq, L)
    bp, fup, z = vctx.fold(seq)
    assert band.shape == (70, 70)
    assert_log_close([logz], [z], what="log Z against Context.fold")
    assert_prob_close(band, sc.tri_to_band(bp, 70, 70), rel=1e-9, what="band against Context.fold")
    assert_prob_close(up[:, 0], np.asarray(fup).reshape(70, -1)[:, 0], rel=1e-9, what="up against Context.fold")


def test_one_letter_below_the_length_differs_from_the_whole_fold(v1):
    n = len(END_PAIR)
    whole, below = sc.masked(END_PAIR, None), sc.masked(END_PAIR, n - 1)
    assert whole["band"][0, n - 1] > 1e-3 and abs(whole["logZ"] - below["logZ"]) > 1e-4
    got = v1.span_fold(END_PAIR, n - 1)
    check(got, below, "end pair, L = n - 1")
    assert_prob_close(hot.band_to_tri(got[0]), below["post"], what="band_to_tri of the result")
    assert abs(got[2] - whole["logZ"]) > 1e-4
    check(v1.span_fold(END_PAIR, n), sc.masked(END_PAIR, n), "end pair, L = n")


def test_the_exponent_ladder_takes_over_where_the_band_overflows(v1):
    """A chain of stable hairpins, 1300 letters at L = n: log Z - s n under the default exponent s = 0.28 lies beyond the flag's
    1e280, so the first attempt is flagged and the call answers from a larger exponent of the ladder -- with the whole fold's
    values (Context.fold takes its own ladder), and the context's fold bits are what they were."""
    rs = np.random.RandomState(9)
    comp = {"G": "C", "C": "G"}
    seq = ""
    while len(seq) < 1300:
        stem = "".join(rs.choice(list("GC"), 10))
        seq += stem + "AAAA" + "".join(comp[x] for x in reversed(stem)) + "AA"
    seq = seq[:1300]
    bp, fup, z = v1.fold(seq)
    assert z - 0.28 * len(seq) > np.log(1e280) + 50.0
    band, up, logz = v1.span_fold(seq, len(seq))
    assert_log_close([logz], [z], what="log Z of the chain")
    assert_prob_close(band, sc.tri_to_band(bp, len(seq), len(seq)), what="band of the chain")
    assert_prob_close(up[:, 0], np.asarray(fup).reshape(len(seq), -1)[:, 0], what="up of the chain")
    bp1, _, z1 = v1.fold(seq)
    assert (bp1 == bp).all() and z1 == z


# ---- interface
def test_the_layout_after_a_span_fold(vctx):
    vctx.span_fold(sc.random_seq(90), 33)
    n, ld, nw, w = (ctypes.c_int() for _ in range(4))
    byref = ctypes.byref
    starts = np.full(1, -1, dtype=np.int32)
    L = vctx.L
    assert L.rh_local_layout(vctx.h, byref(n), byref(ld), byref(nw), byref(w), starts.ctypes.data) == 0
    assert (n.value, ld.value, nw.value, w.value, starts[0]) == (90, 33, 1, 1, 0)
    vctx.span_fold(sc.random_seq(40), 70)
    assert L.rh_local_layout(vctx.h, byref(n), byref(ld), byref(nw), byref(w), None) == 0
    assert (n.value, ld.value, nw.value, w.value) == (40, 40, 1, 1)
    ms = vctx.span_times()
    assert ms[0] > 0.0 and ms[1] > 0.0


def test_candidates_against_a_numpy_threshold(v1):
    band, up, _ = v1.span_fold(sc.random_seq(300), 60)
    for th in (0.5, 0.01):
        rec, total = v1.local_candidates(0, th)
        i, d = np.nonzero(band.astype(np.float32) > np.float32(th))
        assert total == len(i) > 0
        assert (rec["i"] == i + 1).all() and (rec["j"] == i + 1 + d).all()
        assert (rec["p"] == band[i, d].astype(np.float32)).all()
    rec, total = v1.local_candidates(1, 0.9)
    i = np.nonzero(up[:, 0].astype(np.float32) > np.float32(0.9))[0]
    assert total == len(i) > 0 and (rec["i"] == i).all() and (rec["j"] == 0).all()
    assert (rec["p"] == up[i, 0].astype(np.float32)).all()


def test_a_span_fold_drops_the_hp_of_a_local_duplex_and_keeps_hp_loc2(v1):
    q, t = sc.random_seq(12, seed=1), sc.random_seq(60, seed=2)
    hp2 = v1.local_duplex2(q, t, 12, 1, 30, 10)
    v1.local_duplex(q, t, 30, 10)
    v1.local_hp_results()
    v1.span_fold(t, 20)
    with pytest.raises(ractip_amd.RhError, match="no local hybridization result"):
        v1.local_hp_results()
    again = v1.local_hp2_results()
    assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(hp2[:2], again[:2]))


def test_a_refused_call_keeps_the_previous_result(v1):
    seq = sc.random_seq(90)
    first = v1.span_fold(seq, 33)
    for bad_seq, L, text in ((seq, 1, "max_span 1"), ("", 33, "length 0")):
        with pytest.raises(ractip_amd.RhError, match=text):
            v1.span_fold(bad_seq, L)
        assert v1.L.rh_span_fold(v1.h, bad_seq.encode(), len(bad_seq), L) == RH_ERR_ARG
    assert v1.L.rh_span_fold(v1.h, None, 5, 5) == RH_ERR_ARG
    band, up, logz, starts = v1.local_results()
    assert (band == first[0]).all() and (up == first[1]).all() and logz[0] == first[2] and list(starts) == [0]


def test_refused_where_there_are_no_kernels(ctx, v1):
    """CONTRAfold contexts (the `ctx` fixture, either path), Vienna-BL contexts in RH_MODE_LOG and 2.x semantics: RH_ERR_UNSUPPORTED,
    and a previous local result stays"""
    seq = sc.random_seq(40)
    kept = ctx.local_fold(seq, 16, 5)
    assert ctx.L.rh_span_fold(ctx.h, seq.encode(), len(seq), 20) == RH_ERR_UNSUPPORTED
    with pytest.raises(ractip_amd.RhError, match="CONTRAfold"):
        ctx.span_fold(seq, 20)
    assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(kept, ctx.local_results()))
    first = v1.span_fold(seq, 20)
    v1.set_mode(hot.RH_MODE_LOG)
    try:
        with pytest.raises(ractip_amd.RhError, match="log-space"):
            v1.span_fold(seq, 20)
        assert v1.L.rh_span_fold(v1.h, seq.encode(), len(seq), 20) == RH_ERR_UNSUPPORTED
    finally:
        v1.set_mode(hot.RH_MODE_AUTO)
    assert (v1.local_results()[0] == first[0]).all()
    c2 = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL, vienna=dict(semantics=2))
    try:
        with pytest.raises(ractip_amd.RhError, match="2.x"):
            c2.span_fold(seq, 20)
    finally:
        c2.close()


def test_reuse_gives_the_same_bits_and_leaves_the_batch(v1):
    a, b = sc.random_seq(130), sc.random_seq(90, seed=4)
    bp0, up0, z0 = v1.fold(a)
    first = v1.span_fold(a, 64)
    other = v1.span_fold(b, 31)
    check(other, sc.masked(b, 31), "second sequence")
    again = v1.span_fold(a, 64)
    assert (again[0] == first[0]).all() and (again[1] == first[1]).all() and again[2] == first[2]
    bp1, up1, z1 = v1.fold(a)
    assert (bp0 == bp1).all() and (np.asarray(up0) == np.asarray(up1)).all() and z0 == z1


def test_the_pipeline_and_the_command_line(v1, tmp_path):
    seq = sc.random_seq(90)
    ref = sc.masked(seq, 33)
    r = pipeline.span_fold(seq, 33, ctx=v1)
    check((r["bp_band"], r["up"], r["logZ"]), ref, "pipeline.span_fold")
    assert r["max_span"] == 33 and r["n"] == 90
    own = pipeline.span_fold(seq, 33)
    assert (own["bp_band"] == r["bp_band"]).all() and own["logZ"] == r["logZ"]
    fa = tmp_path / "one.fa"
    fa.write_text(">one\n%s\n%s\n" % (seq[:50], seq[50:]))
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "ractip_amd.pipeline", str(fa), "--max-span", "33", "--threshold", "0.3"], capture_output=True,
                         text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0].split()[:2] == [">one", "logZ"] and abs(float(lines[0].split()[2]) - ref["logZ"]) <= 1e-6
    i, d = np.nonzero(ref["band"].astype(np.float32) > np.float32(0.3))
    assert [tuple(int(x) for x in ln.split()[:2]) for ln in lines[1:]] == [(a + 1, a + 1 + b) for a, b in zip(i, d)]
