"""GPU suite: region accessibility on span folds (rh_span_fold_acc) -- up[i][w] = P(letters i .. i + w unpaired) in the ensemble of
rh_span_fold, every column the sum of its exterior, hairpin, one-enclosed-pair and multiloop parts on the band tables -- against
the CPU oracle under the band mask at the same widths (tests/_span_acc_cases.py; pinned against the enumeration by
tests/test_span_acc_cpu.py): band and up at rel 1e-6 above 1e-12, log Z at 1e-9.

Shapes (n, L, max_w) on random ACGU with one N planted from 8 letters on: n below max_w, where rows longer than the sequence hold 0;
no pair possible (L = 2, 4: exactly 1 where the run fits, 0 past the end) and the first possible pair (L = 5); widths 29..33 across
the interior-loop budget of 30 and the band edge (L = 31..34); widths at and above L - 2, which no hairpin holds (L = 20, 24
widths); the wavefront edge of the multiloop rows (L = 63..65); the exterior blocks of 64 entries; two workgroup columns; unpadded
table rows (n = 47); a general case; L >= n at 64 widths, also against Context.fold at max_w 64.  Then identities between the
widths, and the interface."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot, pipeline
import _span_acc_cases as ac
import _span_cases as sc
from _oracle import assert_log_close, assert_prob_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RH_ERR_ARG, RH_ERR_UNSUPPORTED = -1, -5
SHAPES = [(1, 2, 5), (2, 2, 5), (10, 70, 64), (40, 2, 5), (40, 4, 5), (40, 5, 5), (90, 31, 33), (90, 32, 33), (90, 33, 33), (90, 34, 33),
          (90, 20, 24), (130, 63, 15), (130, 64, 15), (130, 65, 15), (64, 70, 15), (65, 70, 15), (66, 70, 15), (128, 40, 15), (129, 40, 15),
          (256, 20, 5), (257, 20, 5), (258, 20, 5), (47, 20, 15), (300, 60, 15), (70, 70, 64), (70, 500, 64)]


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
    n, mw = up.shape
    i, w = np.arange(n)[:, None], np.arange(mw)[None, :]
    assert not up[i + w >= n].any(), what + ": a run that passes the last letter holds 0"
    assert (up <= 1.0).all() and (np.diff(up, axis=1) <= 1e-12).all(), what + ": no row grows with the width"


# ---- parity
@pytest.mark.parametrize("n,L,max_w", SHAPES)
def test_parity_with_the_masked_oracle(v1, n, L, max_w):
    seq = sc.random_seq(n)
    assert ("N" in seq) == (n >= 8)
    check(v1.span_fold(seq, L, max_w), ac.masked_acc(seq, L, max_w), "n=%d L=%d max_w=%d" % (n, L, max_w))


@pytest.mark.parametrize("L", [2, 4])
def test_no_pair_is_possible(v1, L):
    band, up, logz = v1.span_fold(sc.random_seq(40), L, 5)
    i, w = np.arange(40)[:, None], np.arange(5)[None, :]
    assert not band.any() and logz == 0.0
    assert (up[i + w < 40] == 1.0).all() and (up[i + w >= 40] == 0.0).all()


def test_widths_no_hairpin_can_hold_are_exterior_only(v1):
    """L = 20: a run of L - 2 letters and more fits in no loop, so it is unpaired in the exterior or not at all"""
    seq = sc.random_seq(90)
    band, up, logz = v1.span_fold(seq, 20, 24)
    ref = ac.masked_acc(seq, 20, 24)["up"]
    assert_prob_close(up[:, 18:], ref[:, 18:], what="widths 19..24")
    assert (ref[:60, 18:] > 0.0).all()


@pytest.mark.parametrize("L", [70, 500])
def test_span_at_least_the_length_is_the_whole_fold(hotlib, v1, L):
    seq = sc.random_seq(70)
    band, up, logz = v1.span_fold(seq, L, 64)
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    try:
        c.set_max_w(64)
        bp, fup, z = c.fold(seq)
    finally:
        c.close()
    assert_log_close([logz], [z], what="log Z against Context.fold")
    assert_prob_close(band, sc.tri_to_band(bp, 70, 70), what="band against Context.fold")
    assert_prob_close(up, np.asarray(fup).reshape(70, 64), what="up against Context.fold")


# ---- identities
@pytest.mark.parametrize("n,L,max_w", [(90, 33, 33), (130, 64, 15), (300, 60, 15), (257, 20, 5), (70, 70, 64)])
def test_identities_between_the_widths(v1, n, L, max_w):
    seq = sc.random_seq(n)
    band1, up1, z1 = v1.span_fold(seq, L)
    one = v1.span_fold(seq, L, 1)
    assert up1.shape == (n, 1)
    assert (one[0] == band1).all() and (one[1] == up1).all() and one[2] == z1, "max_w = 1 has the bits of rh_span_fold"
    band, up, z = v1.span_fold(seq, L, max_w)
    assert (band == band1).all() and z == z1, "band and log Z have the bits of rh_span_fold"
    assert_prob_close(up[:, 0], up1[:, 0], what="column 0 (the four parts) against 1 - the row sums")
    assert (np.diff(up, axis=1) <= 1e-12).all()
    again = v1.L.rh_span_fold(v1.h, seq.encode(), n, L)
    assert again == 0 and (v1.local_results()[1] == up1).all(), "rh_span_fold keeps width 1"


# ---- interface
def test_the_layout_reports_the_width_asked_for(v1):
    n, ld, nw, w = (ctypes.c_int() for _ in range(4))
    byref = ctypes.byref
    starts = np.full(1, -1, dtype=np.int32)
    v1.set_max_w(7)
    try:
        for seq, L, max_w, want in ((sc.random_seq(90), 33, 15, (90, 33, 1, 15, 0)), (sc.random_seq(40), 70, 3, (40, 40, 1, 3, 0)),
                                    (sc.random_seq(40), 70, 1, (40, 40, 1, 1, 0))):
            assert v1.L.rh_span_fold_acc(v1.h, seq.encode(), len(seq), L, max_w) == 0
            assert v1.L.rh_local_layout(v1.h, byref(n), byref(ld), byref(nw), byref(w), starts.ctypes.data) == 0
            assert (n.value, ld.value, nw.value, w.value, starts[0]) == want
        assert v1.max_w == 7
    finally:
        v1.set_max_w(1)


def test_the_stage_times(v1):
    v1.span_fold(sc.random_seq(300), 60, 15)
    ms = v1.span_acc_times()
    assert len(ms) == 3 and all(x > 0.0 for x in ms)
    sweeps = v1.span_times()
    assert sweeps[0] > 0.0 and sweeps[1] > 0.0
    v1.span_fold(sc.random_seq(300), 60)
    with pytest.raises(ractip_amd.RhError, match="widths above one"):
        v1.span_acc_times()


def test_candidates_against_a_numpy_threshold(v1):
    band, up, _ = v1.span_fold(sc.random_seq(300), 60, 15)
    for th in (0.9, 0.2):
        rec, total = v1.local_candidates(1, th)
        i, w = np.nonzero(up.astype(np.float32) > np.float32(th))
        assert total == len(i) > 0 and (w > 0).any()
        assert (rec["i"] == i).all() and (rec["j"] == w).all()
        assert (rec["p"] == up[i, w].astype(np.float32)).all()
    rec, total = v1.local_candidates(0, 0.5)
    i, d = np.nonzero(band.astype(np.float32) > np.float32(0.5))
    assert total == len(i) > 0 and (rec["i"] == i + 1).all() and (rec["j"] == i + 1 + d).all()


def test_a_refused_call_keeps_the_previous_result(v1):
    seq = sc.random_seq(90)
    first = v1.span_fold(seq, 33, 5)
    for bad_seq, L, max_w, text in ((seq, 33, 0, "max_w 0"), (seq, 33, 65, "max_w 65"), (seq, 33, -3, "max_w -3"), (seq, 1, 5, "max_span 1"),
                                    ("", 33, 5, "length 0")):
        with pytest.raises(ractip_amd.RhError, match=text):
            v1.span_fold(bad_seq, L, max_w)
        assert v1.L.rh_span_fold_acc(v1.h, bad_seq.encode(), len(bad_seq), L, max_w) == RH_ERR_ARG
    assert v1.L.rh_span_fold_acc(v1.h, None, 5, 5, 5) == RH_ERR_ARG
    band, up, logz, starts = v1.local_results()
    assert up.shape == (90, 5)
    assert (band == first[0]).all() and (up == first[1]).all() and logz[0] == first[2] and list(starts) == [0]


def test_refused_where_there_are_no_kernels(ctx, v1):
    seq = sc.random_seq(40)
    assert ctx.L.rh_span_fold_acc(ctx.h, seq.encode(), len(seq), 20, 5) == RH_ERR_UNSUPPORTED
    with pytest.raises(ractip_amd.RhError, match="CONTRAfold"):
        ctx.span_fold(seq, 20, 5)
    first = v1.span_fold(seq, 20, 5)
    v1.set_mode(hot.RH_MODE_LOG)
    try:
        with pytest.raises(ractip_amd.RhError, match="log-space"):
            v1.span_fold(seq, 20, 5)
    finally:
        v1.set_mode(hot.RH_MODE_AUTO)
    assert (v1.local_results()[1] == first[1]).all()


def test_the_context_keeps_its_max_w_and_its_batch(hotlib):
    a = sc.random_seq(130)
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    try:
        c.set_max_w(5)
        bp0, up0, z0 = c.fold(a)
        got = c.span_fold(a, 64, 15)
        assert got[1].shape == (130, 15) and c.max_w == 5
        bp1, up1, z1 = c.fold(a)
        assert np.asarray(up1).shape == (130, 5)
        assert (bp0 == bp1).all() and (np.asarray(up0) == np.asarray(up1)).all() and z0 == z1
    finally:
        c.close()


def test_reuse_gives_the_same_bits(v1):
    a, b = sc.random_seq(130), sc.random_seq(90, seed=4)
    first = v1.span_fold(a, 64, 15)
    other = v1.span_fold(b, 31, 33)
    check(other, ac.masked_acc(b, 31, 33), "second sequence")
    again = v1.span_fold(a, 64, 15)
    assert (again[0] == first[0]).all() and (again[1] == first[1]).all() and again[2] == first[2]


def test_the_exponent_ladder_takes_over_where_the_band_overflows(v1):
    """The 1300-letter chain of stable hairpins of tests/test_gpu_span_fold.py at L = n: the first attempt is flagged, the call
    answers from a larger exponent of the ladder, and the accessibility stage runs on that attempt's model: the values are those of
    the whole fold at max_w 5."""
    rs = np.random.RandomState(9)
    comp = {"G": "C", "C": "G"}
    seq = ""
    while len(seq) < 1300:
        stem = "".join(rs.choice(list("GC"), 10))
        seq += stem + "AAAA" + "".join(comp[x] for x in reversed(stem)) + "AA"
    seq = seq[:1300]
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    try:
        c.set_max_w(5)
        bp, fup, z = c.fold(seq)
    finally:
        c.close()
    assert z - 0.28 * len(seq) > np.log(1e280) + 50.0
    band, up, logz = v1.span_fold(seq, len(seq), 5)
    assert_log_close([logz], [z], what="log Z of the chain")
    assert_prob_close(up, np.asarray(fup).reshape(len(seq), 5), what="up of the chain")
    assert_prob_close(band, sc.tri_to_band(bp, len(seq), len(seq)), what="band of the chain")


# ---- pipeline
def test_the_pipeline_span_fold(v1):
    seq = sc.random_seq(90)
    r = pipeline.span_fold(seq, 33, max_w=5, ctx=v1)
    check((r["bp_band"], r["up"], r["logZ"]), ac.masked_acc(seq, 33, 5), "pipeline.span_fold")
    assert r["max_span"] == 33 and r["n"] == 90
    own = pipeline.span_fold(seq, 33, max_w=5)
    assert (own["up"] == r["up"]).all() and own["logZ"] == r["logZ"]


def oxys_fhla():
    fa = [l.strip() for l in open(os.path.join(ROOT, "ractip_amd", "data", "config5_OxyS_fhlA.fa")) if not l.startswith(">")]
    return fa[0], fa[1]


def test_predict_with_a_span_no_smaller_than_the_molecules(hotlib):
    s1, s2 = oxys_fhla()
    L = max(len(s1), len(s2))
    whole = pipeline.predict(s1, s2)
    span = pipeline.predict(s1, s2, max_span=L)
    assert span[0] == whole[0] and span[1] == whole[1]
    assert set(whole[0]) > {"."} or set(whole[1]) > {"."}      # (a prediction with structure in it)
    local = pipeline.predict(s1, s2, max_span=L, window=L, step=10, local_hp_both=True)
    assert local[0] == whole[0] and local[1] == whole[1]


def test_the_two_file_command_line(hotlib, tmp_path):
    s1, s2 = oxys_fhla()
    L = max(len(s1), len(s2))
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_text(">OxyS\n%s\n" % s1)
    b.write_text(">fhlA\n%s\n" % s2)
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "ractip_amd.pipeline", str(a), str(b), "--max-span", str(L)], capture_output=True, text=True,
                         env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    r1, r2, _ = pipeline.predict(s1, s2)
    assert out.stdout == ">OxyS\n%s\n%s\n>fhlA\n%s\n%s\n" % (s1, r1, s2, r2)


def test_what_predict_refuses_with_a_span():
    with pytest.raises(ValueError, match="Vienna-BL"):
        pipeline.predict("GGGAAACCC", "GGGAAACCC", model="contrafold", max_span=5)
    with pytest.raises(ValueError, match="structure constraints"):
        pipeline.predict("GGGAAACCC", "GGGAAACCC", structures=("." * 9, "." * 9), max_span=5)
    with pytest.raises(ValueError, match="local_hp"):
        pipeline.predict("GGGAAACCC", "GGGAAACCC", window=5, max_span=5)
