"""GPU suite: region accessibility up[i][w] of span folds under the CONTRAfold model (kernels in
ractip_amd/csrc/mccaskill_span_cf_acc.hip): a CONTRAfold context with set_span_contrafold(True) AND set_region_accessibility(True)
answers span_fold / span_fold_batch at max_w 1..64.

The yardstick is tests/_cf_span_acc_ref.py: up_ref = exp(logZ(band and region masked) - logZ(band)) from two runs of the masked
restatement, at the project's assert_prob_close (rel 1e-6 above 1e-12); tests/test_cf_span_acc_cpu.py pins the yardstick and that
every reference used here lies above 1e-9.  Shapes: every region of short sequences at 15 widths; no pair possible; the planted
multiloop with the closing pair on both sides of the band edge (the derivation count of the chain); the loop budget of 30; the
hairpin of forty; the kernels' edges with sampled regions; L >= n against the whole fold; invariants, the ladder, batches and the
interface.  Every context here is the module's own."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot, pipeline
import _cf_span_acc_ref as acc
import _contrafold_weights as cw
import _span_cases as sc
from _oracle import assert_log_close, assert_prob_close
from _cf_span_acc_cases import (EDGE_CASES, EVERY_CASES, FORTY_L, MULTILOOP_L, SCRAMBLED_CASES, SIDE_CASES, case_entries, case_seq)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RH_OK, RH_ERR_UNSUPPORTED = 0, -5
LENGTHS = [257, 1, 300, 3, 13, 129, 64, 65]
RAGGED = [sc.random_seq(n, seed=k) for k, n in enumerate(LENGTHS)]


def make(param_file=None, widths=True):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_CONTRAFOLD, param_file=param_file)
    c.set_span_contrafold(True)
    if widths:
        c.set_region_accessibility(True)
    return c


@pytest.fixture(scope="module")
def cf(hotlib):
    c = make()
    yield c
    c.close()


@pytest.fixture(scope="module")
def whole(hotlib):
    """a second context for Context.fold with the widths on"""
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_CONTRAFOLD)
    c.set_region_accessibility(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scrambled(hotlib, tmp_path_factory):
    path = cw.write(tmp_path_factory.mktemp("spancfacc") / "scrambled.params", cw.scrambled())
    c = make(path)
    yield c, path
    c.close()


def check(c, seq, L, max_w, entries, params=None, what=""):
    band, up, logz = c.span_fold(seq, L, max_w)
    n = len(seq)
    assert up.shape == (n, max_w), what
    got = np.array([up[i, w] for i, w in entries])
    want = acc.up_ref(seq, L, entries, params)
    print("%s n=%d L=%d max_w=%d: %d entries, reference min %.3g, max rel err %.3g" % (
        what, n, L, max_w, len(entries), want.min() if len(want) else 1.0, np.max(np.abs(got - want) / want) if len(want) else 0.0))
    assert_prob_close(got, want, what="%s n=%d L=%d max_w=%d" % (what, n, L, max_w))
    assert all(up[i, w] == 0.0 for i, w in acc.past_the_end(n, max_w)), what + ": entries past the end hold 0"
    return up


def equal(a, b):
    return a[0].shape == b[0].shape and a[1].shape == b[1].shape and (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]


def err(c):
    return c.L.rh_last_error(c.h).decode()


# ---- parity with the yardstick
@pytest.mark.parametrize("case", EVERY_CASES, ids=str)
def test_every_region_at_fifteen_widths(cf, case):
    seq = case_seq(case)
    check(cf, seq, case[2], case[3], case_entries(case), what="every region")


@pytest.mark.parametrize("L", [2, 4])
def test_no_pair_is_possible(cf, L):
    _, up, _ = cf.span_fold(sc.random_seq(40), L, 15)
    for i, w in acc.every(40, 15):
        assert abs(up[i, w] - 1.0) <= 1e-12
    assert all(up[i, w] == 0.0 for i, w in acc.past_the_end(40, 15))


@pytest.mark.parametrize("L", MULTILOOP_L)
def test_the_planted_multiloop_at_the_band_edge(cf, L):
    """the closing pair (1, 85) is in the band at L = 86 and 85 and not below: the chain must count the derivations of the band"""
    seq, trail = acc.planted_multiloop(3)
    assert len(seq) == 85
    up = check(cf, seq, L, 15, acc.multiloop_entries(seq, trail), what="multiloop")
    run = up[trail[0], 5]
    want = {86: 0.6976, 85: 0.6976, 84: 0.2934, 83: 0.2934, 40: 0.1472}[L]
    assert abs(run - want) < 5e-4, "the six trailing letters at L = %d" % L


def test_the_drop_across_the_band_edge(cf):
    seq, trail = acc.planted_multiloop(3)
    inside = cf.span_fold(seq, 85, 15)[1][trail[0], 5]
    outside = cf.span_fold(seq, 84, 15)[1][trail[0], 5]
    assert inside > 0.69 and outside < 0.30, "a chain that ignores the band keeps the closing pair's multiloop"


def test_four_branches_at_the_whole_length(cf):
    seq, trail = acc.planted_multiloop(4)
    check(cf, seq, len(seq), 15, acc.multiloop_entries(seq, trail), what="multiloop 4")


@pytest.mark.parametrize("case", SIDE_CASES, ids=str)
def test_planted_interior_sides_at_the_loop_budget(cf, case):
    seq = case_seq(case)
    check(cf, seq, case[2], case[3], case_entries(case), what="interior side")


@pytest.mark.parametrize("L", FORTY_L)
def test_the_hairpin_of_forty(cf, L):
    """56 letters; the stem pair (4, 53) spans 49 letters: in the band at L = 50, not at L = 49"""
    seq = acc.hairpin_of_forty()
    assert len(seq) == 56
    check(cf, seq, L, 15, case_entries(("forty", 56, L, 15)), what="hairpin 40")


@pytest.mark.parametrize("case", EDGE_CASES, ids=str)
def test_kernel_edges_with_sampled_regions(cf, case):
    seq = case_seq(case)
    check(cf, seq, case[2], case[3], case_entries(case), what="edge")


@pytest.mark.parametrize("case", SCRAMBLED_CASES, ids=str)
def test_a_subset_under_the_scrambled_weights(scrambled, case):
    c, path = scrambled
    seq = case_seq(case)
    check(c, seq, case[2], case[3], case_entries(case), params=path, what="scrambled")


@pytest.mark.parametrize("n", [130, 300])
def test_span_at_least_the_length_is_the_whole_fold(cf, whole, n):
    seq = sc.random_seq(n)
    _, up, _ = cf.span_fold(seq, n + 5, 15)
    whole.set_max_w(15)
    _, fup, _ = whole.fold(seq)
    assert_prob_close(up, np.asarray(fup).reshape(n, 15), what="every region against Context.fold, n = %d" % n)


# ---- invariants
def test_invariants(cf):
    a, b = sc.random_seq(130), sc.random_seq(90)
    one = cf.span_fold(a, 33, 1)
    wide = cf.span_fold(a, 33, 15)
    assert (wide[0] == one[0]).all() and wide[2] == one[2], "band and log Z have the bits of the max_w = 1 call"
    assert (wide[1][:, 0] == one[1][:, 0]).all(), "column 0 has the bits of the width-1 up"
    assert (np.diff(wide[1], axis=1) <= 1e-12).all(), "rows do not increase with the width"
    assert wide[1].min() >= 0.0 and wide[1].max() <= 1.0
    cf.span_fold(b, 20, 15)
    assert equal(cf.span_fold(a, 33, 15), wide), "A, B, A gives A's bits"
    ms = cf.span_acc_times()
    assert len(ms) == 3 and all(t > 0.0 for t in ms)


def hairpin_chain(n):
    """the chain of stable hairpins of tests/test_gpu_span_cf.py"""
    rs = np.random.RandomState(9)
    comp = {"G": "C", "C": "G"}
    seq = ""
    while len(seq) < n:
        stem = "".join(rs.choice(list("GC"), 10))
        seq += stem + "AAAA" + "".join(comp[x] for x in reversed(stem)) + "AA"
    return seq[:n]


def test_the_ladder_holds_the_widths(cf, whole):
    """1560 letters of GC hairpins at L = n: the first attempt is flagged (tests/test_gpu_span_cf.py) and a larger exponent answers;
    up must not depend on the exponent that held.  Reference: Context.fold with the widths on, which takes its own ladder."""
    seq = hairpin_chain(1560)
    n = len(seq)
    whole.set_max_w(5)
    _, fup, z = whole.fold(seq)
    assert z - 0.12 * n > np.log(1e280) + 50.0
    _, up, logz = cf.span_fold(seq, n, 5)
    assert_log_close([logz], [z], what="log Z of the chain")
    assert_prob_close(up, np.asarray(fup).reshape(n, 5), what="up of the chain")


# ---- batches
def item_bytes(n, L, max_w):
    ldn = -(-(n + 1) // 16) * 16
    tables = 11 if max_w == 1 else 15
    return (tables * min(n, L) * ldn + (64 * ldn if max_w > 1 else 0)) * 8


def test_a_ragged_batch_equals_the_single_calls_under_any_chunking(cf):
    L, W = 33, 15
    singles = [cf.span_fold(seq, L, W) for seq in RAGGED]
    sizes = [item_bytes(n, L, W) for n in LENGTHS]
    try:
        all_in_one = cf.span_fold_batch(RAGGED, L, W)
        cf.set_span_batch_bytes(max(sizes))
        some = cf.span_fold_batch(RAGGED, L, W)
        cf.set_span_batch_bytes(1)
        each = cf.span_fold_batch(RAGGED, L, W)
    finally:
        cf.set_span_batch_bytes(0)
    for k, seq in enumerate(RAGGED):
        assert all_in_one[k][1].shape == (len(seq), W)
        assert equal(all_in_one[k], singles[k]) and equal(some[k], singles[k]) and equal(each[k], singles[k]), "item %d (n = %d)" % (k, len(seq))
    # rh_span_batch_results and the candidates of up
    got = cf.span_fold_batch(RAGGED, L, W)
    assert equal(cf.span_batch_results(2), singles[2])
    up = singles[2][1]
    rec, total = cf.span_batch_candidates(2, 1, 0.5)
    i, w = np.nonzero(up.astype(np.float32) > np.float32(0.5))
    assert total == len(i) > 0 and (rec["i"] == i).all() and (rec["j"] == w).all() and (rec["p"] == up[i, w].astype(np.float32)).all()
    assert len(got) == len(RAGGED)


# ---- interface
def test_the_switches(hotlib):
    seq = sc.random_seq(90)
    enc = seq.encode()
    c = make(widths=False)
    try:
        kept = c.span_fold(seq, 33)
        assert c.L.rh_span_fold_acc(c.h, enc, len(seq), 33, 2) == RH_ERR_UNSUPPORTED and "region accessibility" in err(c)
        band, up, logz, starts = c.local_results()
        assert (band == kept[0]).all() and (up == kept[1]).all() and logz[0] == kept[2], "the local result is kept"
        c.set_region_accessibility(True)
        assert c.L.rh_span_fold_acc(c.h, enc, len(seq), 33, 2) == RH_OK
        assert c.L.rh_span_fold_constrained(c.h, enc, len(seq), None, 33, 15) == RH_OK
        assert c.L.rh_span_fold_constrained(c.h, enc, len(seq), b"." * len(seq), 33, 15) == RH_ERR_UNSUPPORTED and "constraint" in err(c)
        assert c.max_w == 1, "the context's own max_w is not touched by a span call"
        c.set_mode(hot.RH_MODE_LOG)
        try:
            assert c.L.rh_span_fold_acc(c.h, enc, len(seq), 33, 15) == RH_ERR_UNSUPPORTED and "log-space" in err(c)
        finally:
            c.set_mode(hot.RH_MODE_AUTO)
    finally:
        c.close()


def test_the_pipeline_span_fold(cf):
    seq = sc.random_seq(90)
    want = cf.span_fold(seq, 33, 15)
    r = pipeline.span_fold(seq, 33, max_w=15, model="contrafold")
    assert equal((r["bp_band"], r["up"], r["logZ"]), want)
    rb = pipeline.span_fold_batch([seq, sc.random_seq(47)], 33, max_w=15, model="contrafold")
    assert equal((rb[0]["bp_band"], rb[0]["up"], rb[0]["logZ"]), want)


def test_predict_on_span_folds_and_the_command_line(hotlib, tmp_path):
    rng = np.random.default_rng(11)
    s1 = "".join("ACGU"[k] for k in rng.integers(0, 4, 40))
    s2 = "".join("ACGU"[k] for k in rng.integers(0, 4, 35))
    want = pipeline.predict(s1, s2, model="contrafold", accessibility=True)
    got = pipeline.predict(s1, s2, model="contrafold", max_span=45, accessibility=True)
    assert tuple(got[:2]) == tuple(want[:2])
    with pytest.raises(ValueError):
        pipeline.predict(s1, s2, model="contrafold", max_span=45)
    # hp from the window averages: one window that holds either molecule is the pair path's hp
    for how in (dict(local_hp=True), dict(local_hp_both=True)):
        got = pipeline.predict(s1, s2, model="contrafold", max_span=45, accessibility=True, window=45, **how)
        assert tuple(got[:2]) == tuple(want[:2]), how
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_text(">a\n%s\n" % s1)
    b.write_text(">b\n%s\n" % s2)
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "ractip_amd.pipeline", str(a), str(b), "--contrafold", "--accessibility", "--max-span", "45"],
                         capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert want[0] in out.stdout and want[1] in out.stdout
