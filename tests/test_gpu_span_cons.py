"""GPU suite: span folds under structure constraints (rh_span_fold_constrained, rh_span_fold_batch_constrained).  The reference is
the CPU oracle under band_mask(n, L) & constraint_mask(cons, n) (tests/_span_cons_cases.py; tests/test_span_cons_cpu.py checks
that every case is moved by its constraint).  Tolerances: rel 1e-6 on band and up above a floor of 1e-12, 1e-9 on log Z, rel 1e-9
against Context.fold; "equal" is == on every array and on log Z.

  1  single constrained calls against the oracle at L = 2, 20, 60 and L >= n, max_w 1 and 15
  2  L >= n: the ensemble of Context.fold(seq, constraint)
  3  a NULL constraint and one that restricts nothing equal span_fold
  4  a ragged batch that mixes constrained and NULL items equals the single calls, and matches the oracle directly
  5  chunk budgets that give one chunk, or one item per chunk, change no bit
  6  refusals leave the previous local result and the previous batch result in place
  7  candidates of a constrained item are those of the single call
  8  pipeline.span_fold(structure=), span_fold_batch(structures=) and the command line in a child process, with '[', ']' and 'e'
     in the structure line"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot, pipeline
import _span_cases as sc
import _span_cons_cases as cc
from _oracle import assert_log_close, assert_prob_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RH_OK, RH_ERR_ARG, RH_ERR_UNSUPPORTED = 0, -1, -5
LENGTHS = [257, 1, 300, 2, 13, 129, 63, 64, 65, 128]      # those of tests/test_gpu_span_batch.py
BATCH_L = 20
FREE = (1, 5, 8)                                          # items of the ragged batch without a constraint (NULL)


@pytest.fixture(scope="module")
def v1(hotlib):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    yield c
    c.close()


def equal(a, b):
    return a[0].shape == b[0].shape and a[1].shape == b[1].shape and (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]


def ragged(L=BATCH_L):
    """(sequences, constraints) of the ragged batch: a constraint per item, None for the items of FREE"""
    items = [cc.case(n, L, seed=k) for k, n in enumerate(LENGTHS)]
    return [s for s, _ in items], [None if k in FREE else t for k, (_, t) in enumerate(items)]


def close(got, ref, what):
    band, up, logz = got
    assert band.shape == ref["band"].shape and up.shape == ref["up"].shape, what
    assert_log_close([logz], [ref["logZ"]], what=what + " log Z")
    assert_prob_close(band, ref["band"], what=what + " band")
    assert_prob_close(up, ref["up"], what=what + " up")


def item_bytes(n, L, max_w):
    Le, ldn = min(n, L), -(-(n + 1) // 16) * 16
    return 13 * Le * ldn * 8 + (2 * 32 * ldn * 8 if max_w > 1 else 0)


# ---- 1
@pytest.mark.parametrize("max_w", cc.MAX_W)
@pytest.mark.parametrize("n,L", cc.SINGLE)
def test_single_calls_against_the_masked_oracle(v1, n, L, max_w):
    seq, cons = cc.case(n, L)
    close(v1.span_fold(seq, L, max_w, cons), cc.masked_cons(seq, L, cons, max_w), "n=%d L=%d max_w=%d" % (n, L, max_w))


@pytest.mark.parametrize("k", range(len(cc.SHORT)))
def test_the_short_cases_against_the_enumeration(v1, k):
    seq, cons, L = cc.SHORT[k]
    close(v1.span_fold(seq, L, 4, cons), cc.masked_cons(seq, L, cons, 4, bruteforce=True), "short case %d" % k)


# ---- 2
@pytest.mark.parametrize("L", [70, 100])
def test_a_span_that_covers_the_sequence_is_the_constrained_fold(v1, L):
    seq, cons = cc.case(70, L)
    band, up, logz = v1.span_fold(seq, L, 1, cons)
    tri, fup, z = v1.fold(seq, cons)
    assert band.shape == (70, 70)
    assert_log_close([logz], [z], what="log Z against Context.fold")
    assert_prob_close(band, sc.tri_to_band(tri, 70, 70), rel=1e-9, what="band against Context.fold")
    assert_prob_close(up[:, 0], np.asarray(fup).reshape(70, -1)[:, 0], rel=1e-9, what="up against Context.fold")


# ---- 3
@pytest.mark.parametrize("L,max_w", [(20, 1), (60, 15)])
def test_a_constraint_that_restricts_nothing_is_span_fold(v1, L, max_w):
    seq = sc.random_seq(300)
    plain = v1.span_fold(seq, L, max_w)
    assert v1.L.rh_span_fold_constrained(v1.h, seq.encode(), len(seq), None, L, max_w) == RH_OK
    band, up, logz, _ = v1.local_results()
    assert equal((band, up, float(logz[0])), plain), "a NULL constraint"
    for cons in ("." * 300, "", "..", "." * 400, "..|.." * 60):
        assert equal(v1.span_fold(seq, L, max_w, cons), plain), repr(cons[:8])
    batch = v1.span_fold_batch([seq, seq[:129], seq], L, max_w, ["." * 300, None, ""])
    assert equal(batch[0], plain) and equal(batch[2], plain) and equal(batch[1], v1.span_fold(seq[:129], L, max_w))
    seq2, cons2 = cc.case(300, L)
    assert not equal(v1.span_fold(seq2, L, max_w, cons2), v1.span_fold(seq2, L, max_w)), "a constraint that restricts changes the result"


# ---- 4
@pytest.mark.parametrize("L,max_w", [(BATCH_L, 1), (BATCH_L, 15), (2, 1), (400, 5)])
def test_a_ragged_mixed_batch_equals_the_single_calls_and_the_oracle(v1, L, max_w):
    seqs, cons = ragged(L)
    assert sum(c is None for c in cons) == len(FREE) and any(c for c in cons)
    got = v1.span_fold_batch(seqs, L, max_w, cons)
    assert len(got) == len(seqs)
    for k, (seq, c) in enumerate(zip(seqs, cons)):
        assert equal(got[k], v1.span_fold(seq, L, max_w, c)), "item %d (n = %d) at L = %d, max_w = %d" % (k, len(seq), L, max_w)
        if L <= 60:
            close(got[k], cc.masked_cons(seq, L, c, max_w), "item %d (n = %d) L=%d max_w=%d" % (k, len(seq), L, max_w))
    assert all(equal(a, v1.span_batch_results(k)) for k, a in enumerate(got)), "the single calls left the batch alone"


# ---- 5
def test_chunk_budgets_change_no_bit(v1):
    L, max_w = BATCH_L, 15
    seqs, cons = ragged(L)
    sizes = [item_bytes(n, L, max_w) for n in LENGTHS]
    try:
        v1.set_span_batch_bytes(sum(sizes))
        whole = v1.span_fold_batch(seqs, L, max_w, cons)
        v1.set_span_batch_bytes(sizes[2])          # what the longest item takes: the chunks of the unconstrained batch
        some = v1.span_fold_batch(seqs, L, max_w, cons)
        v1.set_span_batch_bytes(1)
        each = v1.span_fold_batch(seqs, L, max_w, cons)
    finally:
        v1.set_span_batch_bytes(0)
    for k in range(len(seqs)):
        assert equal(whole[k], some[k]) and equal(whole[k], each[k]), "item %d" % k
    assert equal(whole[2], v1.span_fold(seqs[2], L, max_w, cons[2]))


# ---- 6
def test_refusals_keep_the_previous_results(v1):
    seqs, cons = ragged()
    seqs, cons = seqs[4:8], cons[4:8]
    single = v1.span_fold(seqs[0], 20, 5, cons[0])
    first = v1.span_fold_batch(seqs, 20, 5, cons)
    g = "GGGAAACCC"

    def kept(text):
        band, up, logz, _ = v1.local_results()
        assert equal((band, up, float(logz[0])), single), text
        assert all(equal(a, v1.span_batch_results(k)) for k, a in enumerate(first)), text

    for c, L, text in (("(((", 20, r"span fold: unbalanced '\('"), ("..)", 20, r"span fold: unbalanced '\)'"),
                       ("(...)", 20, "span fold: a forced pair of non-complementary letters"),
                       ("(.......)", 8, "span fold: the constraint pairs letters 1 and 9, which max_span 8 excludes")):
        assert v1.L.rh_span_fold_constrained(v1.h, g.encode(), 9, c.encode(), L, 1) == RH_ERR_ARG
        with pytest.raises(ractip_amd.RhError, match="error -1: " + text):
            v1.span_fold(g, L, 1, c)
        kept(text)
    for cs, L, text in (([None, "(((", ")"], 20, r"span fold batch: item 1: unbalanced '\('"),
                        (["(.......)", "(...)", None], 20, "span fold batch: item 1: a forced pair of non-complementary letters"),
                        (["..(...)", "..", ".(.....)"], 6, "span fold batch: item 2: the constraint pairs letters 2 and 8, which max_span 6 excludes")):
        with pytest.raises(ractip_amd.RhError, match="error -1: " + text):
            v1.span_fold_batch([g, g, g], L, 1, cs)
        kept(text)
    with pytest.raises(ractip_amd.RhError, match="2 constraints for 3 sequences"):
        v1.span_fold_batch([g, g, g], 20, 1, ["..", None])
    for args, text in (((g, 1, 1, "x"), "max_span 1"), ((g, 20, 65, "x"), "max_w 65"), (("", 20, 1, "x"), "length 0")):
        with pytest.raises(ractip_amd.RhError, match=text):
            v1.span_fold(*args)
        kept(text)
    # contexts without span kernels: RH_ERR_UNSUPPORTED exactly where rh_span_fold gives it
    cf = ractip_amd.Context(device=0)
    try:
        assert cf.L.rh_span_fold_constrained(cf.h, g.encode(), 9, b"(.......)", 20, 1) == RH_ERR_UNSUPPORTED
        with pytest.raises(ractip_amd.RhError, match="CONTRAfold"):
            cf.span_fold_batch([g], 20, 1, ["x"])
    finally:
        cf.close()
    v1.set_mode(hot.RH_MODE_LOG)
    try:
        with pytest.raises(ractip_amd.RhError, match="error -5.*log-space"):
            v1.span_fold(g, 20, 1, "x")
        with pytest.raises(ractip_amd.RhError, match="error -5.*log-space"):
            v1.span_fold_batch([g], 20, 1, ["x"])
    finally:
        v1.set_mode(hot.RH_MODE_AUTO)
    kept("log mode")
    c2 = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL, vienna=dict(semantics=2))
    try:
        with pytest.raises(ractip_amd.RhError, match="error -5.*2.x"):
            c2.span_fold(g, 20, 1, "x")
    finally:
        c2.close()


# ---- 7
def test_candidates_of_a_constrained_item_are_those_of_the_single_call(v1):
    items = [cc.case(300, 60), cc.case(13, 60), cc.case(129, 60, seed=6)]
    seqs, cons = [s for s, _ in items], [t for _, t in items]
    v1.span_fold_batch(seqs, 60, 15, cons)
    for item in (0, 2):
        asked = ((0, 0.5), (0, 0.01), (1, 0.9), (1, 0.2))
        got = [v1.span_batch_candidates(item, what, th) for what, th in asked]
        v1.span_fold(seqs[item], 60, 15, cons[item])
        want = [v1.local_candidates(what, th) for what, th in asked]
        for (rec, total), (ref, ref_total) in zip(got, want):
            assert total == ref_total > 0 and (rec == ref).all()


# ---- 8
def structure_line(cons):
    """a FASTA structure line that fold_constraint translates to cons: every third 'x' written as '[', ']' or 'e'"""
    out, k = [], 0
    for ch in cons:
        if ch == "x":
            ch = "x[]e"[k % 4]
            k += 1
        out.append(ch)
    return "".join(out)


def test_the_pipeline_and_the_command_line(v1, tmp_path):
    L, T = 60, 0.3
    items = [cc.case(300, L), cc.case(129, L, seed=6), cc.case(70, L, seed=2)]
    lines = [structure_line(t) for _, t in items]
    assert all(ch in lines[0] for ch in "[]ex") and [pipeline.fold_constraint(u, len(s))[:len(t)] for (s, t), u in zip(items, lines)] == [t for _, t in items]
    one = pipeline.span_fold(items[0][0], L, max_w=5, ctx=v1, structure=lines[0])
    assert equal((one["bp_band"], one["up"], one["logZ"]), v1.span_fold(items[0][0], L, 5, items[0][1]))
    close((one["bp_band"], one["up"], one["logZ"]), cc.masked_cons(items[0][0], L, items[0][1], 5), "pipeline.span_fold")
    many = pipeline.span_fold_batch([s for s, _ in items], L, max_w=5, ctx=v1, structures=[lines[0], None, lines[2]])
    assert equal((many[0]["bp_band"], many[0]["up"], many[0]["logZ"]), (one["bp_band"], one["up"], one["logZ"]))
    assert equal((many[1]["bp_band"], many[1]["up"], many[1]["logZ"]), v1.span_fold(items[1][0], L, 5))
    close((many[2]["bp_band"], many[2]["up"], many[2]["logZ"]), cc.masked_cons(items[2][0], L, items[2][1], 5), "pipeline.span_fold_batch")
    with pytest.raises(ValueError, match="2 structure lines for 3 sequences"):
        pipeline.span_fold_batch([s for s, _ in items], L, ctx=v1, structures=lines[:2])
    # the command line, in a child process: the first record, and every record
    fa = tmp_path / "many.fa"
    fa.write_text("".join(">rec%d some words\n%s\n%s\n%s\n" % (k, s[:50], s[50:], u) for k, ((s, _), u) in enumerate(zip(items, lines))))
    env = dict(os.environ, PYTHONPATH=ROOT)
    want = []
    for k, (s, t) in enumerate(items):
        ref = cc.masked_cons(s, L, t)
        assert not (np.abs(ref["band"] - T) < 1e-4).any(), "no probability sits on the threshold"
        want.append((ref["logZ"], sorted((i + 1, i + 1 + d) for i, d in zip(*np.nonzero(ref["band"] > T)))))

    def records(out):
        recs = []
        for line in out.splitlines():
            if line.startswith(">"):
                recs.append([line.split()[0][1:], float(line.split()[-1]), []])
            else:
                i, j, p = line.split()
                recs[-1][2].append((int(i), int(j)))
        return recs

    first = subprocess.run([sys.executable, "-m", "ractip_amd.pipeline", "--max-span", str(L), "--use-constraint", str(fa), "--threshold", str(T)],
                           capture_output=True, text=True, env=env, cwd=ROOT)
    assert first.returncode == 0, first.stderr[-2000:]
    every = subprocess.run([sys.executable, "-m", "ractip_amd.pipeline", "--max-span", str(L), "--use-constraint", "--all-records", "--threshold", str(T), str(fa)],
                           capture_output=True, text=True, env=env, cwd=ROOT)
    assert every.returncode == 0, every.stderr[-2000:]
    got = records(every.stdout)
    assert len(got) == 3 and records(first.stdout) == got[:1]
    for k, (name, logz, pairs) in enumerate(got):
        assert name == "rec%d" % k and abs(logz - want[k][0]) <= 1e-6 and pairs == want[k][1] and len(pairs) > 0, "record %d" % k
