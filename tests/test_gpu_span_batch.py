"""GPU suite: span folds in batches (rh_span_fold_batch) -- many sequences of ragged lengths through one set of launches, the item a
dimension of every grid.  Item k is the single call rh_span_fold_acc on the same context, bit for bit: "equal" below is == on every
array and on log Z.

  1  a ragged batch (lengths on both sides of the 64-entry exterior blocks, of the 256-column workgroup and of the 16-double row
     pitch, the shortest items between the longest) equals the single calls, at L = 2 .. L >= every n
  2  the batch against the CPU oracle under the band mask directly (rel 1e-6 on band and up above 1e-12, 1e-9 on log Z): a kernel
     that is wrong in the same way for batches and single calls passes 1 and fails here
  3  chunking changes no bit: one chunk, at least three with a single item among them, one item per chunk
     and an item whose tables start past 2^32 bytes of the chunk's buffers equals its single call
  4  the exponent ladder runs per item: the 1300-letter hairpin chain between ordinary sequences
  5  isolation and reuse: A, B, A; the local result, the uploaded batch and hp_loc2 are what they were; a single span fold leaves the batch
  6  refusals leave the previous batch result in place
  7  candidates of an item are those of the single call
  8  the pipeline: span_fold_batch, predict(max_span=L) on a batch of two (structures recorded from the commit before the batch
     existed: tests/golden/span_batch_predict.json), --all-records."""
import ctypes
import json
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
RH_OK, RH_ERR_ARG, RH_ERR_UNSUPPORTED = 0, -1, -5
LENGTHS = [257, 1, 300, 2, 13, 129, 63, 64, 65, 128]      # 1, 2, 13 between 257, 300 and 129
RAGGED = [sc.random_seq(n, seed=k) for k, n in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def v1(hotlib):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    yield c
    c.close()


def equal(a, b):
    return a[0].shape == b[0].shape and a[1].shape == b[1].shape and (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]


def item_bytes(n, L, max_w):
    """the plan formula: 13 band tables of Le * ldn doubles plus, at widths above one, the gap sums of 2 * 32 rows"""
    Le, ldn = min(n, L), -(-(n + 1) // 16) * 16
    return 13 * Le * ldn * 8 + (2 * 32 * ldn * 8 if max_w > 1 else 0)


def greedy(sizes, budget):
    """items per chunk: consecutive items while they fit the budget, at least one"""
    chunks, used = [], 0
    for b in sizes:
        if chunks and used + b <= budget:
            chunks[-1] += 1
            used += b
        else:
            chunks.append(1)
            used = b
    return chunks


def hairpin_chain(n=1300):
    """the chain of stable hairpins of tests/test_gpu_span_fold.py"""
    rs = np.random.RandomState(9)
    comp = {"G": "C", "C": "G"}
    seq = ""
    while len(seq) < n:
        stem = "".join(rs.choice(list("GC"), 10))
        seq += stem + "AAAA" + "".join(comp[x] for x in reversed(stem)) + "AA"
    return seq[:n]


def statuses(c, count):
    out = []
    for k in range(count):
        st = ctypes.c_int(99)
        assert c.L.rh_span_batch_item(c.h, k, None, None, ctypes.byref(st)) == RH_OK
        out.append(st.value)
    return out


# ---- 1
@pytest.mark.parametrize("L,max_w", [(2, 1), (4, 1), (31, 15), (33, 33), (70, 15), (400, 64)])
def test_a_ragged_batch_equals_the_single_calls(v1, L, max_w):
    got = v1.span_fold_batch(RAGGED, L, max_w)
    assert len(got) == len(RAGGED) and statuses(v1, len(RAGGED)) == [RH_OK] * len(RAGGED)
    count, span, w = (ctypes.c_int() for _ in range(3))
    assert v1.L.rh_span_batch_layout(v1.h, ctypes.byref(count), ctypes.byref(span), ctypes.byref(w)) == RH_OK
    assert (count.value, span.value, w.value) == (len(RAGGED), L, max_w)
    for k, seq in enumerate(RAGGED):
        assert got[k][0].shape == (len(seq), min(L, len(seq))) and got[k][1].shape == (len(seq), max_w)
        assert equal(got[k], v1.span_fold(seq, L, max_w)), "item %d (n = %d) at L = %d, max_w = %d" % (k, len(seq), L, max_w)
    assert all(equal(a, b) for a, b in zip(got, [v1.span_batch_results(k) for k in range(len(RAGGED))])), "the single calls left the batch alone"


# ---- 2
@pytest.mark.parametrize("L,max_w", [(7, 1), (7, 8), (31, 1), (31, 8)])
def test_against_the_masked_oracle(v1, L, max_w):
    seqs = [sc.random_seq(n) for n in (13, 65, 130)]
    for seq, (band, up, logz) in zip(seqs, v1.span_fold_batch(seqs, L, max_w)):
        ref = ac.masked_acc(seq, L, max_w) if max_w > 1 else sc.masked(seq, L)
        what = "n=%d L=%d max_w=%d" % (len(seq), L, max_w)
        assert band.shape == ref["band"].shape and up.shape == ref["up"].shape, what
        assert_log_close([logz], [ref["logZ"]], what=what + " log Z")
        assert_prob_close(band, ref["band"], what=what + " band")
        assert_prob_close(up, ref["up"], what=what + " up")


# ---- 3
def test_chunking_changes_no_bit(v1):
    L, max_w = 70, 15
    sizes = [item_bytes(n, L, max_w) for n in LENGTHS]
    try:
        v1.set_span_batch_bytes(sum(sizes))
        whole = v1.span_fold_batch(RAGGED, L, max_w)
        budget = sizes[2]                    # what the longest item takes: 257, 1 | 300 | 2, 13, 129, 63, 64 | 65, 128
        assert greedy(sizes, budget) == [2, 1, 5, 2] and greedy(sizes, sum(sizes)) == [10] and greedy(sizes, 1) == [1] * 10
        v1.set_span_batch_bytes(budget)
        some = v1.span_fold_batch(RAGGED, L, max_w)
        v1.set_span_batch_bytes(1)
        each = v1.span_fold_batch(RAGGED, L, max_w)
    finally:
        v1.set_span_batch_bytes(0)
    for k in range(len(RAGGED)):
        assert equal(whole[k], some[k]) and equal(whole[k], each[k]), "item %d" % k


def test_an_item_whose_tables_start_past_4_gib(v1):
    """three items of 100000 letters at L = 210: 2.18 GB of band tables each, so the third item's tables start past 2^32 bytes of
    the chunk's buffer; the first and the last item equal their single calls"""
    n, L, max_w = 100000, 210, 2
    assert 2 * item_bytes(n, L, max_w) > 2 ** 32 and 3 * item_bytes(n, L, max_w) < 16 * 2 ** 30      # one chunk under the default budget
    seqs = [sc.random_seq(n, seed=k) for k in range(3)]
    enc = [s.encode() for s in seqs]
    arr, lens = (ctypes.c_char_p * 3)(*enc), (ctypes.c_int * 3)(n, n, n)
    assert v1.L.rh_span_fold_batch(v1.h, arr, lens, 3, L, max_w) == RH_OK
    assert statuses(v1, 3) == [RH_OK] * 3
    for k in (2, 0):
        assert equal(v1.span_batch_results(k), v1.span_fold(seqs[k], L, max_w)), "item %d" % k


# ---- 4
def test_the_ladder_runs_per_item(v1):
    chain = hairpin_chain()
    seqs = [sc.random_seq(40, seed=1), sc.random_seq(300, seed=2), chain, sc.random_seq(129, seed=3), sc.random_seq(64, seed=4)]
    _, _, z = v1.fold(chain)
    assert z - 0.28 * len(chain) > np.log(1e280) + 50.0        # the chain's first attempt is flagged; the others' is not
    got = v1.span_fold_batch(seqs, 1300, 5)
    assert statuses(v1, 5) == [RH_OK] * 5
    assert_log_close([got[2][2]], [z], what="log Z of the chain")
    for k, seq in enumerate(seqs):
        assert equal(got[k], v1.span_fold(seq, 1300, 5)), "item %d" % k


# ---- 5
def test_isolation_and_reuse(v1):
    A, B = RAGGED[3:8], [sc.random_seq(n, seed=20 + n) for n in (90, 17, 260)]
    q, t = sc.random_seq(12, seed=1), sc.random_seq(60, seed=2)
    hp2 = v1.local_duplex2(q, t, 12, 1, 30, 10)
    v1.batch_upload([(q, t)])
    v1.batch_compute()
    uploaded = v1.batch_results(0)
    single = v1.span_fold(sc.random_seq(90), 33, 5)
    first = v1.span_fold_batch(A, 40, 5)
    other = v1.span_fold_batch(B, 33, 8)
    assert [x[0].shape for x in other] == [(90, 33), (17, 17), (260, 33)]
    again = v1.span_fold_batch(A, 40, 5)
    assert all(equal(a, b) for a, b in zip(first, again))
    band, up, logz, starts = v1.local_results()
    assert equal((band, up, logz[0]), single) and list(starts) == [0]
    after = v1.batch_results(0)
    assert all((np.asarray(uploaded[key]) == np.asarray(after[key])).all() for key in ("bp1", "bp2", "hp", "up1", "up2", "logZ"))
    assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(hp2[:2], v1.local_hp2_results()[:2]))
    v1.span_fold(sc.random_seq(300), 60, 15)                     # larger tables than the batch's, other widths
    assert all(equal(a, v1.span_batch_results(k)) for k, a in enumerate(first))


# ---- 6
def test_refusals_keep_the_previous_batch(ctx, v1):
    seqs = RAGGED[3:7]
    first = v1.span_fold_batch(seqs, 20, 5)
    enc = [s.encode() for s in seqs]

    def call(c, items, lens, count, L, w, null_seqs=False, null_lens=False):
        arr = (ctypes.c_char_p * len(items))(*items)
        n = (ctypes.c_int * len(lens))(*lens)
        return c.L.rh_span_fold_batch(c.h, None if null_seqs else arr, None if null_lens else n, count, L, w)

    lens = [len(s) for s in seqs]
    for args, text in (((enc, lens, 0, 20, 5), "0 items"), ((enc, lens, -2, 20, 5), "-2 items"),
                       ((enc, lens, 4, 20, 5, True), "array of sequences is NULL"), ((enc, lens, 4, 20, 5, False, True), "array of lengths is NULL"),
                       (([enc[0], None, enc[2], enc[3]], lens, 4, 20, 5), "item 1: the sequence is NULL"),
                       ((enc, lens[:3] + [0], 4, 20, 5), "item 3: the sequence has length 0"),
                       ((enc, [-1] + lens[1:], 4, 20, 5), "item 0: the sequence has length -1"),
                       ((enc, lens, 4, 1, 5), "max_span 1"), ((enc, lens, 4, 20, 0), "max_w 0"), ((enc, lens, 4, 20, 65), "max_w 65"),
                       ((enc, lens[:3] + [2 ** 31 - 1], 4, 20, 5), "item 3: the length 2147483647 overflows")):
        assert call(v1, *args) == RH_ERR_ARG, text
        assert text in v1.L.rh_last_error(v1.h).decode()
        assert all(equal(a, v1.span_batch_results(k)) for k, a in enumerate(first)), text
    for item in (-1, 4):
        assert v1.L.rh_span_batch_item(v1.h, item, None, None, None) == RH_ERR_ARG
        assert v1.L.rh_span_batch_results(v1.h, item, None, None, None) == RH_ERR_ARG
        assert v1.L.rh_span_batch_candidates(v1.h, item, 0, ctypes.c_float(0.5), None, 0) == RH_ERR_ARG
    with pytest.raises(ractip_amd.RhError, match="item 1"):
        v1.span_fold_batch([seqs[0], "", seqs[1]], 20, 5)
    # contexts without span kernels
    assert call(ctx, enc, lens, 4, 20, 5) == RH_ERR_UNSUPPORTED
    with pytest.raises(ractip_amd.RhError, match="CONTRAfold"):
        ctx.span_fold_batch(seqs, 20, 5)
    assert ctx.L.rh_span_batch_layout(ctx.h, None, None, None) == RH_ERR_ARG      # and there is no batch result
    v1.set_mode(hot.RH_MODE_LOG)
    try:
        assert call(v1, enc, lens, 4, 20, 5) == RH_ERR_UNSUPPORTED
        with pytest.raises(ractip_amd.RhError, match="log-space"):
            v1.span_fold_batch(seqs, 20, 5)
    finally:
        v1.set_mode(hot.RH_MODE_AUTO)
    assert all(equal(a, v1.span_batch_results(k)) for k, a in enumerate(first))
    c2 = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL, vienna=dict(semantics=2))
    try:
        assert call(c2, enc, lens, 4, 20, 5) == RH_ERR_UNSUPPORTED
        with pytest.raises(ractip_amd.RhError, match="2.x"):
            c2.span_fold_batch(seqs, 20, 5)
    finally:
        c2.close()


# ---- 7
def test_candidates_of_an_item_are_those_of_the_single_call(v1):
    seqs = [sc.random_seq(300), sc.random_seq(13), sc.random_seq(129, seed=6)]
    v1.span_fold_batch(seqs, 60, 15)
    for item in (0, 2):
        got = [v1.span_batch_candidates(item, what, th) for what, th in ((0, 0.5), (0, 0.01), (1, 0.9), (1, 0.2))]
        short = v1.span_batch_candidates(item, 0, 0.01, cap=3)
        v1.span_fold(seqs[item], 60, 15)
        want = [v1.local_candidates(what, th) for what, th in ((0, 0.5), (0, 0.01), (1, 0.9), (1, 0.2))]
        for (rec, total), (ref, ref_total) in zip(got, want):
            assert total == ref_total > 0 and (rec == ref).all()
        assert short[1] == want[1][1] and len(short[0]) == 3 and (short[0] == want[1][0][:3]).all()
    with pytest.raises(ractip_amd.RhError, match="what"):
        v1.span_batch_candidates(0, 2, 0.5)


# ---- 8
def oxys_fhla():
    fa = [l.strip() for l in open(os.path.join(ROOT, "ractip_amd", "data", "config5_OxyS_fhlA.fa")) if not l.startswith(">")]
    return fa[0], fa[1]


def test_the_pipeline_batch(v1):
    seqs = [sc.random_seq(90), sc.random_seq(13), sc.random_seq(130, seed=2)]
    got = pipeline.span_fold_batch(seqs, 33, max_w=5, ctx=v1)
    for seq, r in zip(seqs, got):
        one = pipeline.span_fold(seq, 33, max_w=5, ctx=v1)
        assert sorted(r) == sorted(one) and r["n"] == len(seq) and r["max_span"] == 33
        assert equal((r["bp_band"], r["up"], r["logZ"]), (one["bp_band"], one["up"], one["logZ"]))
    own = pipeline.span_fold_batch(seqs[:2], 33)
    assert own[0]["up"].shape == (90, 1) and (own[0]["bp_band"] == got[0]["bp_band"]).all() and own[1]["logZ"] == got[1]["logZ"]


def test_predict_folds_its_molecules_as_a_batch_of_two(hotlib):
    s1, s2 = oxys_fhla()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "span_batch_predict.json")))
    assert {c["max_span"] for c in golden["cases"]} >= {max(len(s1), len(s2)), 40}
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    try:
        for case in golden["cases"]:
            L = case["max_span"]
            r1, r2, _ = pipeline.predict(s1, s2, max_span=L, ctx=c)
            assert (r1, r2) == (case["r1"], case["r2"]), "the structures at max_span %d are those of the commit before" % L
            w = max(1, pipeline.ilp.Options().max_w)
            for k, s in enumerate((s1, s2)):                                # the batch result is still the context's
                assert equal(c.span_batch_results(k), c.span_fold(s, L, w))
    finally:
        c.close()


def test_all_records_prints_the_single_file_outputs(hotlib, tmp_path):
    seqs = [sc.random_seq(90), sc.random_seq(13), sc.random_seq(130, seed=2)]
    env = dict(os.environ, PYTHONPATH=ROOT)
    many = tmp_path / "many.fa"
    many.write_text("".join(">rec%d some words\n%s\n%s\n" % (k, s[:50], s[50:]) for k, s in enumerate(seqs)))
    singles = []
    for k, s in enumerate(seqs):
        fa = tmp_path / ("rec%d.fa" % k)
        fa.write_text(">rec%d some words\n%s\n" % (k, s))
        out = subprocess.run([sys.executable, "-m", "ractip_amd.pipeline", str(fa), "--max-span", "33", "--threshold", "0.3"], capture_output=True,
                             text=True, env=env, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        singles.append(out.stdout)
    out = subprocess.run([sys.executable, "-m", "ractip_amd.pipeline", "--max-span", "33", "--all-records", "--threshold", "0.3", str(many)],
                         capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout == "".join(singles) and len(out.stdout.splitlines()) > 3
    first = subprocess.run([sys.executable, "-m", "ractip_amd.pipeline", "--max-span", "33", "--threshold", "0.3", str(many)], capture_output=True,
                           text=True, env=env, cwd=ROOT)
    assert first.stdout == singles[0], "without --all-records the command line reads the first record, as before"
