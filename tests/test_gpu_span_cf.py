"""GPU suite: span folds under the CONTRAfold model (rh_set_span_contrafold; kernels in ractip_amd/csrc/mccaskill_span_cf.hip) --
the ensemble of rh_fold on a CONTRAfold context restricted to pairs (a, b) of complementary letters with b - a < L.

The reference is tests/_cf_span_ref.py, the numpy restatement of the oracle's recurrences with the band and-ed into `pairable`
(pinned to the oracle by tests/test_cf_span_ref_cpu.py): band and up at rel 1e-6 above 1e-12, log Z at 1e-9.  The shapes are those
of tests/test_gpu_span_fold.py, for the same reasons: no pair possible (L = 2, 4) and the first possible pair (L = 5); the loop
budget of 30 (L = 31..34); the wavefront edge of the FM2 rows (L = 63..65 at n = 130); the exterior passes' blocks of 64 entries
(n = 64, 65, 66 at L >= n; n = 128, 129); two workgroup columns (n = 256..258); unpadded rows (n = 47); L >= n, also against
Context.fold of the same context.  A subset runs under the scrambled weight file (tests/_contrafold_weights.py), whose
external_unpaired is not the bundled -0.0097: the unpaired step's weight is folded into the cells (span_fold.h).  Then the exponent
ladder (a chain of GC hairpins), 20000 letters that factorise, batches, and the interface: the switch, what stays refused, the
pipeline and the command line.  Every context here is the module's own: the session's `ctx` fixture is never switched on."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot, pipeline
import _cf_span_ref as ref
import _contrafold_weights as cw
import _span_cases as sc
from _oracle import Oracle, assert_log_close, assert_prob_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RH_OK, RH_ERR_ARG, RH_ERR_UNSUPPORTED = 0, -1, -5
END_PAIR = "GGGCGCGG" + sc.random_seq(54, seed=3, plant_n=False) + "CCGCGCCC"
SHAPES = [(40, 2), (40, 4), (40, 5), (90, 31), (90, 32), (90, 33), (90, 34), (130, 63), (130, 64), (130, 65), (64, 70), (65, 70), (66, 70),
          (128, 40), (129, 40), (256, 20), (257, 20), (258, 20), (47, 20), (300, 60), (70, 70), (70, 500)]
LENGTHS = [257, 1, 300, 3, 13, 129, 64, 65]               # 13 < L = 33 and 1, 3 < 5 between the longest
RAGGED = [sc.random_seq(n, seed=k) for k, n in enumerate(LENGTHS)]


def make(param_file=None, on=True):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_CONTRAFOLD, param_file=param_file)
    if on:
        c.set_span_contrafold(True)
    return c


@pytest.fixture(scope="module")
def cf(hotlib):
    c = make()
    yield c
    c.close()


@pytest.fixture(scope="module")
def scrambled(hotlib, tmp_path_factory):
    path = cw.write(tmp_path_factory.mktemp("spancf") / "scrambled.params", cw.scrambled())
    c = make(path)
    yield c, path
    c.close()


def check(got, want, what):
    band, up, logz = got
    assert band.shape == want["band"].shape and up.shape == want["up"].shape, what
    assert_log_close([logz], [want["logZ"]], what=what + " log Z")
    assert_prob_close(band, want["band"], what=what + " band")
    assert_prob_close(up, want["up"], what=what + " up")
    n, ld = band.shape
    i, d = np.arange(n)[:, None], np.arange(ld)[None, :]
    assert not band[(d == 0) | (i + d >= n)].any(), what + ": column 0 and the entries past the end hold 0"


def err(c):
    return c.L.rh_last_error(c.h).decode()


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


def equal(a, b):
    return a[0].shape == b[0].shape and a[1].shape == b[1].shape and (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]


def hairpin_chain(n):
    """the chain of stable hairpins of tests/test_gpu_span_fold.py"""
    rs = np.random.RandomState(9)
    comp = {"G": "C", "C": "G"}
    seq = ""
    while len(seq) < n:
        stem = "".join(rs.choice(list("GC"), 10))
        seq += stem + "AAAA" + "".join(comp[x] for x in reversed(stem)) + "AA"
    return seq[:n]


# ---- parity
@pytest.mark.parametrize("n,L", SHAPES)
def test_parity_with_the_band_masked_restatement(cf, n, L):
    seq = sc.random_seq(n)
    assert "N" in seq
    check(cf.span_fold(seq, L), ref.span_ref(seq, L), "n=%d L=%d" % (n, L))


@pytest.mark.parametrize("L", [2, 4])
def test_no_pair_is_possible(cf, L):
    seq = sc.random_seq(40)
    band, up, logz = cf.span_fold(seq, L)
    assert not band.any() and (up == 1.0).all()
    assert_log_close([logz], [40 * ref.span_ref(seq, L)["eu"]], what="log Z of the unpaired chain")


def test_the_first_possible_pair(cf):
    band, _, _ = cf.span_fold(sc.random_seq(40), 5)
    assert band[:, 4].any() and not band[:, :4].any()


@pytest.mark.parametrize("n,L", [(90, 33), (130, 64), (257, 20)])
def test_parity_under_the_scrambled_weights(scrambled, n, L):
    c, path = scrambled
    seq = sc.random_seq(n)
    want = ref.span_ref(seq, L, path)
    assert abs(want["eu"] + 0.0097) > 0.01, "the scrambled file moves external_unpaired"
    check(c.span_fold(seq, L), want, "scrambled n=%d L=%d" % (n, L))


@pytest.mark.parametrize("L", [70, 500])
def test_span_at_least_the_length_is_the_whole_fold(cf, L):
    seq = sc.random_seq(70)
    band, up, logz = cf.span_fold(seq, L)
    bp, fup, z = cf.fold(seq)
    assert band.shape == (70, 70)
    assert_log_close([logz], [z], what="log Z against Context.fold")
    assert_prob_close(band, sc.tri_to_band(bp, 70, 70), rel=1e-9, what="band against Context.fold")
    assert_prob_close(up[:, 0], np.asarray(fup).reshape(70, -1)[:, 0], rel=1e-9, what="up against Context.fold")


def test_the_end_pair_sequence(cf):
    n = len(END_PAIR)
    whole, below = ref.span_ref(END_PAIR, n), ref.span_ref(END_PAIR, n - 1)
    assert whole["band"][0, n - 1] > 0.9 and whole["logZ"] - below["logZ"] > 2.0
    got = cf.span_fold(END_PAIR, n - 1)
    check(got, below, "end pair, L = n - 1")
    assert_prob_close(hot.band_to_tri(got[0]), below["post"], what="band_to_tri of the result")
    check(cf.span_fold(END_PAIR, n), whole, "end pair, L = n")


def test_the_exponent_ladder_takes_over_where_the_band_overflows(cf):
    """The chain of GC hairpins cut to 1560 letters, at L = n: log Z - 0.12 n (the default exponent of the CONTRAfold ladder) lies
    beyond the flag's 1e280 (kSpanHuge, the Vienna sweeps' threshold), so the first attempt is flagged and the call answers from a
    larger exponent -- with the whole fold's values (Context.fold takes its own ladder), and the context's fold bits stay."""
    seq = hairpin_chain(1560)
    n = len(seq)
    bp, fup, z = cf.fold(seq)
    assert z - 0.12 * n > np.log(1e280) + 50.0
    band, up, logz = cf.span_fold(seq, n)
    assert_log_close([logz], [z], what="log Z of the chain")
    assert_prob_close(band, sc.tri_to_band(bp, n, n), what="band of the chain")
    assert_prob_close(up[:, 0], np.asarray(fup).reshape(n, -1)[:, 0], what="up of the chain")
    bp1, _, z1 = cf.fold(seq)
    assert (bp1 == bp).all() and z1 == z


def test_twenty_thousand_letters_factorise(cf):
    """n = 20000, L = 30: 400 inserts of 14 random G/C letters (six distinct), each followed by 29 A's.  A pairs with neither G, C
    nor A, so with u = log Z("A"): log Z = n u + sum_k (log Z("A" + ins_k + "A") - 16 u), and band and up on an insert are the
    oracle's on "A" + ins + "A", cut back.  log F5i[j] leaves 0.12 j by more than 745 nats: a scaled-linear exterior would have
    left the double range, the logarithms of the exterior passes are doing work."""
    N, L, COUNT, M = 20000, 30, 400, 14
    o = Oracle()
    ins = sc.inserts(COUNT, M)
    seq, starts = sc.long_sequence(N, L, ins)
    u = o.inference("A")["logZ"]
    refs = {}
    for s in set(ins):
        r = o.inference("A" + s + "A")
        band = sc.tri_to_band(r["post"], M + 2, M + 2)
        up = 1.0 - np.array([band[i].sum() + sum(band[i - d, d] for d in range(1, i + 1)) for i in range(M + 2)])
        refs[s] = (r["logZ"], band[1:1 + M, :M], up[1:1 + M])
    gain = {s: refs[s][0] - (M + 2) * u for s in refs}
    total = N * u + sum(gain[s] for s in ins)
    # log F5i[j] from the identity at the end of every insert's spacer and at the last letter
    f5 = [(at + M + 1, (at + M + 1) * u + sum(gain[s] for s in ins[:k + 1])) for k, at in enumerate(starts)] + [(N, total)]
    assert max(abs(g - 0.12 * j) for j, g in f5) > 745.0
    band, up, logz = cf.span_fold(seq, L)
    assert band.shape == (N, L) and up.shape == (N, 1)
    assert_log_close([logz], [total], what="log Z of the long sequence")
    covered = np.zeros(N, dtype=bool)
    for s, at in zip(ins, starts):
        _, rb, ru = refs[s]
        assert_prob_close(band[at:at + M, :M], rb, what="band on the insert at %d" % at)
        assert_prob_close(up[at:at + M, 0], ru, what="up on the insert at %d" % at)
        assert not band[at:at + M, M:].any()
        covered[at:at + M] = True
    assert not band[~covered].any() and (up[~covered] == 1.0).all()


# ---- batches
def item_bytes(n, L):
    """the plan formula under the CONTRAfold model: 11 band tables of Le * ldn doubles"""
    return 11 * min(n, L) * (-(-(n + 1) // 16) * 16) * 8


def test_a_ragged_batch_equals_the_single_calls_under_any_chunking(cf):
    L = 33
    sizes = [item_bytes(n, L) for n in LENGTHS]
    singles = [cf.span_fold(seq, L) for seq in RAGGED]
    try:
        whole = cf.span_fold_batch(RAGGED, L)
        cf.set_span_batch_bytes(max(sizes))        # 257, 1 | 300 | 3, 13, 129, 64 | 65: chunked by the bytes of ELEVEN tables per item
        assert greedy(sizes, max(sizes)) == [2, 1, 4, 1]
        some = cf.span_fold_batch(RAGGED, L)
        cf.set_span_batch_bytes(1)                 # one item per chunk
        each = cf.span_fold_batch(RAGGED, L)
    finally:
        cf.set_span_batch_bytes(0)
    for k, seq in enumerate(RAGGED):
        assert whole[k][0].shape == (len(seq), min(L, len(seq))) and whole[k][1].shape == (len(seq), 1)
        assert equal(whole[k], singles[k]) and equal(some[k], singles[k]) and equal(each[k], singles[k]), "item %d (n = %d)" % (k, len(seq))
    check(whole[2], ref.span_ref(RAGGED[2], L), "item 2 of the batch")
    check(whole[4], ref.span_ref(RAGGED[4], L), "item 4 of the batch (n < L)")
    assert equal(cf.span_fold(RAGGED[0], L), singles[0]), "a repeated call gives the same bits"


def test_candidates_of_a_batch_item_against_a_numpy_threshold(cf):
    got = cf.span_fold_batch(RAGGED, 33)
    band, up, _ = got[2]
    for th in (0.5, 0.01):
        rec, total = cf.span_batch_candidates(2, 0, th)
        i, d = np.nonzero(band.astype(np.float32) > np.float32(th))
        assert total == len(i) > 0
        assert (rec["i"] == i + 1).all() and (rec["j"] == i + 1 + d).all() and (rec["p"] == band[i, d].astype(np.float32)).all()
    rec, total = cf.span_batch_candidates(2, 1, 0.9)
    i = np.nonzero(up[:, 0].astype(np.float32) > np.float32(0.9))[0]
    assert total == len(i) > 0 and (rec["i"] == i).all() and (rec["p"] == up[i, 0].astype(np.float32)).all()


# ---- interface
def refused(c, seq, L, text):
    """the four entry points answer RH_ERR_UNSUPPORTED with `text` in the message"""
    enc = seq.encode()
    arr, lens = (ctypes.c_char_p * 1)(enc), (ctypes.c_int * 1)(len(seq))
    calls = [lambda: c.L.rh_span_fold(c.h, enc, len(seq), L), lambda: c.L.rh_span_fold_acc(c.h, enc, len(seq), L, 1),
             lambda: c.L.rh_span_fold_batch(c.h, arr, lens, 1, L, 1), lambda: c.L.rh_span_fold_constrained(c.h, enc, len(seq), None, L, 1)]
    for call in calls:
        assert call() == RH_ERR_UNSUPPORTED
        assert text in err(c)


def test_the_switch(hotlib):
    seq = sc.random_seq(40)
    c = make(on=False)
    try:
        assert c.get_span_contrafold() is False
        kept = c.local_fold(seq, 16, 5)
        refused(c, seq, 20, "CONTRAfold")
        with pytest.raises(ractip_amd.RhError, match="CONTRAfold"):
            c.span_fold(seq, 20)
        assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(kept, c.local_results()))
        c.set_span_contrafold(True)
        assert c.get_span_contrafold() is True
        check(c.span_fold(seq, 20), ref.span_ref(seq, 20), "switched on")
        c.set_span_contrafold(False)
        assert c.get_span_contrafold() is False
        refused(c, seq, 20, "CONTRAfold")
    finally:
        c.close()


def test_what_stays_refused_with_the_switch_on(cf):
    seq = sc.random_seq(90)
    first = cf.span_fold(seq, 33)
    batch = cf.span_fold_batch(RAGGED[:3], 33)

    def kept():
        band, up, logz, starts = cf.local_results()
        assert (band == first[0]).all() and (up == first[1]).all() and logz[0] == first[2] and list(starts) == [0]
        assert all(equal(cf.span_batch_results(k), batch[k]) for k in range(3))

    enc = seq.encode()
    arr, lens = (ctypes.c_char_p * 1)(enc), (ctypes.c_int * 1)(len(seq))
    cons = (ctypes.c_char_p * 1)(b"." * len(seq))
    for call, text in ((lambda: cf.L.rh_span_fold_acc(cf.h, enc, len(seq), 33, 2), "region accessibility"),
                       (lambda: cf.L.rh_span_fold_batch(cf.h, arr, lens, 1, 33, 4), "region accessibility"),
                       (lambda: cf.L.rh_span_fold_constrained(cf.h, enc, len(seq), b"." * len(seq), 33, 1), "constraint"),
                       (lambda: cf.L.rh_span_fold_batch_constrained(cf.h, arr, lens, 1, cons, 33, 1), "constraint")):
        assert call() == RH_ERR_UNSUPPORTED and text in err(cf), text
        kept()
    cf.set_mode(hot.RH_MODE_LOG)
    try:
        assert cf.L.rh_span_fold(cf.h, enc, len(seq), 33) == RH_ERR_UNSUPPORTED and "log-space" in err(cf)
        assert cf.L.rh_span_fold_batch(cf.h, arr, lens, 1, 33, 1) == RH_ERR_UNSUPPORTED and "log-space" in err(cf)
    finally:
        cf.set_mode(hot.RH_MODE_AUTO)
    kept()
    assert cf.L.rh_span_fold(cf.h, enc, len(seq), 1) == RH_ERR_ARG
    kept()
    # a NULL constraint (every entry NULL for a batch) is the plain call
    assert cf.L.rh_span_fold_constrained(cf.h, enc, len(seq), None, 33, 1) == RH_OK
    nulls = (ctypes.c_char_p * 1)(None)
    assert cf.L.rh_span_fold_batch_constrained(cf.h, arr, lens, 1, nulls, 33, 1) == RH_OK
    assert equal(cf.span_batch_results(0), first)


def test_the_setter_changes_nothing_on_a_vienna_context(hotlib):
    v = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    try:
        seq = sc.random_seq(90)
        before = v.span_fold(seq, 33)
        v.set_span_contrafold(True)
        assert v.get_span_contrafold() is False
        assert equal(v.span_fold(seq, 33), before)
        check(before, sc.masked(seq, 33), "the Vienna-BL span fold")
    finally:
        v.close()


def test_layout_times_and_the_fold_bits(cf):
    a = sc.random_seq(130)
    bp0, up0, z0 = cf.fold(a)
    cf.span_fold(sc.random_seq(90), 33)
    n, ld, nw, w = (ctypes.c_int() for _ in range(4))
    byref = ctypes.byref
    starts = np.full(1, -1, dtype=np.int32)
    assert cf.L.rh_local_layout(cf.h, byref(n), byref(ld), byref(nw), byref(w), starts.ctypes.data) == RH_OK
    assert (n.value, ld.value, nw.value, w.value, starts[0]) == (90, 33, 1, 1, 0)
    cf.span_fold(sc.random_seq(40), 70)
    assert cf.L.rh_local_layout(cf.h, byref(n), byref(ld), byref(nw), byref(w), None) == RH_OK
    assert (n.value, ld.value, nw.value, w.value) == (40, 40, 1, 1)
    ms = cf.span_times()
    assert ms[0] > 0.0 and ms[1] > 0.0
    cf.span_fold_batch(RAGGED[:3], 33)
    bp1, up1, z1 = cf.fold(a)
    assert (bp0 == bp1).all() and (np.asarray(up0) == np.asarray(up1)).all() and z0 == z1


def test_the_pipeline_and_the_command_line(cf, tmp_path):
    seq, other = sc.random_seq(90), sc.random_seq(47)
    want = cf.span_fold(seq, 33)
    r = pipeline.span_fold(seq, 33, model="contrafold")
    assert equal((r["bp_band"], r["up"], r["logZ"]), want) and r["max_span"] == 33 and r["n"] == 90
    rb = pipeline.span_fold_batch([seq, other], 33, model="contrafold")
    assert equal((rb[0]["bp_band"], rb[0]["up"], rb[0]["logZ"]), want)
    for call in (lambda: pipeline.span_fold(seq, 33, model="contrafold", structure="." * 90),
                 lambda: pipeline.span_fold_batch([seq], 33, model="contrafold", structures=["." * 90])):
        with pytest.raises(ValueError, match="constraint"):
            call()
    with pytest.raises(ValueError):
        pipeline.predict(seq, other, model="contrafold", max_span=33)
    fa = tmp_path / "two.fa"
    fa.write_text(">one\n%s\n%s\n>two\n%s\n" % (seq[:50], seq[50:], other))
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *args: subprocess.run([sys.executable, "-m", "ractip_amd.pipeline", str(fa), "--max-span", "33", "--contrafold"] + list(args),
                                       capture_output=True, text=True, env=env, cwd=ROOT)

    def lines_of(name, res):
        i, d = np.nonzero(res["bp_band"].astype(np.float32) > np.float32(0.3))
        return [(">" + name, res["logZ"])] + [(int(a) + 1, int(a) + 1 + int(b)) for a, b in zip(i, d)]

    def parsed(text):
        out = []
        for ln in text.strip().splitlines():
            f = ln.split()
            out.append((f[0], float(f[2])) if ln.startswith(">") else (int(f[0]), int(f[1])))
        return out

    def same(got, want_lines):
        assert len(got) == len(want_lines)
        for g, w in zip(got, want_lines):
            if isinstance(w[0], str):
                assert g[0] == w[0] and abs(g[1] - w[1]) <= 1e-6
            else:
                assert g == w

    out = run("--threshold", "0.3")
    assert out.returncode == 0, out.stderr[-2000:]
    same(parsed(out.stdout), lines_of("one", r))
    out = run("--threshold", "0.3", "--all-records")
    assert out.returncode == 0, out.stderr[-2000:]
    same(parsed(out.stdout), lines_of("one", rb[0]) + lines_of("two", rb[1]))
    out = run("--use-constraint")
    assert out.returncode != 0 and "constraint" in out.stderr
