"""GPU suite: indexed batches (rh_batch_upload_indexed) -- every distinct sequence folded once, pairs by index.

The shape of the main batch: 3 queries (7, 41, 70 letters) x 4 targets (23, 58, 64, 90 letters) = 12 pairs over 7 distinct sequences:
one sequence below kStripMinN = 40 beside strip-length ones, and lengths on both sides of the 58- and 64-column duplex group edges.
A second index over the same seven sequences (ROLES) adds two pairs in which a target is s1 and a query s2, and a sequence paired
with itself, so a sequence appears in both roles.  Both batches have the same longest sequence as their expanded form, so every sweep
gets the same plan, and a sequence's result bits depend on its own letters only: every per-pair output of the indexed batch must equal
the expanded batch's, bit for bit, under both models and both Vienna-BL hybridization sources."""
import os
import subprocess

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot
from _oracle import OraclePool, assert_log_close, assert_prob_close, check_pair_properties

pytestmark = pytest.mark.gpu

REL = 1e-6   # of tests/test_gpu_parity.py, for the same quantities

rng = np.random.RandomState(20261019)
QUERIES = ["".join(rng.choice(list("ACGU"), n)) for n in (7, 41, 70)]
TARGETS = ["".join(rng.choice(list("ACGU"), n)) for n in (23, 58, 64, 90)]
SEQS = QUERIES + TARGETS                                         # distinct indices 0..2 = queries, 3..6 = targets
CROSS = [(q, 3 + t) for q in range(3) for t in range(4)]         # 12 pairs
ROLES = CROSS + [(4, 1), (6, 6)]                                 # + target 58 as s1 with query 41 as s2, and target 90 with itself
ORACLE_PAIRS = (0, 6, 11)                                        # (7, 23), (41, 64), (70, 90)
TH = (0.01, 0.01, 0.001, 0.003, 0.003)                           # thresholds of the scans which = 0..4 (low enough for long lists)
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")


def expand(seqs, index):
    return [(seqs[i], seqs[j]) for i, j in index]


def snapshot(c, npairs):
    """Every per-pair output of the computed batch."""
    return dict(res=[c.batch_results(p) for p in range(npairs)],
                cand=[[c.batch_candidates(p, w, TH[w]) for w in range(5)] for p in range(npairs)],
                cand_all=[tuple(a.copy() for a in c.batch_candidates_all(w, TH[w])) for w in range(5)],
                logz=c.batch_logz())


def assert_same_bits(got, want, what):
    assert len(got["res"]) == len(want["res"])
    for p, (a, b) in enumerate(zip(got["res"], want["res"])):
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), "%s: pair %d %s differs" % (what, p, k)
    assert got["cand"] == want["cand"], what
    for w in range(5):
        assert np.array_equal(got["cand_all"][w][0], want["cand_all"][w][0]) and np.array_equal(got["cand_all"][w][1], want["cand_all"][w][1]), (what, w)
    assert np.array_equal(got["logz"], want["logz"]), what


def make_context(kind):
    """"cf-auto" / "cf-log": the CONTRAfold model on either path; "v-duplex": Vienna-BL with hp from pf_duplex; "v-cofold": from the
    two-molecule ensemble (seeded from the folds)."""
    if kind.startswith("cf"):
        c = ractip_amd.Context(device=0)
        c.set_mode(1 if kind == "cf-log" else 0)
    else:
        c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
        c.set_hybrid(kind == "v-cofold")
    return c


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    yield p
    p.close()


@pytest.fixture(scope="module", params=["v-duplex", "v-cofold"])
def vctx(hotlib, request):
    c = make_context(request.param)
    c.kind = request.param
    yield c
    c.close()


_runs = {}


def both(c, name, index):
    """(expanded, indexed) snapshots of one index on one context, computed once per (context, index)."""
    key = (id(c), name)
    if key not in _runs:
        c.batch_upload(expand(SEQS, index))
        c.batch_compute()
        plain = snapshot(c, len(index))
        c.batch_upload_indexed(SEQS, index)
        c.batch_compute()
        _runs[key] = (plain, snapshot(c, len(index)))
    return _runs[key]


# ---- 1. same bits as the expanded batch
@pytest.mark.parametrize("name", ["cross", "roles"])
def test_contrafold_same_bits_as_the_expanded_batch(ctx, name):
    plain, indexed = both(ctx, name, CROSS if name == "cross" else ROLES)
    assert_same_bits(indexed, plain, "CONTRAfold %s %s" % (ctx.path_name, name))


@pytest.mark.parametrize("name", ["cross", "roles"])
def test_vienna_same_bits_as_the_expanded_batch(vctx, name):
    plain, indexed = both(vctx, name, CROSS if name == "cross" else ROLES)
    assert_same_bits(indexed, plain, "%s %s" % (vctx.kind, name))
    if vctx.kind == "v-cofold":
        assert vctx.last_hybrid_path() == 1 and vctx.last_path() == 1   # the seeded sweeps on the linear kernels, no fallback


# ---- 2. against the oracles
def test_contrafold_against_the_oracle(ctx, opool):
    _, indexed = both(ctx, "cross", CROSS)
    pairs = expand(SEQS, CROSS)
    for p in ORACLE_PAIRS:
        s1, s2 = pairs[p]
        r = indexed["res"][p]
        o1, o2, od = opool.inference(s1).result(), opool.inference(s2).result(), opool.duplex(s1, s2).result()
        what = "pair %d (%d,%d)" % (p, len(s1), len(s2))
        assert abs(r["logZ"][0] - o1["logZ"]) < 1e-9 and abs(r["logZ"][1] - o2["logZ"]) < 1e-9, what
        assert_log_close([r["logZ"][2]], [od["logZ2"][0]], tol=1e-9, what=what)
        assert_prob_close(r["bp1"], o1["post"], rel=REL, what="bp1 " + what)
        assert_prob_close(r["bp2"], o2["post"], rel=REL, what="bp2 " + what)
        assert_prob_close(r["hp"], od["post"], rel=REL, what="hp " + what)
    for (s1, s2), r in zip(pairs, indexed["res"]):
        check_pair_properties(s1, s2, r)


def test_vienna_against_the_oracle(vctx, opool):
    _, indexed = both(vctx, "cross", CROSS)
    pairs = expand(SEQS, CROSS)
    for p in ORACLE_PAIRS:
        s1, s2 = pairs[p]
        r = indexed["res"][p]
        o1, o2 = opool.mccaskill(s1, max_w=15).result(), opool.mccaskill(s2, max_w=15).result()
        if vctx.kind == "v-cofold":
            od = opool.cofold(s1, s2).result()
            ohp, oz = od["hp"], od["logZ"]
        else:
            od = opool.pf_duplex(s1, s2).result()
            ohp, oz = od["pr"], od["logZ"]
        assert_prob_close(r["bp1"], o1["post"], rel=REL, what="bp1")
        assert_prob_close(r["bp2"], o2["post"], rel=REL, what="bp2")
        assert_prob_close(r["up1"], o1["up"], rel=REL, abs_floor=1e-11, what="up1")
        assert_prob_close(r["up2"], o2["up"], rel=REL, abs_floor=1e-11, what="up2")
        assert_prob_close(r["hp"], ohp, rel=REL, what="hp")
        assert np.abs(r["logZ"] - np.array([o1["logZ"], o2["logZ"], oz])).max() < 1e-8
    for (s1, s2), r in zip(pairs, indexed["res"]):
        # check_pair_properties states up = 1 - row sums, the CONTRAfold model's width-1 accessibility; the Vienna-BL accessibility has
        # fifteen widths from sums of its own (checked against the oracle above), so it is handed the row-sum form of this bp here
        rr = dict(r)
        for k, s in (("1", s1), ("2", s2)):
            n = len(s)
            P = np.zeros((n + 1, n + 1))
            P[np.triu_indices(n + 1, 0)] = r["bp" + k]
            rr["up" + k] = np.maximum(0.0, 1.0 - (P + P.T).sum(axis=1)[1:])
            # ... and its width-1 column agrees with that form: bp and up each hold REL against the oracle, the row sums to at most 1
            assert np.abs(r["up" + k][:, 0] - rr["up" + k]).max() < 3 * REL
        check_pair_properties(s1, s2, rr)


# ---- 3. the folds are shared
def test_the_folds_are_shared(ctx):
    ctx.batch_upload_indexed(SEQS, CROSS)
    assert ctx.batch_index() == (7, CROSS)
    ctx.batch_compute()
    allr = ctx.batch_results_all()
    assert len(allr["bp"]) == 7 and len(allr["up"]) == 7 and len(allr["hp"]) == 12 and allr["logZ"].shape == (12, 3)
    for p, (i, j) in enumerate(CROSS):
        r = ctx.batch_results(p)
        assert np.array_equal(allr["bp"][i], r["bp1"]) and np.array_equal(allr["bp"][j], r["bp2"])
        assert np.array_equal(allr["up"][i], r["up1"]) and np.array_equal(allr["up"][j], r["up2"])
        assert np.array_equal(allr["hp"][p], r["hp"]) and np.array_equal(allr["logZ"][p], r["logZ"])
    user = {0: (0, 0), 1: (4, 0), 2: (8, 0), 3: (0, 1), 4: (1, 1), 5: (2, 1), 6: (3, 1)}   # sequence -> (a pair that uses it, its side)
    for what, th in ((0, TH[0]), (1, TH[3])):
        recs, first = ctx.batch_candidates_seq_all(what, th)
        assert len(first) == 8 and first[0] == 0 and first[7] == len(recs) and len(recs) > 0
        for k, (p, side) in user.items():
            mine = recs[first[k]:first[k + 1]]
            single = ctx.batch_candidates(p, (0 if what == 0 else 3) + side, th)
            assert [(int(a), int(b), float(v)) for a, b, v in zip(mine["i"], mine["j"], mine["p"])] == [(i, j, float(np.float32(v))) for i, j, v in single]
    # the plain upload is the identity index
    ctx.batch_upload(expand(SEQS, CROSS)[:3])
    assert ctx.batch_index() == (6, [(0, 1), (2, 3), (4, 5)])


# ---- 4. fallbacks
def test_a_flagged_sequence_is_listed_once_and_flags_its_pairs(hotlib, opool):
    """The 700-letter GC helix of test_mixed_batch_only_the_flagged_problems_fall_back as the query of three pairs (CONTRAfold model,
    auto): it leaves the double range on the default exponent, is recomputed once, and its three hp and its bp agree with the oracle."""
    helix = "G" * 348 + "AAAA" + "C" * 348
    r60 = np.random.RandomState(60)
    targets = ["".join(r60.choice(list("ACGU"), 60)) for _ in range(3)]
    oh = opool.inference(helix)
    od = [opool.duplex(helix, t) for t in targets]
    c = make_context("cf-auto")
    try:
        c.batch_upload_indexed([helix] + targets, [(0, 1), (0, 2), (0, 3)])
        c.batch_compute()
        assert c.last_path() == 3
        assert sorted(c.batch_fallbacks(0) + c.batch_fallbacks(2)) == [0]
        for p, t in enumerate(targets):
            r = c.batch_results(p)
            o = od[p].result()
            assert abs(r["logZ"][2] - o["logZ2"][0]) < 1e-7 * abs(o["logZ2"][0])
            assert_prob_close(r["hp"], o["post"], rel=REL, what="helix duplex %d" % p)
            assert abs(r["logZ"][0] - oh.result()["logZ"]) < 1e-7 * abs(oh.result()["logZ"])
        assert_prob_close(c.batch_results(0)["bp1"], oh.result()["post"], rel=REL, what="helix bp")
    finally:
        c.close()


# ---- 5. reuse: graph keys, the pair image, dxtab_log
def _reuse_steps():
    r5 = np.random.RandomState(5)
    rnd = lambda n: "".join(r5.choice(list("ACGU"), n))
    a = [rnd(50), rnd(44), rnd(61), rnd(37)]                    # two plain pairs; permuted as an index: the same shapes
    c3 = [rnd(30), rnd(75), rnd(12), rnd(20), rnd(66), rnd(9)]  # three plain pairs, other shapes
    return [("plain", a, [(0, 1), (2, 3)], 0),
            ("indexed", a, [(2, 3), (0, 1)], 0),                # nseq = 2 npairs, every length bound equal: must not replay the plain graphs' image
            ("plain", c3, [(0, 1), (2, 3), (4, 5)], 0),
            ("indexed", SEQS, ROLES, 0),
            ("indexed", SEQS, ROLES, 1),                        # log-space kernels on the same upload ...
            ("indexed", SEQS, ROLES, 0)]                        # ... and back: the linear duplex kernels need their zero pad columns again


def _run_step(c, step):
    how, seqs, index, mode = step
    c.set_mode(mode)
    if how == "plain":
        c.batch_upload(expand(seqs, index))
    else:
        c.batch_upload_indexed(seqs, index)
    c.batch_compute()
    return snapshot(c, len(index))


@pytest.mark.parametrize("kind", ["cf-auto", "v-duplex", "v-cofold"])
def test_reused_context_has_the_bits_of_a_fresh_one(hotlib, kind):
    steps = _reuse_steps()
    c = make_context(kind)
    try:
        got = [_run_step(c, s) for s in steps]
    finally:
        c.close()
    for k, s in enumerate(steps):
        if k == 5:   # (step 5 on a fresh context is step 3)
            assert_same_bits(got[5], got[3], "%s step 5 against step 3" % kind)
            continue
        f = make_context(kind)
        try:
            assert_same_bits(got[k], _run_step(f, s), "%s step %d (%s)" % (kind, k, s[0]))
        finally:
            f.close()


# ---- 6. rejections
@pytest.mark.parametrize("bad", [[(0, 3), (1, 7)], [(0, 3), (-1, 4)], []], ids=["index-eq-nseq", "negative-index", "no-pairs"])
def test_rejected_uploads_leave_the_previous_batch(ctx, bad):
    _, indexed = both(ctx, "cross", CROSS)
    ctx.batch_upload_indexed(SEQS, CROSS)
    ctx.batch_compute()
    with pytest.raises(ractip_amd.RhError):
        ctx.batch_upload_indexed(SEQS, bad)
    assert ctx.batch_index() == (7, CROSS)
    assert_same_bits(snapshot(ctx, 12), indexed, "after a rejected upload")


# ---- 7. the C++ adapter: the indexed members return what the plain members return for the expanded pairs
def test_host_adapter_indexed_members(hotlib):
    """prob_cli prints %.9g floats and %.17g log Z: equal text is equal bits.  Also as an in-process shard of two contexts, whose
    blocks reference different subsets of the sequences."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "ractip_amd", "host")])
    cli = os.path.join(root, "ractip_amd", "host", "prob_cli")
    args = [s for i, j in ROLES[::3] for s in (SEQS[i], SEQS[j])]        # five pairs, sequences shared between them

    def out(mode, *front, devices="0"):
        return subprocess.run([cli, mode] + list(front) + args, check=True, capture_output=True, text=True, env=dict(os.environ, RACTIP_DEVICES=devices)).stdout

    plain = out("solve")
    assert plain.count("pair ") == 5
    assert out("solve_indexed") == plain and out("solve_indexed", devices="0,0") == plain
    assert out("solve_default_indexed", "15") == out("solve_default", "15")


# ---- 8. the upload clears hp by the lengths of ITS pairs
def test_hp_beyond_the_pairs_is_zero_on_reused_buffers(hotlib):
    """dx_hp_clear_rest zeroes what no posterior kernel writes, by the pair-major lengths pair_gather builds: a second batch of the
    same layout (buffers reused as they are) with shorter pairs in the slots of longer ones leaves nothing of the first in the
    padded hp matrices, for both kinds of upload."""
    r8 = np.random.RandomState(8)
    rnd = lambda n: "".join(r8.choice(list("ACGU"), n))
    long_ = [rnd(90) for _ in range(4)]
    short = [rnd(90), rnd(90), rnd(17), rnd(33), rnd(5)]
    c = make_context("cf-auto")
    try:
        for indexed in (False, True):
            c.batch_upload([(long_[0], long_[1]), (long_[2], long_[3]), (long_[1], long_[2])])
            c.batch_compute()
            index = [(0, 1), (2, 3), (4, 2)]
            if indexed:
                c.batch_upload_indexed(short, index)
            else:
                c.batch_upload(expand(short, index))
            c.batch_compute()
            bufs = c.batch_results_all_into()
            hp = np.array(bufs[2])
            hld = hp.shape[1] // 92                                  # rows = n1max + 2
            for p, (i, j) in enumerate(index):
                m = hp[p].reshape(92, hld).copy()
                n1, n2 = len(short[i]), len(short[j])
                assert m[1:n1 + 1, 1:n2 + 1].max() > 0
                m[1:n1 + 1, 1:n2 + 1] = 0.0
                assert not m.any(), (indexed, p)
            for b in bufs:
                c.pinned_free(b)
    finally:
        c.close()
