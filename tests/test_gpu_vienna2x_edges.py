"""GPU suite (-m gpu): pf_fold, pf_unstru and the two-molecule ensemble under RH_VIENNA_SEM_20 (the log-space kernels of
mccaskill_vienna.hip with the 2.x tables: stemE / stemM, loop kinds 3 and 4, tri- / tetra- / hexaloops) past the 16 letters that
enumeration reaches: at the lengths where lse_stream2 runs a second and a partial last iteration (4-wide at 256, 8-wide at 512), on
the first diagonals that hold a 30-letter loop, with loops planted at the budget and one letter past it, at every cut edge of the
co-fold, at every accessibility width class and under structure constraints.

The reference is oracle/vienna2x_oracle.c through OraclePool.fold2x / cofold2x: PARITY UNPINNED against ViennaRNA (absent); the
restatement is pinned to oracle/vienna2x.py (E_IntLoop, enumeration of every structure) by tests/test_vienna2x_oracle.py, which also
proves these inputs fit.  The context is the synthetic one of tests/test_gpu_vienna2x.py (vienna2x.random_tables(23) through a v2.0
parameter file).

Tolerances are the project's: REL = 1e-6 on bp and hp, REL with abs_floor = 1e-11 on up, 1e-9 * max(1, |log Z|) on log Z, the same
bits where only placement changes."""
import numpy as np
import pytest

import _vienna2x_cases as cases
from _oracle import OraclePool, assert_prob_close, tri_offset
from _vienna2x_cases import v2

pytestmark = pytest.mark.gpu

REL = 1e-6
TS = cases.TABLES


@pytest.fixture(scope="module")
def par_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("par") / "synthetic_v20.par")
    v2.write_par_v20(path, cases.tables())
    return path


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    p.tables2x(TS, cases.tables())
    yield p
    p.close()


def context(par_file, max_w=None, hybrid=False):
    import ractip_amd
    c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL, param_file=par_file, vienna=dict(use_bl_param=False))
    try:
        assert c.vienna_semantics() == 2
        c.set_hybrid(hybrid)
        if max_w is not None:
            c.set_max_w(max_w)
    except Exception:
        c.close()
        raise
    return c


def run_batch(c, pairs, hybrid=False):
    c.batch_upload(pairs)
    c.batch_compute()
    assert c.last_path() == 2, c.last_path()
    if hybrid:
        assert c.last_hybrid_path() == 2, c.last_hybrid_path()
    return [c.batch_results(p) for p in range(len(pairs))]


def logz_close(z, ref):
    return abs(z - ref) <= 1e-9 * max(1.0, abs(ref))


def check_fold(got, o, what):
    bp, up, z = got
    assert logz_close(z, o["logZ"]), (what, z, o["logZ"])
    assert_prob_close(bp, o["post"], rel=REL, what="bp " + what)
    assert_prob_close(up, o["up"], rel=REL, abs_floor=1e-11, what="up " + what)


def folds_of(pairs, res):
    """[(sequence, (bp, up, log Z))] of a batch"""
    out = []
    for (s1, s2), r in zip(pairs, res):
        out.append((s1, (r["bp1"], r["up1"].reshape(len(s1), -1), r["logZ"][0])))
        out.append((s2, (r["bp2"], r["up2"].reshape(len(s2), -1), r["logZ"][1])))
    return out


def same_bits(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).ravel(), np.asarray(y).ravel()), what


# ---- single folds at the stream and budget edges
@pytest.mark.parametrize("which", (0, 1), ids=("pinned", "unpinned"))
def test_edge_lengths_dense_vs_cpu_restatement(hotlib, par_file, opool, which):
    """bp, up (width 15) and log Z of every sequence of a ragged batch == the restatement, 8 sequences on the pinned grid and 10 on
    the other one; each sequence folded alone has the bits it has inside its batch"""
    pairs = cases.edge_batches()[which]
    assert (len(pairs) * 2 % 8 == 0) == (which == 0)
    for s1, s2 in pairs:
        opool.fold2x(TS, s1), opool.fold2x(TS, s2)
    c = context(par_file)
    try:
        assert c.max_w == 15
        got = folds_of(pairs, run_batch(c, pairs))
        alone = []
        for s, _ in got:
            alone.append(c.fold(s))
            assert c.last_path() == 2
    finally:
        c.close()
    for (s, g), a in zip(got, alone):
        what = "n=%d (%s batch)" % (len(s), "pinned" if which == 0 else "unpinned")
        same_bits(g, (a[0], a[1].reshape(len(s), -1), a[2]), "alone != in the batch, " + what)
        check_fold(g, opool.fold2x(TS, s).result(), what)


# ---- planted loops at the budget
def test_planted_loops_at_the_budget_vs_cpu_restatement(hotlib, par_file, opool):
    """a bulge of 30 against 31 (either side), 1xn at n = 29 against 30 (either side), 2x3 and 3x2, 14x16 against 15x16, and the 1x29
    loop closed by a pair of span 513 in a 520-letter sequence (FM2's second iteration beside the kind-3 lanes), one batch.  What
    the planted pairs weigh is asserted on the restatement by test_planted_loops_dominate_at_the_budget_and_vanish_past_it; here
    the kernels must give the same."""
    planted = cases.planted_inputs()
    seqs = [x[1] for x in planted]
    assert len(seqs) % 2 == 1
    seqs.append("A")
    for s in seqs:
        opool.fold2x(TS, s)
    pairs = list(zip(seqs[0::2], seqs[1::2]))
    c = context(par_file)
    try:
        got = dict(folds_of(pairs, run_batch(c, pairs)))
    finally:
        c.close()
    for name, s, p, q, at_budget in planted:
        o = opool.fold2x(TS, s).result()
        check_fold(got[s], o, "planted " + name)
        pq = got[s][0][tri_offset(len(s), p) + q]
        assert (pq >= 0.9) if at_budget else (pq <= 0.01), (name, pq)


# ---- two-molecule ensemble at the cut edges
def test_two_molecule_ensemble_at_the_cut_edges(hotlib, par_file, opool):
    """hp and log Z of the co_pf_fold semantics == the restatement: cut after letter 1, after letter 64, one letter before the end,
    n2 = 256 .. 258 (XP stream) and n1 = 256 .. 258 (XS stream); through cofold and through a batch under set_hybrid(True), the
    same bits on both routes"""
    pairs = cases.cut_pairs()
    for s1, s2 in pairs:
        opool.cofold2x(TS, s1, s2)
    c = context(par_file, hybrid=True)
    try:
        res = run_batch(c, pairs, hybrid=True)
        single = []
        for s1, s2 in pairs:
            single.append(c.cofold(s1, s2))
            assert c.last_hybrid_path() == 2
    finally:
        c.close()
    for (s1, s2), r, (hp, z) in zip(pairs, res, single):
        what = "cut %d of %d" % (len(s1), len(s1) + len(s2))
        o = opool.cofold2x(TS, s1, s2).result()
        assert np.array_equal(r["hp"], hp) and r["logZ"][2] == z, ("batch != cofold, " + what)
        assert logz_close(z, o["logZ"]), (what, z, o["logZ"])
        assert_prob_close(hp, o["hp"], rel=REL, what="hp " + what)


# ---- accessibility widths
def acc_pairs():
    seqs = cases.acc_seqs() + ["ACGU"]
    return list(zip(seqs[0::2], seqs[1::2]))


@pytest.mark.parametrize("W", cases.WIDTHS)
def test_accessibility_widths_under_2x(hotlib, par_file, opool, W):
    """up[i][w] = P(letters i+1 .. i+1+w unpaired), w < max_w, == the restatement (pinned to enumeration at width 4 and to
    1 - P(paired) at 520 letters), sequences shorter than the width among them"""
    pairs = acc_pairs()
    seqs = [s for pr in pairs for s in pr]
    for s in seqs:
        opool.fold2x(TS, s, W)
    c = context(par_file, max_w=W)
    try:
        assert c.max_w == W
        got = folds_of(pairs, run_batch(c, pairs))
    finally:
        c.close()
    for s, g in got:
        assert g[1].shape == (len(s), W)
        check_fold(g, opool.fold2x(TS, s, W).result(), "n=%d max_w=%d" % (len(s), W))
        assert (np.diff(g[1], axis=1) <= 1e-12).all() and g[1].min() >= 0 and g[1].max() <= 1 + 1e-12


def test_width_changes_on_one_context_under_2x(hotlib, par_file):
    """15 -> 64 -> 1 on one context: each step bit for bit what a fresh context computes"""
    pairs = acc_pairs()
    c = context(par_file)
    try:
        for W in (15, 64, 1):
            c.set_max_w(W)
            got = run_batch(c, pairs)
            f = context(par_file, max_w=W)
            try:
                want = run_batch(f, pairs)
            finally:
                f.close()
            for p, (r, r0) in enumerate(zip(got, want)):
                assert r["up1"].size == len(pairs[p][0]) * W
                for k in ("bp1", "bp2", "up1", "up2", "logZ"):
                    assert np.array_equal(r[k], r0[k]), ("max_w %d after another width" % W, p, k)
    finally:
        c.close()


# ---- constraints
def test_constrained_fold_under_2x(hotlib, par_file, opool):
    """a 130-letter fold under an 'x' run and a forced pair == the restatement under constraint_mask; the unconstrained call that
    follows equals the unconstrained restatement: the mask does not linger"""
    seq, cons = cases.constraint_case()
    n = len(seq)
    fo, fc = opool.fold2x(TS, seq), opool.fold2x(TS, seq, 15, cons)
    c = context(par_file)
    try:
        got = c.fold(seq, constraint=cons)
        assert c.last_path() == 2
        after = c.fold(seq)
        assert c.last_path() == 2
    finally:
        c.close()
    oc, of = fc.result(), fo.result()
    assert abs(oc["logZ"] - of["logZ"]) > 1e-3, "the constraint does not bind"
    check_fold(got, oc, "constrained n=130")
    check_fold(after, of, "unconstrained after a constrained fold, n=130")
    bp, up, _ = got
    x0, x1 = cases.CONS_X
    fi, fj = cases.CONS_FORCED
    assert up[x0 - 1:x1, 0].min() > 1 - 1e-12
    row = bp[tri_offset(n, fi) + fi + 1:tri_offset(n, fi) + n + 1]
    assert row.sum() == bp[tri_offset(n, fi) + fj] and bp[tri_offset(n, fi) + fj] > 0
    assert sum(bp[tri_offset(n, i) + fi] for i in range(1, fi)) == 0


def test_constrained_two_molecule_ensemble_under_2x(hotlib, par_file, opool):
    """a forced pair across the cut == the restatement under the mask over s1+s2, then the unconstrained ensemble"""
    s1, s2, cons = cases.co_constraint_case()
    fo, fc = opool.cofold2x(TS, s1, s2), opool.cofold2x(TS, s1, s2, cons)
    c = context(par_file)
    try:
        hp, z = c.cofold(s1, s2, constraint=cons)
        assert c.last_hybrid_path() == 2
        hp_free, z_free = c.cofold(s1, s2)
        assert c.last_hybrid_path() == 2
    finally:
        c.close()
    oc, of = fc.result(), fo.result()
    assert abs(oc["logZ"] - of["logZ"]) > 1e-3, "the constraint does not bind"
    assert logz_close(z, oc["logZ"]), (z, oc["logZ"])
    assert_prob_close(hp, oc["hp"], rel=REL, what="constrained cofold %d + %d" % (len(s1), len(s2)))
    f = cases.CO_FORCED
    assert hp[f] > 0 and abs(hp[f] - hp[f[0]].sum()) < 1e-15 and abs(hp[f] - hp[:, f[1]].sum()) < 1e-15
    assert logz_close(z_free, of["logZ"]), (z_free, of["logZ"])
    assert_prob_close(hp_free, of["hp"], rel=REL, what="cofold after a constrained call")
