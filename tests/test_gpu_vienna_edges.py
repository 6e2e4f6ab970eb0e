"""GPU suite (-m gpu) for the Vienna-BL model (the default of `ractip a.fa b.fa`) at the lengths where its scaled linear kernels
(mccaskill_vlin.hip) and the f64-MFMA block products they share with the CONTRAfold model (mccaskill_far.hip) change form:
383 / 384 / 385 (a sequence takes the two-level products from 384 letters), 447 / 448 / 449 (seven 64-letter macro tiles),
511 / 512 / 513 (16-letter block and 64-letter group edges), the cut of the two-molecule ensemble on and next to those lengths,
constrained letters inside the tiles that the products read, every class of accessibility width (1 .. 64), and every switch that
changes what the single-molecule sweeps run.

The reference throughout is oracle/vienna_oracle.c through ViennaOracle: PARITY UNPINNED against ViennaRNA (absent and
unversioned); the restatement is itself pinned to brute-force enumeration of every structure (tests/test_vienna_oracle.py, the
widths above 30 included).  OraclePool runs its calls on a few threads while the GPU computes.

Tolerances are the project's: REL = 1e-6 on bp and hp, REL with abs_floor = 1e-11 on up, 1e-9 * max(1, |log Z|) on log Z, 1e-10
between two organisations of the same arithmetic, the same bits where only placement or launch mode changes."""
import contextlib
import os

import numpy as np
import pytest

from _oracle import OraclePool, assert_prob_close, tri_offset

pytestmark = pytest.mark.gpu

REL = 1e-6
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")
MODES = [("auto", 0, 1), ("log", 1, 2)]   # name, rh_set_mode, the rh_last_path it must report
MODE_IDS = [m[0] for m in MODES]


def rnd(rng, n):
    return "".join(rng.choice(list("ACGU"), n))


def put(s, letter, ch):
    """s with its 1-based letter replaced"""
    return s[:letter - 1] + ch + s[letter:]


@contextlib.contextmanager
def switches(env, clear=()):
    """The environment switches a context reads when it is created (rh_api.hip: kEnvSwitches): `env` set and `clear` unset."""
    saved = {k: os.environ.get(k) for k in set(env) | set(clear)}
    try:
        for k in clear:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def vcontext(mode=0, hybrid=False, max_w=None):
    import ractip_amd
    c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL)
    try:
        c.set_mode(mode)
        c.set_hybrid(hybrid)
        if max_w is not None:
            c.set_max_w(max_w)
    except Exception:
        c.close()
        raise
    return c


def run_batch(c, pairs, path=None):
    c.batch_upload(pairs)
    c.batch_compute()
    if path is not None:
        assert c.last_path() == path, (c.last_path(), path)
        assert c.batch_fallbacks(0) == [] and c.batch_fallbacks(2) == []
    return [c.batch_results(p) for p in range(len(pairs))]


def assert_same_bits(r, r0, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(r[k]), np.asarray(r0[k])), (what, k)


def logz_close(z, ref):
    return abs(z - ref) <= 1e-9 * max(1.0, abs(ref))


def check_folds(pairs, res, opool, what, max_w=15):
    """bp, up and log Z of every sequence of a batch against the CPU restatement"""
    for p, ((s1, s2), r) in enumerate(zip(pairs, res)):
        for s, key, ukey, kz in ((s1, "bp1", "up1", 0), (s2, "bp2", "up2", 1)):
            o = opool.mccaskill(s, max_w).result()
            w = "%s pair %d n=%d" % (what, p, len(s))
            assert logz_close(r["logZ"][kz], o["logZ"]), (w, r["logZ"][kz], o["logZ"])
            assert_prob_close(r[key], o["post"], rel=REL, what="%s %s" % (key, w))
            assert_prob_close(r[ukey], o["up"], rel=REL, abs_floor=1e-11, what="%s %s" % (ukey, w))


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    yield p
    p.close()


# ---- single-molecule folds at the block, group and two-level edges, ragged, pinned and not
EDGE_PINNED = ((383, 513), (384, 449), (385, 448), (447, 512))   # 8 sequences: the XCD-pinned grids
EDGE_UNPINNED = ((511, 257), (256, 255), (513, 64))              # 6 sequences
EDGE_SUB = (0, 3)   # pairs of the pinned batch that run again as an unpinned batch with the same longest length (513)


def edge_batches():
    rng = np.random.RandomState(384)
    return tuple([(rnd(rng, a), rnd(rng, b)) for a, b in lens] for lens in (EDGE_PINNED, EDGE_UNPINNED))


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_edge_lengths_dense_vs_cpu_restatement(hotlib, opool, name, mode, path):
    """bp, up (width 15) and log Z of every sequence == oracle/vienna_oracle.c (PARITY UNPINNED against ViennaRNA; the restatement is
    pinned to enumeration), on the scaled linear kernels (no fallback) and on the log-space kernels.  A sequence keeps its bits in any
    other batch with the same longest length (test_vienna_bl_full_batch states it at n = 500): two pairs of the pinned batch again as
    an unpinned batch."""
    pinned, unpinned = edge_batches()
    for s1, s2 in pinned + unpinned:
        opool.mccaskill(s1), opool.mccaskill(s2)
    sub = [pinned[p] for p in EDGE_SUB]
    assert max(len(s) for pr in sub for s in pr) == max(len(s) for pr in pinned for s in pr) and len(sub) * 2 % 8 != 0
    c = vcontext(mode)
    try:
        assert c.max_w == 15
        got_p = run_batch(c, pinned, path)
        got_u = run_batch(c, unpinned, path)
        got_s = run_batch(c, sub, path)
    finally:
        c.close()
    for q, p in enumerate(EDGE_SUB):
        assert_same_bits(got_s[q], got_p[p], ("pinned pair %d in an unpinned batch" % p, name))
    check_folds(pinned, got_p, opool, "pinned " + name)
    check_folds(unpinned, got_u, opool, "unpinned " + name)


# ---- the switches that change what the single-molecule sweeps run (plan_mc_vlin, far_products, vlin_finish_acc), on the pinned batch
# "kernels":   rh_batch_kernels names another kernel set, results to 1e-10
# "bits":      launch mode or a switch these sweeps read the same way as the default: the default's names and its bits
# "form":      the names are the same (the one- / two-level choice is made per sequence inside the block-product kernels): the sequences
#              that change form change some bit, the others keep theirs
# "order":     the names are the same although other kernel instances run (vlin_*_diag MODE 0 for MODE 1 / 2: the look-ahead sums
#              of the next diagonal are added in another order): results to 1e-10 and some bit of every sequence changes
# "acc":       only the accessibility changes organisation: bp and log Z keep their bits, up to 1e-10
# "misreport": FINDING.  plan_mc_vlin reports block size 32 / the LDS products, but the Vienna-BL sweeps have block
#              size 16 on the MFMA products only: the default kernels run and every bit is the default's.  The names differ, the
#              arithmetic cannot: these two switches do nothing on this model.
ORG_VARIANTS = [
    ({"RH_LIN_BS": "0"}, "kernels"),
    ({"RH_LIN_BS": "32"}, "misreport"),
    ({"RH_LOOKAHEAD": "0"}, "order"),
    ({"RH_LOOKAHEAD": "1"}, "bits"),      # any value but 0 selects the look-ahead pairs
    ({"RH_FAR2": "0"}, "form"),           # every sequence of 384 letters or more changes form (to one-level)
    ({"RH_FAR2": "1"}, "form"),           # only the 383-letter sequence changes form (to two-level)
    ({"RH_FAR_MFMA": "0"}, "misreport"),
    ({"RH_FAR_PK": "0"}, "kernels"),
    ({"RH_FAR_PK": "0", "RH_FAR2": "1"}, "kernels"),   # (the gathered products have no two-level form)
    ({"RH_LIN_BS": "0", "RH_LOOKAHEAD": "0"}, "kernels"),
    ({"RH_ACC_WIDE": "0"}, "acc"),
    ({"RH_ACC_FINAL_T": "0"}, "bits"),
    ({"RH_NO_GRAPH": "1"}, "bits"),
]
ORG_KEYS = sorted({k for env, _ in ORG_VARIANTS for k in env})


def run_organisation(env):
    pinned, _ = edge_batches()
    with switches(env, clear=ORG_KEYS):
        c = vcontext(0)
    try:
        res = run_batch(c, pinned, 1)
        return c.batch_kernels(), res
    finally:
        c.close()


@pytest.fixture(scope="module")
def org_default(hotlib):
    return run_organisation({})


@pytest.mark.parametrize("env,kind", ORG_VARIANTS, ids=["+".join("%s=%s" % kv for kv in env.items()) for env, _ in ORG_VARIANTS])
def test_single_molecule_organisations_agree_on_the_pinned_edge_batch(hotlib, org_default, env, kind):
    """The Vienna-BL counterpart of test_organisations_agree_on_a_pinned_production_batch: every variant against the default, whose
    results test_edge_lengths_dense_vs_cpu_restatement compares with the CPU restatement (PARITY UNPINNED against ViennaRNA; the
    restatement is pinned to enumeration)."""
    pinned, _ = edge_batches()
    seqs = [s for pr in pinned for s in pr]
    base_k, base = org_default
    kern, got = run_organisation(env)

    def fold_bits(q, keys):   # does sequence q have the default's bits?
        r, r0, k = got[q // 2], base[q // 2], q % 2
        return all(np.array_equal(r[key + "12"[k]], r0[key + "12"[k]]) for key in keys) and r["logZ"][k] == r0["logZ"][k]

    same = [fold_bits(q, ("bp", "up")) for q in range(len(seqs))]
    print("%r: names %s; sequences with the default's bits: %s" % (env, "differ" if kern != base_k else "equal",
                                                                    [len(s) for s, e in zip(seqs, same) if e]))
    if kind in ("bits", "misreport"):
        assert (kern == base_k) == (kind == "bits"), (env, kern)
        for p, (r, r0) in enumerate(zip(got, base)):
            assert_same_bits(r, r0, (env, p))
        return
    if kind == "kernels":
        assert kern != base_k, ("the variant ran the default kernels", env, kern)
    else:
        assert kern == base_k, (env, kern)
    if kind == "form":
        forced = env["RH_FAR2"] == "1"
        for s, e in zip(seqs, same):
            changes = (len(s) < 384) == forced
            assert e != changes, (env, len(s), "changed form" if changes else "kept its form")
    if kind == "order":
        assert not any(same), (env, "sequences that kept every bit", [len(s) for s, e in zip(seqs, same) if e])
    if kind == "acc":
        assert all(fold_bits(q, ("bp",)) for q in range(len(seqs))), env
    for p, (r, r0) in enumerate(zip(got, base)):
        what = "%r pair %d" % (env, p)
        assert np.allclose(r["logZ"], r0["logZ"], rtol=0, atol=1e-10), what
        for key in ("bp1", "bp2", "hp"):
            assert_prob_close(r[key], r0[key], rel=1e-10, what="%s %s" % (key, what))
        for key in ("up1", "up2"):
            assert np.abs(r[key] - r0[key]).max() <= 1e-10, (key, what)


# ---- constraints where the block products read: one 400-letter sequence (two-level form: 7 macro tiles per axis)
CONS_N = 400
X_RUN = (250, 262)        # 'x' over letters 250..262: across 256, the edge of a 64-letter group and of a 16-letter block
FORCED = (40, 350)        # '(' ... ')' of span 310: the pair's cell lies in a two-level tile
NEAR_384 = {383: "<", 384: "|", 385: ">"}


def constraint_cases():
    rng = np.random.RandomState(400)
    seq = put(put(rnd(rng, CONS_N), FORCED[0], "G"), FORCED[1], "C")
    x = list("." * CONS_N)
    x[X_RUN[0] - 1:X_RUN[1]] = "x" * (X_RUN[1] - X_RUN[0] + 1)
    f = list("." * CONS_N)
    f[FORCED[0] - 1], f[FORCED[1] - 1] = "(", ")"
    m = list("." * CONS_N)
    for letter, ch in NEAR_384.items():
        m[letter - 1] = ch
    return seq, {"x run": "".join(x), "forced pair": "".join(f), "< | > at 383..385": "".join(m)}


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_constraints_inside_the_block_products(hotlib, opool, name, mode, path):
    """fold(seq, constraint=...) under fold_constrained at a length that reaches the two-level block products, against
    vo.mccaskill(..., constraint=...) (PARITY UNPINNED against ViennaRNA; the restatement under the mask is pinned to enumeration by
    test_structure_constraints_equal_bruteforce).  Then the mask must not linger: an unconstrained fold on the same context has
    the bits of a fresh context."""
    seq, cases = constraint_cases()
    n = len(seq)
    free = opool.mccaskill(seq)
    c = vcontext(mode)
    try:
        got = {}
        for what, cons in cases.items():
            got[what] = c.fold(seq, constraint=cons)
            assert c.last_path() == path, (what, c.last_path())
        after = c.fold(seq)
        assert c.last_path() == path
    finally:
        c.close()
    c = vcontext(mode)
    try:
        fresh = c.fold(seq)
    finally:
        c.close()
    for a, b in zip(after, fresh):
        assert np.array_equal(a, b), "an unconstrained fold after constrained ones differs from a fresh context's"
    o = free.result()
    assert logz_close(fresh[2], o["logZ"])
    assert_prob_close(fresh[0], o["post"], rel=REL, what="unconstrained bp n=400 " + name)
    for what, cons in cases.items():
        oc = opool.constrained("mccaskill", seq, 15, constraint=cons)
        bp, up, z = got[what]
        w = "%s (%s)" % (what, name)
        assert logz_close(z, oc["logZ"]), (w, z, oc["logZ"])
        assert_prob_close(bp, oc["post"], rel=REL, what="constrained bp " + w)
        assert_prob_close(up, oc["up"], rel=REL, abs_floor=1e-11, what="constrained up " + w)
        if what in ("x run", "forced pair"):
            assert abs(oc["logZ"] - o["logZ"]) > 1e-3, (w, "the constraint does not bind")
        if what == "x run":
            assert up[X_RUN[0] - 1:X_RUN[1], 0].min() > 1 - 1e-12, w                      # 'x' letters are unpaired
        if what == "forced pair":
            fi, fj = FORCED
            row = bp[tri_offset(n, fi) + fi + 1:tri_offset(n, fi) + n + 1]
            assert row.sum() == bp[tri_offset(n, fi) + fj] and bp[tri_offset(n, fi) + fj] > 0, w   # fi pairs with fj or with nothing
            assert sum(bp[tri_offset(n, i) + fi] for i in range(1, fi)) == 0, w


# ---- two-molecule ensemble with the cut on and next to the two-level threshold and a group edge (N = 449), one-letter strands
CUT_PAIRS = ((384, 65), (383, 66), (385, 64), (448, 1), (1, 448), (320, 129))
CO_FORCED = (380, 40)     # s1[380] pairs s2[40]: a forced pair across the cut of the (384, 65) pair
CO_VARIANTS = ({"RH_CO_SEED": "0"}, {"RH_CO_WINDOW": "0"}, {"RH_CO_SEED": "0", "RH_CO_WINDOW": "0"})


def cut_pairs():
    rng = np.random.RandomState(449)
    pairs = [(rnd(rng, a), rnd(rng, b)) for a, b in CUT_PAIRS]
    pairs[0] = (put(pairs[0][0], CO_FORCED[0], "G"), put(pairs[0][1], CO_FORCED[1], "C"))
    return pairs


def run_cut_pairs(mode, env, path):
    with switches(env, clear=("RH_CO_SEED", "RH_CO_WINDOW")):
        c = vcontext(mode, hybrid=True)
    try:
        res = run_batch(c, cut_pairs(), path)
        assert c.last_hybrid_path() == path
        return res
    finally:
        c.close()


@pytest.fixture(scope="module")
def cut_default(hotlib, opool):
    for s1, s2 in cut_pairs():
        opool.cofold(s1, s2)
    return run_cut_pairs(0, {}, 1)


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_two_molecule_ensemble_at_the_cut_edges(hotlib, opool, cut_default, name, mode, path):
    """hp and log Z of co_pf_fold semantics == vo.cofold (PARITY UNPINNED against ViennaRNA; the restatement is pinned to
    enumeration by test_cofold_equals_bruteforce_enumeration), scaled linear sweeps (seeded from the single folds, windowed around
    the cuts) and log-space kernels."""
    pairs = cut_pairs()
    res = cut_default if mode == 0 else run_cut_pairs(mode, {}, path)
    for (s1, s2), r in zip(pairs, res):
        o = opool.cofold(s1, s2).result()
        what = "cut %d of %d (%s)" % (len(s1), len(s1) + len(s2), name)
        assert logz_close(r["logZ"][2], o["logZ"]), (what, r["logZ"][2], o["logZ"])
        assert_prob_close(r["hp"], o["hp"], rel=REL, what="hp " + what)


@pytest.mark.parametrize("env", CO_VARIANTS, ids=["+".join("%s=%s" % kv for kv in env.items()) for env in CO_VARIANTS])
def test_two_molecule_organisations_agree_at_the_cut_edges(hotlib, cut_default, env):
    """test_vienna_bl_two_molecule_organisations_agree (N <= 256) at N = 449: unseeded sweeps, every group launched, and both."""
    for (s1, s2), r, r0 in zip(cut_pairs(), run_cut_pairs(0, env, 1), cut_default):
        what = "%r cut %d of %d" % (env, len(s1), len(s1) + len(s2))
        assert abs(r["logZ"][2] - r0["logZ"][2]) <= 1e-10, what
        assert_prob_close(r["hp"], r0["hp"], rel=1e-10, what="hp " + what)


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_constrained_two_molecule_ensemble_at_the_cut_edge(hotlib, opool, name, mode, path):
    """The (384, 65) pair under a constraint over s1+s2: a forced intermolecular pair across the cut and an 'x' run in s1 across
    letter 256, against vo.cofold(..., constraint=...) (PARITY UNPINNED against ViennaRNA; pinned to enumeration on toys)."""
    s1, s2 = cut_pairs()[0]
    n1, n2 = len(s1), len(s2)
    cons = list("." * (n1 + n2))
    cons[CO_FORCED[0] - 1], cons[n1 + CO_FORCED[1] - 1] = "(", ")"
    cons[X_RUN[0] - 1:X_RUN[1]] = "x" * (X_RUN[1] - X_RUN[0] + 1)
    cons = "".join(cons)
    c = vcontext(mode)
    try:
        hp, z = c.cofold(s1, s2, constraint=cons)
        assert c.last_hybrid_path() == path
        free = c.cofold(s1, s2)
    finally:
        c.close()
    o = opool.constrained("cofold", s1, s2, constraint=cons)
    assert logz_close(z, o["logZ"]), (name, z, o["logZ"])
    assert_prob_close(hp, o["hp"], rel=REL, what="constrained cofold 384 + 65 (%s)" % name)
    assert hp[X_RUN[0]:X_RUN[1] + 1].max() == 0
    assert hp[CO_FORCED] > 0 and abs(hp[CO_FORCED] - hp[CO_FORCED[0]].sum()) < 1e-15 and abs(hp[CO_FORCED] - hp[:, CO_FORCED[1]].sum()) < 1e-15
    of = opool.cofold(s1, s2).result()   # the mask does not linger
    assert logz_close(free[1], of["logZ"]) and abs(of["logZ"] - o["logZ"]) > 1e-3
    assert_prob_close(free[0], of["hp"], rel=REL, what="cofold 384 + 65 after a constrained call (%s)" % name)


# ---- accessibility at every width class
# 1, 2; 14, 15, 16: vlin_acc_final_t has up to fifteen widths, from 16 on vlin_acc_final runs with max_w as the grid's z-dimension;
# 30, 31, 32: the longest interior-loop side is 30, the gap sums vanish above it; 64: the largest width rh_set_max_w takes
WIDTHS = (1, 2, 14, 15, 16, 30, 31, 32, 64)
# 1, 5, 20, 31: shorter than some of the widths; 55, 56, 57: the 56-span ring of vlin_acc_gaps_wide; 64, 65, 256, 257: wavefront and
# workgroup edges of vlin_acc_final_t and vlin_acc_final; 300
ACC_LENS = (1, 5, 20, 31, 55, 56, 57, 64, 65, 256, 257, 300)


def acc_pairs():
    rng = np.random.RandomState(64)
    seqs = [rnd(rng, n) for n in ACC_LENS]
    return list(zip(seqs[0::2], seqs[1::2]))


def ups(pairs, res, W):
    """[(sequence, up as (n, W))] of a batch; the shape the results came in is checked"""
    out = []
    for (s1, s2), r in zip(pairs, res):
        for s, u in ((s1, r["up1"]), (s2, r["up2"])):
            assert u.shape == ((len(s), W) if W > 1 else (len(s),)), (len(s), W, u.shape)
            out.append((s, u.reshape(len(s), W)))
    return out


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("W", WIDTHS)
def test_accessibility_at_every_width_class(hotlib, opool, W, name, mode, path):
    """up[i][w] = P(letters i+1 .. i+1+w unpaired), w < max_w, == pf_unstru semantics of oracle/vienna_oracle.c (PARITY UNPINNED
    against ViennaRNA; the restatement is pinned to enumeration, at widths above 30 by
    test_mccaskill_wide_widths_equal_bruteforce_enumeration), ragged lengths incl. sequences shorter than the width."""
    pairs = acc_pairs()
    for s1, s2 in pairs:
        opool.mccaskill(s1, W), opool.mccaskill(s2, W)
    c = vcontext(mode, max_w=W)
    try:
        assert c.max_w == W
        res = run_batch(c, pairs, path)
    finally:
        c.close()
    for s, up in ups(pairs, res, W):
        o = opool.mccaskill(s, W).result()
        assert_prob_close(up, o["up"], rel=REL, abs_floor=1e-11, what="up n=%d max_w=%d (%s)" % (len(s), W, name))
        assert (np.diff(up, axis=1) <= 1e-12).all(), (len(s), W, "up grows with the width")
        assert up.min() >= 0 and up.max() <= 1 + 1e-12


@pytest.mark.parametrize("W", (15, 16))
def test_accessibility_final_step_routes_have_the_same_bits(hotlib, W):
    """RH_ACC_FINAL_T=0 (one thread per letter and width) against the default: the same terms in the same order, the same bits at
    width 15 (test_vienna_bl_accessibility_organisations_agree); at 16 the default takes that route itself."""
    pairs = acc_pairs()

    def run(env):
        with switches(env, clear=("RH_ACC_FINAL_T",)):
            c = vcontext(0, max_w=W)
        try:
            return run_batch(c, pairs, 1)
        finally:
            c.close()

    for p, (r, r0) in enumerate(zip(run({"RH_ACC_FINAL_T": "0"}), run({}))):
        assert_same_bits(r, r0, ("RH_ACC_FINAL_T=0", W, p))


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_width_changes_between_uploads_on_one_context(hotlib, name, mode, path):
    """max_w sizes the up and gap buffers and is baked into the captured launches: 15 -> 64 -> 2 on one context, each bit for bit
    what a fresh context computes."""
    pairs = acc_pairs()
    c = vcontext(mode)
    try:
        for W in (15, 64, 2):
            c.set_max_w(W)
            got = run_batch(c, pairs, path)
            f = vcontext(mode, max_w=W)
            try:
                want = run_batch(f, pairs, path)
            finally:
                f.close()
            ups(pairs, got, W)
            for p, (r, r0) in enumerate(zip(got, want)):
                assert_same_bits(r, r0, ("max_w %d after another width" % W, name, p))
    finally:
        c.close()
