"""GPU suite (-m gpu): letters that are not A, C, G or U -- N, DNA's T, soft-masked lower case, X and '-' -- through every fold and duplex
kernel family, in ragged batches and alone.

Every kernel has its own code for such a letter ("Unknown letters"): under the CONTRAfold model it is code 4, which never
pairs, selects slot 4 of the 5-wide tables and doubles as the sentinel beyond both ends; under the Vienna model T reads as U and
everything else is code 0, row 0 of the mismatch and small-loop tables, "no neighbour" in the exterior and multiloop stems, and a
letter that keeps a hairpin out of the tri- / tetra- / hexaloop tables.  The inputs (tests/_alphabet_cases.py) substitute ONE letter of
a planted single-loop input, named by the role the energy model reads it in; tests/test_unknown_letters_cpu.py proves on the references
that each substitution moves log Z or a posterior by at least 100 x the tolerance used here, so a kernel that read the letter as A, as
U or as "none" fails.

References: oracle/cf_oracle.c (pinned to the reference's engines on these inputs by tests/golden/contrafold_unknown_letters.npz),
oracle/vienna_oracle.c and oracle/vienna2x_oracle.c (PARITY UNPINNED against ViennaRNA, which is absent; pinned to enumeration).

Tolerances are the project's: REL = 1e-6 on bp and hp, REL with abs_floor = 1e-11 on Vienna up, 2e-6 on the float CONTRAfold up,
1e-9 * max(1, |log Z|) on log Z, 1e-10 between two organisations, the same bits where only the spelling of the input changes."""
import numpy as np
import pytest

import _alphabet_cases as ac
import _contrafold_cases as cf
import _vienna2x_cases as v2cases
import test_gpu_batch_constraints as tbc
import test_gpu_contrafold_edges as tce
import test_gpu_duplex_edges as tde
import test_gpu_vienna_edges as tve
from _oracle import NEG, OraclePool, assert_prob_close, tri_offset
from _vienna2x_cases import v2

pytestmark = pytest.mark.gpu

REL = 1e-6
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")
MODES = tce.MODES       # ("auto", 0, 1), ("log", 1, 2): name, rh_set_mode, the rh_last_path it must report
MODE_IDS = tce.MODE_IDS
TS = v2cases.TABLES


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    p.tables2x(TS, v2cases.tables())
    s1, s2 = helper_batches()[1][5]       # (the longest oracle calls of the module, section j: queued first, they run beside the rest)
    p.mccaskill(s1), p.mccaskill(s2), p.cofold(s1, s2)
    yield p
    p.close()


def logz_close(z, ref):
    return abs(z - ref) <= 1e-9 * max(1.0, abs(ref))


def same_bits(r, r0, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(r[k]), np.asarray(r0[k])), (what, k)


def as_pairs(seqs, filler="A"):
    seqs = list(seqs) + [filler] * (len(seqs) % 2)
    return list(zip(seqs[0::2], seqs[1::2]))


def folds_of(pairs, res):
    """sequence -> (bp, up, log Z) of a batch"""
    out = {}
    for (s1, s2), r in zip(pairs, res):
        out[s1] = (r["bp1"], r["up1"], float(r["logZ"][0]))
        out[s2] = (r["bp2"], r["up2"], float(r["logZ"][1]))
    return out


# ---- a. CONTRAfold model: the planted roles on the strip edges, on the default organisation and on every other one
def cf_subs():
    return ac.cf_role_set() + ac.cf_short_set()


@pytest.fixture(scope="module")
def cf_runs(hotlib, opool):
    """Every role x loop input and its short copy on the default organisation, "auto" (strips) and "log", behind the 300-letter dummy"""
    seqs = [s.seq for s in cf_subs()]
    tce.submit(opool, seqs)
    out = {}
    for name, mode, path in MODES:
        c = tce.context(mode)
        try:
            out[name] = tce.run_batches(c, seqs, path, tce.KERNELS[name], far=tce.FAR_PK if name == "auto" else None)
        finally:
            c.close()
    return out


def assert_planted_cells_are_above_the_floor(opool, subs):
    """the closing and the enclosed pair of every input: the relative bar applies to them (a stem-middle substitution removes a pair
    of the stem's middle, not these)"""
    for s in subs:
        g, n = cf.coords(s.case), len(s.seq)
        post = opool.inference(s.seq).result()["post"]
        for x, y in ((g["a"], g["b"]), (g["a2"], g["b2"])):
            if s.seq[x - 1] in "ACGU" and s.seq[y - 1] in "ACGU":
                assert post[tri_offset(n, x) + y] > 1e-12, (s.what, x, y)


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_contrafold_roles_dense_vs_oracle(opool, cf_runs, name, mode, path):
    """lin_inside_strip / lin_outside_strip behind lin_inside_diag ("auto", rh_last_path = 1, no fallback) and mc_inside_diag /
    mc_outside_diag ("log"): bp, up and log Z of every role x loop input == oracle/cf_oracle.c, the closing pair on columns 57 / 58 and
    every residue of its diagonal mod 8, and the same roles at 41..79 letters"""
    subs = cf_subs()
    tce.check_against_the_oracle(opool, [s.seq for s in subs], cf_runs[name], name, [s.what for s in subs])
    assert_planted_cells_are_above_the_floor(opool, subs)
    for s in subs:
        up = cf_runs[name][s.seq].up           # N, n and T are all unknown letters here: unpaired
        assert all(up[p - 1] == 1.0 for p in s.pos), s.what


@pytest.mark.parametrize("rot", range(len(tce.VARIANTS)), ids=["+".join("%s=%s" % kv for kv in v[0].items()) for v in tce.VARIANTS])
def test_contrafold_roles_on_every_organisation(opool, cf_runs, rot):
    """Each organisation switch of test_gpu_contrafold_edges.py on a quarter of the role set (every role in every quarter); RH_SMALL=1
    on the whole short set (lin_small_fold, its own copy of the weights): against the oracle, and against the default to 1e-10 (the
    same bits where only placement or the launch mode changes)"""
    env, kernels, far, kind = tce.VARIANTS[rot]
    subs = ac.thinned(ac.cf_role_set(), rot) + (ac.cf_short_set() if "RH_SMALL" in env else ac.thinned(ac.cf_short_set(), rot))
    seqs, names = [s.seq for s in subs], [s.what for s in subs]
    c = tce.context(0, env)
    try:
        res = tce.run_batches(c, seqs, 1, kernels, far=far)
    finally:
        c.close()
    tce.check_against_the_oracle(opool, seqs, res, "%r" % (env,), names)
    base = cf_runs["auto"]
    for s, w in zip(seqs, names):
        a, b = res[s], base[s]
        if kind == "bits":
            assert np.array_equal(a.bp, b.bp) and np.array_equal(a.up, b.up) and a.z == b.z, (env, w)
            continue
        assert abs(a.z - b.z) <= 1e-10, (env, w, a.z, b.z)
        assert_prob_close(a.bp, b.bp, rel=1e-10, what="bp %r vs the default: %s" % (env, w))
        assert np.abs(a.up - b.up).max() <= 1e-10, (env, w)


# ---- b. CONTRAfold model: mixed letters at the lengths where the launch sequence changes form
CF_EDGE_PINNED = ((383, 39), (384, 40), (385, 41), (57, 110))       # 8 sequences
CF_EDGE_UNPINNED = ((58, 109), (385, 57), (40, 383))                # 6 sequences


def cf_edge_batches():
    rng = np.random.RandomState(385)
    return tuple([(ac.mixed(rng, a), ac.mixed(rng, b)) for a, b in lens] for lens in (CF_EDGE_PINNED, CF_EDGE_UNPINNED))


def check_cf_folds(opool, folds, what):
    for s, (bp, up, z) in folds.items():
        o = opool.inference(s).result()
        w = "%s n=%d" % (what, len(s))
        assert abs(z - o["logZ"]) < 1e-9 * max(1.0, abs(o["logZ"])), (w, z, o["logZ"])
        assert_prob_close(bp, o["post"], rel=REL, what="bp " + w)
        assert np.abs(up.astype(np.float32) - opool.cf.up_float(len(s), bp.astype(np.float32))).max() < 2e-6, "up " + w


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_contrafold_mixed_letters_at_the_edge_lengths(hotlib, opool, name, mode, path):
    """~6 % N, 3 % T, 8 % lower case at 39 / 40 / 41 (kStripMinN), 57 / 58 (a group), 109 / 110 (lin_small_fold's range) and
    383 / 384 / 385 letters (the two-level block products): dense == oracle/cf_oracle.c; each sequence alone has its bits of the batch"""
    pinned, unpinned = cf_edge_batches()
    assert {len(s) for b in (pinned, unpinned) for pr in b for s in pr} == {39, 40, 41, 57, 58, 109, 110, 383, 384, 385}
    for pr in pinned + unpinned:
        tce.submit(opool, pr)
    c = tce.context(mode)
    try:
        folds = {}
        for batch in (pinned, unpinned):
            c.batch_upload(batch)
            c.batch_compute()
            assert c.last_path() == path and c.batch_fallbacks(0) == [] and c.batch_fallbacks(2) == [], (c.last_path(), c.batch_fallbacks(0))
            folds.update(folds_of(batch, [c.batch_results(p) for p in range(len(batch))]))
        alone = {s: c.bpp(s) for s in folds}
        assert c.last_path() == path
    finally:
        c.close()
    check_cf_folds(opool, folds, name)
    for s, (bp, z) in alone.items():
        assert np.array_equal(bp, folds[s][0]) and z == folds[s][2], ("alone differs from the batch", name, len(s))


# ---- c. spelling changes nothing but what the model says
def spelling_pairs():
    rng = np.random.RandomState(120)
    return [(ac.mixed(rng, 120), ac.mixed(rng, 120)), (ac.mixed(rng, 400), ac.mixed(rng, 400))]


def run_spelled(c, pairs, single, path):
    """the batch results and the single-problem results (bpp / fold and duplex) of the pairs"""
    c.batch_upload(pairs)
    c.batch_compute()
    assert c.last_path() == path and c.batch_fallbacks(0) == [] and c.batch_fallbacks(2) == [], (c.last_path(), path)
    res = [c.batch_results(p) for p in range(len(pairs))]
    for (s1, s2), r in zip(pairs, res):
        r["single"] = np.concatenate([np.ravel(x) for s in (s1, s2) for x in single(c, s)] + [np.ravel(x) for x in c.duplex(s1, s2)])
    return res


def assert_spelling(res, res0, same, what):
    for p, (r, r0) in enumerate(zip(res, res0)):
        eq = all(np.array_equal(np.asarray(r[k]), np.asarray(r0[k])) for k in KEYS + ("single",))
        assert eq == same, (what, p, "the bits differ" if same else "not one bit differs")


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_contrafold_spelling(hotlib, name, mode, path):
    """Lower case, upper case and mixed case are the same input; T is an unknown letter like N (and so not U: some bit changes)"""
    pairs = spelling_pairs()
    assert all("T" in s.upper() and "N" in s.upper() and s != s.upper() for pr in pairs for s in pr)
    spell = lambda f: [(f(a), f(b)) for a, b in pairs]
    c = tce.context(mode)
    try:
        single = lambda c, s: c.bpp(s)
        base = run_spelled(c, pairs, single, path)
        assert_spelling(run_spelled(c, spell(str.lower), single, path), base, True, "lower case")
        assert_spelling(run_spelled(c, spell(str.upper), single, path), base, True, "upper case")
        assert_spelling(run_spelled(c, spell(lambda s: s.replace("T", "N").replace("t", "n")), single, path), base, True, "T -> N")
        assert_spelling(run_spelled(c, spell(lambda s: s.replace("T", "U").replace("t", "u")), single, path), base, False, "T -> U")
    finally:
        c.close()


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_vienna_bl_spelling(hotlib, name, mode, path):
    """Lower case is upper case, T is U, and X and '-' are the unknown letter N"""
    pairs = spelling_pairs()
    spell = lambda f: [(f(a), f(b)) for a, b in pairs]
    c = tve.vcontext(mode)
    try:
        single = lambda c, s: c.fold(s)
        base = run_spelled(c, pairs, single, path)
        assert_spelling(run_spelled(c, spell(str.lower), single, path), base, True, "lower case")
        assert_spelling(run_spelled(c, spell(str.upper), single, path), base, True, "upper case")
        assert_spelling(run_spelled(c, spell(lambda s: s.replace("T", "U").replace("t", "u")), single, path), base, True, "T -> U")
        assert_spelling(run_spelled(c, spell(lambda s: s.replace("N", "X").replace("n", "x")), single, path), base, True, "N -> X")
        assert_spelling(run_spelled(c, spell(lambda s: s.replace("N", "-").replace("n", "-")), single, path), base, True, "N -> -")
        assert_spelling(run_spelled(c, spell(lambda s: s.replace("T", "N").replace("t", "n")), single, path), base, False, "T -> N")
    finally:
        c.close()


# ---- d. degenerate inputs
def degenerate_batches():
    """(with, without): all-N sequences of 64 and 300 letters beside ordinary ones, and the ordinary ones in a batch with the same
    longest length"""
    rng = np.random.RandomState(64)
    o300, o120, o80, o41 = (cf.rnd(rng, n) for n in (300, 120, 80, 41))
    return [(o300, "N" * 64), ("N" * 300, o120), (o80, o41)], [(o300, o120), (o80, o41)]


def degenerate_run(c, opool_fold, name):
    with_n, without = degenerate_batches()
    c.batch_upload(without)
    c.batch_compute()
    plain = [c.batch_results(p) for p in range(len(without))]
    c.batch_upload(with_n)
    c.batch_compute()
    res = [c.batch_results(p) for p in range(len(with_n))]
    cand = [c.batch_candidates_all(which, 0.0) for which in (0, 1, 2)]
    cand = [(rec.copy(), first.copy()) for rec, first in cand]
    # the ordinary neighbours keep their bits
    assert np.array_equal(res[0]["bp1"], plain[0]["bp1"]) and np.array_equal(res[0]["up1"], plain[0]["up1"]) and res[0]["logZ"][0] == plain[0]["logZ"][0], name
    assert np.array_equal(res[1]["bp2"], plain[0]["bp2"]) and np.array_equal(res[1]["up2"], plain[0]["up2"]) and res[1]["logZ"][1] == plain[0]["logZ"][1], name
    same_bits(res[2], plain[1], name + ": the ordinary pair")
    # the all-N problems
    for p, key, ukey, kz, which in ((0, "bp2", "up2", 1, 1), (1, "bp1", "up1", 0, 0)):
        s = with_n[p][kz]
        assert set(s) == {"N"}
        r = res[p]
        o = opool_fold(s)
        assert logz_close(r["logZ"][kz], o["logZ"]), (name, len(s), r["logZ"][kz], o["logZ"])
        assert not r[key].any(), (name, len(s), "bp of an all-N sequence")
        assert not r["hp"].any() and r["logZ"][2] <= NEG / 2, (name, len(s), r["logZ"][2])
        for w in (which, 2):
            rec, first = cand[w]
            assert first[p + 1] == first[p], (name, len(s), "candidates of an all-N problem", w)
        yield s, r[ukey], o
    rec, first = cand[2]
    assert first[3] > first[2], "the ordinary pair has hp candidates at threshold 0"


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_all_n_sequences_in_a_batch(hotlib, opool, name, mode, path):
    """All-N sequences of 64 and 300 letters: log Z == the oracle, bp identically 0, up 1 (CONTRAfold) or the oracle's columns
    (Vienna-BL), hp 0 with the NEG sentinel on its log Z, no candidate record at threshold 0; their neighbours keep their bits"""
    c = tce.context(mode)
    try:
        for s, up, o in degenerate_run(c, lambda s: opool.inference(s).result(), "CONTRAfold " + name):
            assert (up == 1.0).all(), (name, len(s))
    finally:
        c.close()
    c = tve.vcontext(mode)
    try:
        for s, up, o in degenerate_run(c, lambda s: opool.mccaskill(s).result(), "Vienna-BL " + name):
            assert_prob_close(up, o["up"], rel=REL, abs_floor=1e-11, what="up of an all-N sequence n=%d %s" % (len(s), name))
    finally:
        c.close()


N_RUNS = ((420, 110, 310), (420, 1, 200))


def test_long_runs_of_n_whichever_path_the_library_takes(hotlib, opool):
    """201 and 200 unknown letters in 420: nothing pairs across half of the sequence, so the scaled values of the linear kernels see a
    partition function far from what the length suggests.  "auto" mode, dense against the oracle on whichever path was taken (it is
    printed, not asserted)."""
    pairs = [tuple(ac.n_run(*r) for r in N_RUNS)]
    for s in pairs[0]:
        opool.inference(s), opool.mccaskill(s)
    c = tce.context(0)
    try:
        c.batch_upload(pairs)
        c.batch_compute()
        took = "CONTRAfold: rh_last_path %d, fallbacks %r / %r" % (c.last_path(), c.batch_fallbacks(0), c.batch_fallbacks(2))
        folds = folds_of(pairs, [c.batch_results(0)])
    finally:
        c.close()
    print(took)
    for s, (bp, up, z) in folds.items():
        o = opool.inference(s).result()
        assert abs(z - o["logZ"]) < 1e-9 * max(1.0, abs(o["logZ"])), (took, z, o["logZ"])
        big = o["post"] > 1e-12
        assert (np.abs(bp - o["post"])[big] <= REL * o["post"][big]).all() and np.abs(bp - o["post"])[~big].max() <= 1e-12, took
        assert np.abs(up.astype(np.float32) - opool.cf.up_float(len(s), bp.astype(np.float32))).max() < 2e-6, took
    c = tve.vcontext(0)
    try:
        c.batch_upload(pairs)
        c.batch_compute()
        took = "Vienna-BL: rh_last_path %d, fallbacks %r / %r" % (c.last_path(), c.batch_fallbacks(0), c.batch_fallbacks(2))
        res = [c.batch_results(0)]
    finally:
        c.close()
    print(took)
    try:
        tve.check_folds(pairs, res, opool, "runs of N")
    except AssertionError as e:
        raise AssertionError("%s; %s" % (took, e))


# ---- e. CONTRAfold duplex
DX_LENS = ((130, 70), (58, 62), (64, 65))


def dx_pairs():
    rng = np.random.RandomState(130)
    return [("mixed %d x %d" % (a, b), ac.mixed(rng, a), ac.mixed(rng, b)) for a, b in DX_LENS]


@pytest.fixture(scope="module")
def dx_default(hotlib, opool):
    for _, s1, s2 in dx_pairs():
        opool.duplex(s1, s2)
    c = tde.cf_context(0, {})
    try:
        return tde.run_batch_and_alone(c, dx_pairs(), 1, tde.CF_KERNEL["auto"], alone=False)
    finally:
        c.close()


def test_contrafold_duplex_mixed_letters_vs_oracle(opool, dx_default):
    """dxl_strip8 and dx_sweep_diag on pairs with N, T and lower case at 58 / 62 / 64 / 65 / 70 / 130 letters (the 57- and 62-column
    group edges): hp and log Z == oracle/cf_oracle.c; hp rows and columns of unknown letters are 0"""
    pairs = dx_pairs()
    c = tde.cf_context(1, {})
    try:
        log = tde.run_batch_and_alone(c, pairs, 2, tde.CF_KERNEL["log"], alone=False)
    finally:
        c.close()
    for what, run in (("auto", dx_default), ("log", log)):
        tde.check_cf_against_the_oracle(pairs, run["res"], opool, what)
        for (_, s1, s2), r in zip(pairs, run["res"]):
            for i, ch in enumerate(s1):
                if ch.upper() not in "ACGU":
                    assert r["hp"][i + 1].max() == 0, (what, i)
            for j, ch in enumerate(s2):
                if ch.upper() not in "ACGU":
                    assert r["hp"][:, j + 1].max() == 0, (what, j)


@pytest.mark.parametrize("env,kernel", tde.CF_ORGS, ids=["+".join("%s=%s" % kv for kv in env.items()) for env, _ in tde.CF_ORGS])
def test_contrafold_duplex_mixed_letters_on_every_organisation(opool, dx_default, env, kernel):
    pairs = dx_pairs()
    c = tde.cf_context(0, env)
    try:
        run = tde.run_batch_and_alone(c, pairs, 1, kernel, alone=False)
    finally:
        c.close()
    tde.check_cf_against_the_oracle(pairs, run["res"], opool, kernel)
    for (what, _, _), r, r0 in zip(pairs, run["res"], dx_default["res"]):
        assert abs(r["logZ"][2] - r0["logZ"][2]) <= 1e-10, (kernel, what)
        assert_prob_close(r["hp"], r0["hp"], rel=1e-10, what="hp %s vs dxl_strip8: %s" % (kernel, what))


# ---- f. Vienna-BL folds
BL_LONG = 400     # one mixed sequence that reaches the two-level block products: the switches of the products act on it


def bl_pairs():
    """the role set, and one 400-letter mixed sequence as the last pair's second sequence"""
    seqs = [s.seq for s in ac.bl_gpu_set()]
    return as_pairs(seqs + ["A"] * (1 - len(seqs) % 2) + ac.mixed_seqs(BL_LONG, (BL_LONG,)))


@pytest.fixture(scope="module")
def bl_default(hotlib, opool):
    pairs = bl_pairs()
    for s1, s2 in pairs:
        opool.mccaskill(s1), opool.mccaskill(s2)
    c = tve.vcontext(0)
    try:
        res = tve.run_batch(c, pairs, 1)
        return c.batch_kernels(), res
    finally:
        c.close()


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_vienna_bl_roles_dense_vs_cpu_restatement(opool, bl_default, name, mode, path):
    """vlin_inside_diag / vlin_outside_diag ("auto", rh_last_path = 1, no fallback) and mcv_inside_diag / mcv_outside_diag ("log"): bp,
    up at max_w 15 and log Z of every Vienna-BL role x loop input == oracle/vienna_oracle.c (PARITY UNPINNED against ViennaRNA)"""
    pairs = bl_pairs()
    if mode == 0:
        res = bl_default[1]
    else:
        c = tve.vcontext(mode)
        try:
            res = tve.run_batch(c, pairs, path)
        finally:
            c.close()
    tve.check_folds(pairs, res, opool, "roles " + name)
    folds = folds_of(pairs, res)
    for s in ac.bl_gpu_set():
        if s.letter != "T":
            assert all(folds[s.seq][1][p - 1, 0] > 1 - 1e-12 for p in s.pos), s.what


@pytest.mark.parametrize("env,kind", tve.ORG_VARIANTS, ids=["+".join("%s=%s" % kv for kv in env.items()) for env, _ in tve.ORG_VARIANTS])
def test_vienna_bl_roles_on_every_single_molecule_organisation(opool, bl_default, env, kind):
    """Every switch of test_gpu_vienna_edges.py (the look-ahead and plain forms of vlin_*_diag, its widths, the block products, the
    accessibility routes) on the role set and one 400-letter mixed sequence, which the block products compute in their two-level
    form: against the restatement, and against the default to 1e-10.  That a switch took effect is read from rh_batch_kernels, as
    test_single_molecule_organisations_agree_on_the_pinned_edge_batch reads it: other names for "kernels" and "misreport" (where
    only the names differ: DESIGN.md 5.1c), the default's names otherwise; a changed form (RH_FAR2) or order (RH_LOOKAHEAD=0) keeps
    the names and changes bits of the long sequence."""
    pairs = bl_pairs()
    assert len(pairs[-1][1]) == BL_LONG >= 384 and max(len(s) for pr in pairs[:-1] for s in pr) < 64
    base_k, base = bl_default
    with tve.switches(env, clear=tve.ORG_KEYS):
        c = tve.vcontext(0)
    try:
        res = tve.run_batch(c, pairs, 1)
        kern = c.batch_kernels()
    finally:
        c.close()
    tve.check_folds(pairs, res, opool, "roles %r" % (env,))
    assert (kern != base_k) == (kind in ("kernels", "misreport")), (env, kind, kern, base_k)
    long_same = np.array_equal(res[-1]["bp2"], base[-1]["bp2"])
    if kind == "order" or env == {"RH_FAR2": "0"}:      # (RH_FAR2=1 forces the form this sequence has already)
        assert not long_same, (env, "the 400-letter sequence kept every bit")
    for p, (r, r0) in enumerate(zip(res, base)):
        what = "%r pair %d" % (env, p)
        if kind in ("bits", "misreport"):
            same_bits(r, r0, what)
            continue
        assert np.allclose(r["logZ"][:2], r0["logZ"][:2], rtol=0, atol=1e-10), what
        for key in ("bp1", "bp2"):
            assert_prob_close(r[key], r0[key], rel=1e-10, what="%s %s" % (key, what))
        for key in ("up1", "up2"):
            assert np.abs(r[key] - r0[key]).max() <= 1e-10, (key, what)


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("W", (1, 15, 16, 31, 64))
def test_vienna_bl_accessibility_over_a_run_of_unknown_letters(hotlib, opool, W, name, mode, path):
    """36 unknown letters, longer than the 30-letter side of an interior loop, at every width class"""
    s = ac.n_run(130, 40, 75)
    pairs = [(s, s[::-1])]
    for x in pairs[0]:
        opool.mccaskill(x, W)
    c = tve.vcontext(mode, max_w=W)
    try:
        res = tve.run_batch(c, pairs, path)
    finally:
        c.close()
    tve.check_folds(pairs, [dict(r, up1=r["up1"].reshape(130, W), up2=r["up2"].reshape(130, W)) for r in res], opool, "run of N", max_w=W)
    up = res[0]["up1"].reshape(130, W)
    for w in range(min(W, 36)):
        assert up[39:75 - w, w].min() > 1 - 1e-12, (W, w)      # a region inside the run is unpaired


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_vienna_bl_mixed_letters_in_the_block_products(hotlib, opool, name, mode, path):
    """383 (one-level products), 384 (two-level) and 449 letters (seven macro tiles) with N, T and lower case"""
    seqs = ac.mixed_seqs(449, (383, 384, 449, 64))
    pairs = as_pairs(seqs)
    for s in seqs:
        opool.mccaskill(s)
    c = tve.vcontext(mode)
    try:
        res = tve.run_batch(c, pairs, path)
    finally:
        c.close()
    tve.check_folds(pairs, res, opool, "mixed " + name)


# ---- g. Vienna-BL two-molecule ensemble and pf_duplex
CUT_LENS = ((63, 40, "last"), (64, 40, "first"), (65, 40, "both"), (383, 66, "both"))


def cut_pairs():
    rng = np.random.RandomState(63)
    out = []
    for a, b, where in CUT_LENS:
        s1, s2 = cf.rnd(rng, a), cf.rnd(rng, b)
        if where in ("last", "both"):
            s1 = s1[:-1] + "N"
        if where in ("first", "both"):
            s2 = "N" + s2[1:]
        out.append((s1, s2))
    return out


def end_pairs():
    """pf_duplex: N at each strand end, one at a time and all four"""
    rng = np.random.RandomState(65)
    out = []
    for k in range(5):
        s1, s2 = cf.rnd(rng, 30 + k), cf.rnd(rng, 66 - k)
        if k in (0, 4):
            s1 = "N" + s1[1:]
        if k in (1, 4):
            s1 = s1[:-1] + "N"
        if k in (2, 4):
            s2 = "n" + s2[1:]
        if k in (3, 4):
            s2 = s2[:-1] + "X"
        out.append((s1, s2))
    return out


def run_cut(mode, env, path):
    with tve.switches(env, clear=("RH_CO_SEED", "RH_CO_WINDOW")):
        c = tve.vcontext(mode, hybrid=True)
    try:
        res = tve.run_batch(c, cut_pairs(), path)
        assert c.last_hybrid_path() == path
        return res
    finally:
        c.close()


@pytest.fixture(scope="module")
def cut_default(hotlib, opool):
    for s1, s2 in cut_pairs():
        opool.cofold(s1, s2)
    return run_cut(0, {}, 1)


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_vienna_bl_unknown_letters_at_the_cut(opool, cut_default, name, mode, path):
    """The two-molecule ensemble with N as the last letter of s1, the first of s2, or both, the cut after letters 63, 64, 65 and 383:
    hp and log Z == vo.cofold (PARITY UNPINNED).  The kernels write an unknown neighbour and the missing one beyond the cut as the
    same code 0 (GAPOK(i) ? s_ip1 : 0), so the two score alike; what these inputs tell apart is that the N itself never pairs across
    the cut and that no dangle crosses it"""
    res = cut_default if mode == 0 else run_cut(mode, {}, path)
    for (s1, s2), r in zip(cut_pairs(), res):
        o = opool.cofold(s1, s2).result()
        what = "cut %d of %d (%s)" % (len(s1), len(s1) + len(s2), name)
        assert logz_close(r["logZ"][2], o["logZ"]), (what, r["logZ"][2], o["logZ"])
        assert_prob_close(r["hp"], o["hp"], rel=REL, what="hp " + what)


@pytest.mark.parametrize("env", tve.CO_VARIANTS, ids=["+".join("%s=%s" % kv for kv in env.items()) for env in tve.CO_VARIANTS])
def test_vienna_bl_cofold_organisations_agree_with_unknown_letters_at_the_cut(cut_default, env):
    for (s1, s2), r, r0 in zip(cut_pairs(), run_cut(0, env, 1), cut_default):
        what = "%r cut %d of %d" % (env, len(s1), len(s1) + len(s2))
        assert abs(r["logZ"][2] - r0["logZ"][2]) <= 1e-10, what
        assert_prob_close(r["hp"], r0["hp"], rel=1e-10, what="hp " + what)


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_vienna_bl_pf_duplex_with_unknown_strand_ends(hotlib, opool, name, mode, path):
    """pf_duplex (dxvl_sweep4<false> / dxv_sweep_diag) with N at each of the four strand ends and at all of them == vo.pf_duplex"""
    pairs = end_pairs()
    for s1, s2 in pairs:
        opool.pf_duplex(s1, s2)
    c = tve.vcontext(mode)
    try:
        res = tve.run_batch(c, pairs, path)
        assert c.last_hybrid_path() == path and c.batch_kernels()[2][0] == tde.V_KERNEL[name]
    finally:
        c.close()
    for (s1, s2), r in zip(pairs, res):
        o = opool.pf_duplex(s1, s2).result()
        what = "pf_duplex %s / %s (%s)" % (s1[0] + ".." + s1[-1], s2[0] + ".." + s2[-1], name)
        assert logz_close(r["logZ"][2], o["logZ"]), (what, r["logZ"][2], o["logZ"])
        assert_prob_close(r["hp"], o["pr"], rel=REL, what="hp " + what)


# ---- h. constraints over unknown letters (Vienna-BL)
def constrained_batch():
    """The ragged constrained batch of test_gpu_batch_constraints.py with N under every '|', '<', '>' and 'x', and under the first
    '.' inside every forced pair"""
    pairs, cons, joint = tbc.ragged_batch(tbc.PARITY_EXTRA)
    out, hit = [], set()
    for (s1, s2), (c1, c2), cj in zip(pairs, cons, joint):
        new = []
        for s, cs, own in ((s1, c1, (cj or "")[:len(s1)]), (s2, c2, (cj or "")[len(s1):])):
            s = list(s)
            for k, ch in enumerate(cs or ""):
                if ch in "|<>x" and own[k:k + 1] not in ("(", ")"):
                    s[k] = "N"
                    hit.add(ch)
            for i, j in tbc.matched(cs):
                for k in range(i + 1, j):
                    if cs[k] == "." and own[k:k + 1] not in ("(", ")"):
                        s[k] = "N"
                        hit.add("inside")
                        break
            new.append("".join(s))
        out.append(tuple(new))
    assert hit == set("|<>x") | {"inside"}
    return out, cons, joint


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_constraints_over_unknown_letters(hotlib, opool, name, mode, path):
    """The device-built masks do not depend on the letters: byte for byte constraint_mask; bp, up, hp and log Z == the restatement
    under the same mask"""
    pairs, cons, joint = constrained_batch()
    c = tbc.vcontext(mode, hybrid=True)
    try:
        res = tbc.run(c, pairs, cons, joint)
        assert c.last_path() == path, (c.last_path(), path)
        for p, (s1, s2) in enumerate(pairs):
            for q, s in enumerate((s1, s2)):
                m = c.debug_allow_mask(0, 2 * p + q)
                assert np.array_equal(m, tbc.expected_image(cons[p][q], len(s), m.shape[0])), ("sequence", 2 * p + q)
            m = c.debug_allow_mask(1, p)
            assert np.array_equal(m, tbc.expected_image(joint[p], len(s1) + len(s2), m.shape[0])), ("pair", p)
    finally:
        c.close()
    for p, ((s1, s2), r) in enumerate(zip(pairs, res)):
        for q, (s, key, ukey) in enumerate(((s1, "bp1", "up1"), (s2, "bp2", "up2"))):
            cs = cons[p][q]
            o = opool.mccaskill(s).result() if cs is None else opool.constrained("mccaskill", s, 15, constraint=cs)
            w = "%s sequence %d n=%d" % (name, 2 * p + q, len(s))
            assert logz_close(r["logZ"][q], o["logZ"]), (w, r["logZ"][q], o["logZ"])
            assert_prob_close(r[key], o["post"], rel=REL, what="bp " + w)
            assert_prob_close(r[ukey], o["up"], rel=REL, abs_floor=1e-11, what="up " + w)
        o = opool.cofold(s1, s2).result() if joint[p] is None else opool.constrained("cofold", s1, s2, constraint=joint[p])
        w = "%s pair %d (%d, %d)" % (name, p, len(s1), len(s2))
        assert logz_close(r["logZ"][2], o["logZ"]), (w, r["logZ"][2], o["logZ"])
        assert_prob_close(r["hp"], o["hp"], rel=REL, what="hp " + w)


def test_forced_pairs_on_unknown_and_respelled_letters(hotlib):
    """'(' on an N is rejected (RH_ERR_ARG) and the previous batch stays in place; '(' ... ')' on T-A and on g-c is accepted and
    equals U-A / G-C bit for bit"""
    import ractip_amd
    rng = np.random.RandomState(7)
    body = cf.rnd(rng, 30)
    good = [("U" + body + "A", "G" + body[::-1] + "C")]
    respelled = [("T" + body + "A", "g" + body[::-1] + "c")]
    cons = [("(" + "." * 30 + ")", "(" + "." * 30 + ")")]
    c = tbc.vcontext(0)
    try:
        want = tbc.run(c, good, cons)
        with pytest.raises(ractip_amd.RhError, match=r"error -1: sequence 0: a forced pair of non-complementary letters"):      # RH_ERR_ARG
            c.batch_upload([("N" + body + "A", good[0][1])], constraints=cons)
        same_bits(c.batch_results(0), want[0], "the batch before a rejected upload")
        c.batch_compute()
        same_bits(c.batch_results(0), want[0], "the batch before a rejected upload, computed again")
        same_bits(tbc.run(c, respelled, cons)[0], want[0], "T-A and g-c under a forced pair")
    finally:
        c.close()


# ---- i. 2.x semantics
@pytest.fixture(scope="module")
def par_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("par") / "synthetic_v20.par")
    v2.write_par_v20(path, v2cases.tables())
    return path


def context20(par_file, hybrid=False):
    import ractip_amd
    c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL, param_file=par_file, vienna=dict(use_bl_param=False))
    try:
        assert c.vienna_semantics() == 2
        c.set_hybrid(hybrid)
    except Exception:
        c.close()
        raise
    return c


def test_2x_roles_dense_vs_cpu_restatement(hotlib, par_file, opool):
    """mccaskill_vienna.hip under the 2.x tables (random set: row 0 of every mismatch table has values of its own): N at each letter
    of a tri-, tetra- and hexaloop, next to either pair of 1xn and 2x3 loops, as the one neighbour of an exterior stem and beside no
    neighbour at all == oracle/vienna2x_oracle.c (PARITY UNPINNED)"""
    subs = ac.v2_role_set()
    pairs = as_pairs([s.seq for s in subs])
    for s1, s2 in pairs:
        opool.fold2x(TS, s1), opool.fold2x(TS, s2)
    c = context20(par_file)
    try:
        c.batch_upload(pairs)
        c.batch_compute()
        assert c.last_path() == 2
        folds = folds_of(pairs, [c.batch_results(p) for p in range(len(pairs))])
    finally:
        c.close()
    for s in subs:
        o = opool.fold2x(TS, s.seq).result()
        bp, up, z = folds[s.seq]
        assert logz_close(z, o["logZ"]), (s.what, z, o["logZ"])
        assert_prob_close(bp, o["post"], rel=REL, what="bp " + s.what)
        assert_prob_close(up, o["up"], rel=REL, abs_floor=1e-11, what="up " + s.what)


def test_2x_cofold_with_unknown_letters_at_the_cut(hotlib, par_file, opool):
    pairs = cut_pairs()[:3]
    for s1, s2 in pairs:
        opool.cofold2x(TS, s1, s2)
    c = context20(par_file, hybrid=True)
    try:
        c.batch_upload(pairs)
        c.batch_compute()
        assert c.last_hybrid_path() == 2
        res = [c.batch_results(p) for p in range(len(pairs))]
    finally:
        c.close()
    for (s1, s2), r in zip(pairs, res):
        o = opool.cofold2x(TS, s1, s2).result()
        what = "2.x cut %d of %d" % (len(s1), len(s1) + len(s2))
        assert logz_close(r["logZ"][2], o["logZ"]), (what, r["logZ"][2], o["logZ"])
        assert_prob_close(r["hp"], o["hp"], rel=REL, what="hp " + what)


def end_pairs_2x():
    """short strands (vienna2x.pf_duplex is plain Python): N as the strand end and as the neighbour of the last pair at each of the
    four ends -- dxE reads code 0 (unknown neighbour) where a strand that ends there has code 5 (none)"""
    core1, core2 = "GGCAUGCAGGACUAGC", "GCUAGUCCUGCAUGCC"
    out = [(core1, core2)]
    for k in range(4):
        s1, s2 = core1, core2
        if k == 0:
            s1 = "N" + s1
        if k == 1:
            s1 = s1 + "N"
        if k == 2:
            s2 = "N" + s2
        if k == 3:
            s2 = s2 + "N"
        out.append((s1, s2))
        out.append((("N" + core1[1:]) if k == 0 else (core1[:-1] + "N") if k == 1 else core1,
                    ("N" + core2[1:]) if k == 2 else (core2[:-1] + "N") if k == 3 else core2))
    out.append(("N" + core1 + "N", "N" + core2 + "N"))
    return out


@pytest.mark.parametrize("dmode,kernel,hpath", [(1, "dxv_sweep_diag", 2), (0, "dxvl_sweep4<true>", 1)], ids=["log", "linear"])
def test_2x_pf_duplex_with_unknown_strand_ends(hotlib, par_file, dmode, kernel, hpath):
    """pf_duplex under 2.x energies in log space and, with rh_set_duplex_mode(RH_MODE_AUTO), on dxvl_sweep4<true> == vienna2x.pf_duplex"""
    T = v2cases.tables()
    pairs = end_pairs_2x()
    c = context20(par_file)
    try:
        c.set_duplex_mode(dmode)
        c.batch_upload(pairs)
        c.batch_compute()
        assert c.last_hybrid_path() == hpath and c.batch_kernels()[2][0] == kernel, (c.last_hybrid_path(), c.batch_kernels()[2])
        res = [c.batch_results(p) for p in range(len(pairs))]
    finally:
        c.close()
    seen = set()
    for (s1, s2), r in zip(pairs, res):
        efw, ebk, pr = v2.pf_duplex(T, s1, s2)
        what = "2.x pf_duplex %s / %s" % (s1, s2)
        assert abs(efw - ebk) <= 1e-10 * max(1.0, abs(efw)) and logz_close(r["logZ"][2], efw), (what, r["logZ"][2], efw)
        assert_prob_close(r["hp"], pr, rel=REL, what="hp " + what)
        seen.add(round(efw, 9))
    assert len(seen) == len(pairs), "two of the strand-end inputs have the same log Z: an end does not discriminate"


# ---- j. indexed upload
def test_indexed_upload_of_respelled_sequences(hotlib):
    """A 3 x 3 indexed upload whose sequences include two that differ only in case and two that differ only in T / U: distinct
    strings, folded separately; every per-pair output equals the expanded batch's bit for bit, under both models"""
    import ractip_amd
    q = ac.mixed_seqs(33, (41, 70))
    t = ac.mixed_seqs(34, (58, 64))
    seqs = [q[0], q[0].swapcase(), q[1], t[0], t[0].replace("T", "U").replace("t", "u"), t[1]]
    assert len(set(seqs)) == 6 and "T" in t[0].upper()
    index = [(a, 3 + b) for a in range(3) for b in range(3)]
    expanded = [(seqs[i], seqs[j]) for i, j in index]
    for model in (ractip_amd.hot.RH_MODEL_CONTRAFOLD, ractip_amd.hot.RH_MODEL_VIENNA_BL):
        c = ractip_amd.Context(device=0, model=model)
        try:
            c.batch_upload(expanded)
            c.batch_compute()
            want = [c.batch_results(p) for p in range(len(index))]
            c.batch_upload_indexed(seqs, index)
            c.batch_compute()
            assert c.batch_index()[0] == 6
            got = [c.batch_results(p) for p in range(len(index))]
        finally:
            c.close()
        for p, (r, r0) in enumerate(zip(got, want)):
            same_bits(r, r0, ("indexed", model, p))
        same_bits(got[0], got[3], "case only", keys=("bp1", "up1"))       # q[0] and its swapped case: the same fold
        if model == ractip_amd.hot.RH_MODEL_VIENNA_BL:
            same_bits(got[0], got[1], "T / U only", keys=("bp2", "up2", "hp"))
        else:
            assert not np.array_equal(got[0]["bp2"], got[1]["bp2"]), "T is not U under the CONTRAfold model"


# ---- j. helper context: a flagged pair with unknown letters is recomputed on a second context
def helper_batches():
    """(plain, with the chain): the batches of test_vienna_bl_flagged_pairs_are_recomputed_alone (tests/test_gpu_parity.py: the same
    generator in the same state, the same lengths), with N, T and lower-case letters in the 900-letter chain of GC hairpins and in
    its 190-letter partner.  T is U under this model: it goes where the chain has an A, so every stem stays."""
    rng = np.random.default_rng(9)
    comp = {"G": "C", "C": "G"}

    def hairpins(n):
        s = ""
        while len(s) < n:
            stem = "".join(rng.choice(list("GC"), size=10))
            s += stem + "AAAA" + "".join(comp[ch] for ch in reversed(stem)) + "AA"
        return s[:n]
    rnd_ = lambda n: "".join(rng.choice(list("ACGU"), size=n))
    plain = [(rnd_(300), rnd_(260)), (rnd_(150), rnd_(333)), (rnd_(64), rnd_(65)), (rnd_(400), rnd_(90)),
             (rnd_(220), rnd_(210)), (rnd_(900), rnd_(190)), (rnd_(128), rnd_(127)), (rnd_(77), rnd_(300))]
    chain = list(hairpins(900))
    for k in range(0, 900, 26):          # one hairpin of 26 letters: 10 + AAAA + 10 + AA
        if k + 26 <= 900:
            assert "".join(chain[k + 10:k + 14]) == "AAAA" and "".join(chain[k + 24:k + 26]) == "AA"
    chain[11] = "N"                       # a hairpin letter
    chain[26 * 7 + 24] = "N"              # between two hairpins
    chain[26 * 12 + 3] = "N"              # inside a stem: that pair is gone
    chain[26 * 20 + 12] = "T"             # a hairpin letter, read as U
    chain[26 * 30 + 25] = "X"
    for k in (5, 26 * 3 + 17, 26 * 15 + 11, 26 * 25 + 2, 899):
        chain[k] = chain[k].lower()
    partner = list(plain[5][1])
    partner[0], partner[63], partner[64], partner[189] = "N", "n", "T", "N"
    for k in range(20, 40):
        partner[k] = partner[k].lower()
    mixed = list(plain)
    mixed[5] = ("".join(chain), "".join(partner))
    return plain, mixed


def run_helper_batch(pairs, env):
    with tve.switches(env, clear=("RH_PAIR_HELPER",)):
        c = tve.vcontext(0, hybrid=True)
    try:
        c.batch_upload(pairs)
        c.batch_compute()
        return c.last_path(), sorted(c.batch_fallbacks(2) + c.batch_fallbacks(0)), [c.batch_results(p) for p in range(len(pairs))]
    finally:
        c.close()


@pytest.fixture(scope="module")
def helper_oracle(opool):
    """the 900-letter fold and the 1090-letter two-molecule ensemble take the CPU restatement many seconds: the opool fixture queued
    them when the module's first test started (the calls are memoised: these are the same futures)"""
    s1, s2 = helper_batches()[1][5]
    return opool.mccaskill(s1), opool.mccaskill(s2), opool.cofold(s1, s2)


def test_flagged_pair_with_unknown_letters_is_recomputed_on_the_helper_context(hotlib, helper_oracle):
    """recompute_pairs_on_helper (fallbacks.hip) writes the flagged pair back as text from its codes ("NACGU"[code]), stages it on a
    second context with its own tables and copies bp, up, hp and log Z back at this batch's strides: the pair that holds the chain
    is the only one flagged (rh_last_path = 3), it has the bits of the same pair computed alone, every other pair keeps the bits of a
    batch without the chain, and the recomputed pair == oracle/vienna_oracle.c (PARITY UNPINNED against ViennaRNA)"""
    plain, mixed = helper_batches()
    s1, s2 = mixed[5]
    assert len(s1) == 900 and len(s2) == 190 and {"N", "T", "X"} <= set(s1) and s1 != s1.upper() and {"N", "n", "T"} <= set(s2)
    path0, _, base = run_helper_batch(plain, {})
    assert path0 == 1
    path, flagged, res = run_helper_batch(mixed, {"RH_PAIR_HELPER": "2"})
    assert path == 3 and flagged == [10, 11], (path, flagged)      # sequences 10 and 11: the one pair, on the helper
    for p in range(len(plain)):
        if p != 5:
            same_bits(res[p], base[p], "pair %d beside the recomputed one" % p)
    path1, flagged1, alone = run_helper_batch([mixed[5]], {})
    print("the pair alone: rh_last_path %d, flagged %r; equal bits: %r"
          % (path1, flagged1, {k: bool(np.array_equal(res[5][k], alone[0][k])) for k in KEYS}))
    same_bits(res[5], alone[0], "the recomputed pair against the same pair alone")
    o1, o2, oc = (f.result() for f in helper_oracle)
    r = res[5]
    for q, (o, key, ukey) in enumerate(((o1, "bp1", "up1"), (o2, "bp2", "up2"))):
        assert logz_close(r["logZ"][q], o["logZ"]), (q, r["logZ"][q], o["logZ"])
        assert_prob_close(r[key], o["post"], rel=REL, what="%s of the recomputed pair" % key)
        assert_prob_close(r[ukey], o["up"], rel=REL, abs_floor=1e-11, what="%s of the recomputed pair" % ukey)
    assert logz_close(r["logZ"][2], oc["logZ"]), (r["logZ"][2], oc["logZ"])
    assert_prob_close(r["hp"], oc["hp"], rel=REL, what="hp of the recomputed pair")
    for k, ch in enumerate(s1):
        if ch in "NX":
            assert r["up1"][k, 0] > 1 - 1e-12 and r["hp"][k + 1].max() == 0, k
