"""GPU suite (-m gpu): structure constraints on the batched, device-resident interface -- rh_batch_upload_constrained, the mask
kernel behind it (ractip_amd/csrc/allow_mask.hip), and the callers above it (hot.Context.batch_upload, ProbabilityEngine::
solve_probabilities_default with structure lines).

The masks are compared byte for byte with tests/_oracle.py:constraint_mask, the numpy restatement of ViennaRNA-1.8 make_ptypes under
fold_constrained that clears rectangles; the product evaluates a closed form per cell.  Probabilities go against
oracle/vienna_oracle.c under that numpy mask (PARITY UNPINNED against ViennaRNA, pinned to enumeration on short inputs).
Tolerances are the project's: REL = 1e-6 on bp and hp, REL with abs_floor = 1e-11 on up, 1e-9 relative on log Z, 1e-10 between
two organisations of the same arithmetic, the same bits where nothing but the route of the mask changed.

The mask kernel's tile is 64 rows, so the lengths 63 / 64 / 65 of the ragged batch are its tile edges."""
import os
import subprocess

import numpy as np
import pytest

from _oracle import OraclePool, assert_prob_close, constraint_mask, threshold_scans, tri_offset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ractip_amd", "host", "prob_cli")
REL = 1e-6
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")
MODES = [("auto", 0, 1), ("log", 1, 2)]   # name, rh_set_mode, the rh_last_path it must report
MODE_IDS = [m[0] for m in MODES]
SCANS = ((0, 0.5), (1, 0.5), (2, 0.1), (3, 0.003), (4, 0.003))   # which, threshold: the reference's defaults

S1_LENS = (65, 1, 2, 64, 31)
S2_LENS = (64, 63, 31, 65, 1)
# One constraint per sequence, in upload order (s1, s2 of pair 0, s1, s2 of pair 1, ...).  Between them: every class character,
# nesting three deep and two sibling brackets inside one parent (65), a bracket at letters 1 and n (65, 64), '<' next to '(',
# a string shorter than its sequence (the first 64), an empty string (63) and a None entry (the first 31).
FOLD_CONS = (
    "(.((.((...)).(...).)).x.|.<(...)>..<<..>>" + "." * 23 + ")",      # 65
    "<<<(((....)))>>>xxx|.(..).",                                      # 64, shorter than the sequence
    "x",                                                               # 1
    "",                                                                # 63
    "<>",                                                              # 2
    None,                                                              # 31
    "(" + "(...).(....).x" + "." * 48 + ")",                           # 64
    "..<(....)..|..xx..>>.." + "." * 20 + "((((...))))" + "." * 12,    # 65
    "((((...))))....x....<...>......",                                 # 31
    ".",                                                               # 1
)


def rnd(rng, n):
    return "".join(rng.choice(list("ACGU"), n))


def matched(cons):
    """(i, j) of every matched bracket pair, 0-based"""
    stack, out = [], []
    for k, ch in enumerate(cons or ""):
        if ch == "(":
            stack.append(k)
        elif ch == ")":
            out.append((stack.pop(), k))
    assert not stack
    return out


def ragged_batch(extra=()):
    """The pairs, their per-sequence constraints and their joint constraints.  Forced pairs are G-C.  Joint strings: two forced
    pairs across the cut and 'x' on both sides of it where the lengths allow, one forced pair for (1, 63), None for (2, 31) and a
    string shorter than s1+s2 for (31, 1)."""
    rng = np.random.RandomState(271)
    lens = list(zip(S1_LENS, S2_LENS)) + list(extra)
    cons = list(FOLD_CONS)
    for a, b in extra:   # long sequences: a forced pair far apart, a run of 'x' across a tile edge of the mask kernel, '<' '|' '>'
        for n in (a, b):
            c = list("." * n)
            c[2], c[n - 3] = "(", ")"
            c[60:68] = "x" * 8
            c[n // 2: n // 2 + 3] = "<|>"
            cons.append("".join(c))
    seqs = []
    for k, n in enumerate(x for pr in lens for x in pr):
        s = list(rnd(rng, n))
        assert cons[k] is None or len(cons[k]) <= n
        for i, j in matched(cons[k]):
            s[i], s[j] = "G", "C"
        seqs.append(s)
    joint = []
    for p, (a, b) in enumerate(lens):
        s1, s2 = seqs[2 * p], seqs[2 * p + 1]
        free1 = [i for i in range(a) if (cons[2 * p] or "")[i:i + 1] not in ("(", ")")]      # letters no fold constraint made G or C
        free2 = [j for j in range(b) if (cons[2 * p + 1] or "")[j:j + 1] not in ("(", ")")]
        c = list("." * (a + b))
        if (a, b) == (2, 31):
            joint.append(None)
            continue
        if (a, b) == (31, 1):
            joint.append("x.x")          # shorter than s1+s2
            continue
        k = 2 if min(len(free1), len(free2)) >= 6 else 1
        for t in range(k):               # s1's free letters t-th from the left with s2's t-th from the right: nested across the cut
            i, j = free1[t], free2[-1 - t]
            s1[i], s2[j] = "G", "C"
            c[i], c[a + j] = "(", ")"
        if k == 2:
            c[free1[-1]] = c[free1[-2]] = "x"      # 'x' on both sides of the cut
            c[a + free2[0]] = c[a + free2[1]] = "x"
        joint.append("".join(c))
    pairs = [("".join(seqs[2 * p]), "".join(seqs[2 * p + 1])) for p in range(len(lens))]
    return pairs, [(cons[2 * p], cons[2 * p + 1]) for p in range(len(lens))], joint


def vcontext(mode=0, hybrid=False, max_w=None, model=None):
    import ractip_amd
    c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL if model is None else model)
    try:
        c.set_mode(mode)
        if hybrid:
            c.set_hybrid(True)
        if max_w is not None:
            c.set_max_w(max_w)
    except Exception:
        c.close()
        raise
    return c


def run(c, pairs, cons=None, joint=None):
    c.batch_upload(pairs, constraints=cons, co_constraints=joint)
    c.batch_compute()
    return [c.batch_results(p) for p in range(len(pairs))]


def assert_same_bits(res, ref, what):
    assert len(res) == len(ref)
    for p, (r, r0) in enumerate(zip(res, ref)):
        for k in KEYS:
            assert np.array_equal(np.asarray(r[k]), np.asarray(r0[k])), (what, p, k)


def logz_close(z, ref):
    return abs(z - ref) <= 1e-9 * max(1.0, abs(ref))


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    yield p
    p.close()


def expected_image(cons, n, ld):
    want = np.zeros((ld, ld), dtype=np.uint8)
    want[:n + 1, :n + 1] = constraint_mask(cons or "", n)
    return want


# ---- 1. the bytes the kernel writes
def test_mask_bytes_of_a_ragged_batch(hotlib):
    pairs, cons, joint = ragged_batch()
    c = vcontext(hybrid=True)
    try:
        c.batch_upload(pairs)
        assert c.debug_allow_mask(0, 0) is None and c.debug_allow_mask(1, 0) is None      # a batch without constraints: no mask
        c.batch_upload(pairs, constraints=cons, co_constraints=joint)
        seen = set()
        for p, (s1, s2) in enumerate(pairs):
            for q, s in enumerate((s1, s2)):
                m = c.debug_allow_mask(0, 2 * p + q)
                n, ld = len(s), m.shape[0]
                assert m.shape == (ld, ld) and ld >= max(S1_LENS + S2_LENS) + 2
                assert np.array_equal(m, expected_image(cons[p][q], n, ld)), ("sequence", 2 * p + q, cons[p][q])
                seen |= set(cons[p][q] or "")
            m = c.debug_allow_mask(1, p)
            n, ld = len(s1) + len(s2), m.shape[0]
            assert ld >= max(a + b for a, b in zip(S1_LENS, S2_LENS)) + 2
            assert np.array_equal(m, expected_image(joint[p], n, ld)), ("pair", p, joint[p])
        assert seen >= set("x()<>|.")
        # what the joint strings hold: two forced pairs across the cut and 'x' on both sides of it
        a = len(pairs[0][0])
        assert joint[0][:a].count("(") == 2 and joint[0][a:].count(")") == 2 and "x" in joint[0][:a] and "x" in joint[0][a:]
        # a constrained batch under pf_duplex: the joint strings are checked and not staged
        c.set_hybrid(False)
        c.batch_upload(pairs, constraints=cons, co_constraints=joint)
        assert c.debug_allow_mask(0, 0) is not None and c.debug_allow_mask(1, 0) is None
    finally:
        c.close()


# ---- 2. a constrained batch against the CPU restatement
PARITY_EXTRA = ((257, 130),)
BINDING_FOLDS = (0, 1, 6, 7, 8, 10, 11)   # sequences whose constraint holds a forced pair or a run of 'x' in 31 letters or more
BINDING_PAIRS = (0, 3, 5)                 # pairs whose joint string forces two pairs across the cut


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_constrained_batch_vs_cpu_restatement(hotlib, opool, name, mode, path):
    pairs, cons, joint = ragged_batch(PARITY_EXTRA)
    for s1, s2 in pairs:
        opool.mccaskill(s1), opool.mccaskill(s2), opool.cofold(s1, s2)
    c = vcontext(mode, hybrid=True)
    try:
        assert c.max_w == 15
        res = run(c, pairs, cons, joint)
        assert c.last_path() == path, (c.last_path(), path)
    finally:
        c.close()
    for p, ((s1, s2), r) in enumerate(zip(pairs, res)):
        for q, (s, key, ukey) in enumerate(((s1, "bp1", "up1"), (s2, "bp2", "up2"))):
            k, n, cs = 2 * p + q, len(s), cons[p][q]
            free = opool.mccaskill(s).result()
            o = free if cs is None else opool.constrained("mccaskill", s, 15, constraint=cs)
            w = "%s sequence %d n=%d" % (name, k, n)
            print("%s: logZ %.12g oracle %.12g unconstrained %.12g" % (w, r["logZ"][q], o["logZ"], free["logZ"]))
            if n <= 20 and cs is not None:   # the restatement under this mask is itself pinned to enumeration
                b = opool.vo.fold_bruteforce(s, max_w=15, constraint=cs)
                assert abs(o["logZ"] - b["logZ"]) < 1e-11 and np.abs(o["post"] - b["post"]).max() < 1e-11 and np.abs(o["up"] - b["up"]).max() < 1e-11
            assert logz_close(r["logZ"][q], o["logZ"]), (w, r["logZ"][q], o["logZ"])
            assert_prob_close(r[key], o["post"], rel=REL, what="bp " + w)
            assert_prob_close(r[ukey], o["up"], rel=REL, abs_floor=1e-11, what="up " + w)
            if k in BINDING_FOLDS:
                assert abs(r["logZ"][q] - free["logZ"]) > 1e-3 and abs(o["logZ"] - free["logZ"]) > 1e-3, (w, "the constraint does not bind")
            for i, ch in enumerate(cs or ""):
                if ch == "x":
                    assert r[ukey][i, 0] > 1 - 1e-12, (w, i)                 # 'x' letters are unpaired
            for i, j in matched(cs):                                         # a forced letter pairs with its partner or nothing
                row = tri_offset(n, i + 1)
                assert r[key][row + i + 2:row + n + 1].sum() == r[key][row + j + 1], (w, i, j)
        cj = joint[p]
        free = opool.cofold(s1, s2).result()
        o = free if cj is None else opool.constrained("cofold", s1, s2, constraint=cj)
        w = "%s pair %d (%d, %d)" % (name, p, len(s1), len(s2))
        print("%s: logZ %.12g oracle %.12g unconstrained %.12g" % (w, r["logZ"][2], o["logZ"], free["logZ"]))
        if len(s1) + len(s2) <= 20 and cj is not None:
            b = opool.vo.cofold(s1, s2, bruteforce=True, constraint=cj)
            assert abs(o["logZ"] - b["logZ"]) < 1e-11 and np.abs(o["post"] - b["post"]).max() < 1e-11
        assert logz_close(r["logZ"][2], o["logZ"]), (w, r["logZ"][2], o["logZ"])
        assert_prob_close(r["hp"], o["hp"], rel=REL, what="hp " + w)
        if p in BINDING_PAIRS:
            assert abs(r["logZ"][2] - free["logZ"]) > 1e-3 and abs(o["logZ"] - free["logZ"]) > 1e-3, (w, "the joint constraint does not bind")
        for i, ch in enumerate((cj or "")[:len(s1)]):
            if ch == "x":
                assert r["hp"][i + 1].max() == 0, (w, i)                     # hp rows of 'x' letters are 0
        for j, ch in enumerate((cj or "")[len(s1):]):
            if ch == "x":
                assert r["hp"][:, j + 1].max() == 0, (w, j)


# ---- 3. the single-problem entry points kept their bits when the host builder went
def test_single_problem_results_did_not_move(hotlib):
    """rh_fold_constrained and rh_cofold_constrained on the constraint cases of test_vienna_bl_structure_constraints, of
    test_vienna_bl_constrained_two_molecule_ensemble and of constraint_cases() in test_gpu_vienna_edges.py (n = 400): the arrays
    recorded on an MI355X from the commit before the masks moved to the device (tests/golden/constrained_single_parent.npz: inputs
    and float64 results of a default-mode Vienna-BL context, width 15; the n = 400 bp tables as (index, value) of their cells
    that are not +0.0)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "constrained_single_parent.npz"), allow_pickle=False)
    nf = len([k for k in g.files if k.startswith("fold/") and k.endswith("/seq")])
    nc = len([k for k in g.files if k.startswith("cofold/") and k.endswith("/cons")])
    assert nf == 13 and nc == 6
    c = vcontext()
    try:
        for k in range(nf):
            seq, cons = str(g["fold/%d/seq" % k]), str(g["fold/%d/cons" % k])
            bp, up, z = c.fold(seq, constraint=cons)
            if "fold/%d/bp" % k in g.files:
                want = g["fold/%d/bp" % k]
            else:
                want = np.zeros(len(bp))
                want[g["fold/%d/bp_idx" % k]] = g["fold/%d/bp_val" % k]
                assert not np.signbit(bp[bp == 0]).any()
            assert np.array_equal(bp, want), ("bp", k, cons[:40])
            assert np.array_equal(up, g["fold/%d/up" % k]), ("up", k, cons[:40])
            assert z == float(g["fold/%d/logZ" % k]), ("logZ", k, cons[:40])
        for k in range(nc):
            s1, s2, cons = str(g["cofold/%d/s1" % k]), str(g["cofold/%d/s2" % k]), str(g["cofold/%d/cons" % k])
            hp, z = c.cofold(s1, s2, constraint=cons)
            assert np.array_equal(hp, g["cofold/%d/hp" % k]), ("hp", k, cons[:40])
            assert z == float(g["cofold/%d/logZ" % k]), ("cofold logZ", k, cons[:40])
    finally:
        c.close()


# ---- 4. nothing lingers
def test_constrained_and_unconstrained_uploads_alternate_without_traces(hotlib):
    """One context: a longer constrained batch, then the ragged batch constrained, unconstrained and constrained again.  A stale
    mask, a stale graph key (the graphs key on the mask pointer through their argument) or padding left over from the longer batch
    would change a bit against fresh contexts."""
    big, big_cons, big_joint = ragged_batch(PARITY_EXTRA)
    pairs, cons, joint = ragged_batch()
    c = vcontext(hybrid=True)
    try:
        run(c, big, big_cons, big_joint)
        first = run(c, pairs, cons, joint)
        middle = run(c, pairs)
        assert c.debug_allow_mask(0, 0) is None and c.debug_allow_mask(1, 0) is None
        third = run(c, pairs, cons, joint)
    finally:
        c.close()
    fresh = []
    for kw in ({}, dict(cons=cons, joint=joint)):
        c = vcontext(hybrid=True)
        try:
            fresh.append(run(c, pairs, **kw))
        finally:
            c.close()
    assert_same_bits(middle, fresh[0], "unconstrained after constrained vs a fresh context")
    assert_same_bits(third, first, "constrained again vs the first constrained compute")
    assert_same_bits(first, fresh[1], "constrained after a longer batch vs a fresh context")
    assert any(not np.array_equal(a["bp1"], b["bp1"]) for a, b in zip(first, middle))


# ---- 5. which ensemble the joint string reaches
def test_joint_constraint_follows_the_hybrid_source(hotlib):
    pairs, cons, joint = ragged_batch()
    c = vcontext()
    try:
        with_j = run(c, pairs, cons, joint)
        without = run(c, pairs, cons)
        for p in range(len(pairs)):        # pf_duplex takes no constraint (src/ractip.cpp:390-398)
            assert np.array_equal(with_j[p]["hp"], without[p]["hp"]) and with_j[p]["logZ"][2] == without[p]["logZ"][2], p
        c.set_hybrid(True)
        co_j = run(c, pairs, cons, joint)
        co_free = run(c, pairs, cons)
        for p, (s1, s2) in enumerate(pairs):
            if joint[p] is None:
                assert np.array_equal(co_j[p]["hp"], co_free[p]["hp"]), p
                continue
            if p in BINDING_PAIRS:
                assert np.abs(co_j[p]["hp"] - co_free[p]["hp"]).max() > 1e-6, p
            hp, z = c.cofold(s1, s2, constraint=joint[p])   # the single call may plan its sweeps differently: 1e-10, not bits
            c.set_hybrid(True)
            assert np.abs(co_j[p]["hp"] - hp).max() <= 1e-10 and abs(co_j[p]["logZ"][2] - z) <= 1e-10 * max(1.0, abs(z)), p
    finally:
        c.close()


# ---- 6. rejected uploads
def test_rejected_constraints_name_the_problem_and_leave_the_context_usable(hotlib):
    import ractip_amd
    pairs, cons, joint = ragged_batch()
    c = vcontext(hybrid=True)
    try:
        good = run(c, pairs, cons, joint)
        bad = list(cons)
        bad[2] = ("<>", "..((..")                     # entry 3 of 5: sequence 5
        with pytest.raises(ractip_amd.RhError, match=r"sequence 5: unbalanced '\('"):
            c.batch_upload(pairs, constraints=bad, co_constraints=joint)
        bad[2] = ("<>", "..)")
        with pytest.raises(ractip_amd.RhError, match=r"sequence 5: unbalanced '\)'"):
            c.batch_upload(pairs, constraints=bad, co_constraints=joint)
        gg = [("GAAG", "GGGAAACCC"), ("GGGAAACCC", "GAAG")]
        with pytest.raises(ractip_amd.RhError, match=r"sequence 3: a forced pair of non-complementary letters"):
            c.batch_upload(gg, constraints=[(None, "(((...)))"), ("(((...)))", "(..)")])
        with pytest.raises(ractip_amd.RhError, match=r"pair 1: a forced pair of non-complementary letters"):
            c.batch_upload(gg, co_constraints=[None, "(" + "." * 11 + ")"])      # G of s1 with G of s2
        with pytest.raises(ractip_amd.RhError, match="5 pairs"):
            c.batch_upload(pairs, constraints=cons[:2])
        assert_same_bits(run(c, pairs, cons, joint), good, "after rejected uploads")
    finally:
        c.close()
    cf = vcontext(model=ractip_amd.hot.RH_MODEL_CONTRAFOLD)
    try:
        before = run(cf, pairs)
        with pytest.raises(ractip_amd.RhError, match="Vienna-BL model only"):
            cf.batch_upload(pairs, co_constraints=joint)
        with pytest.raises(ractip_amd.RhError, match="Vienna-BL model only"):
            cf.batch_upload(pairs, constraints=cons)
        assert_same_bits(run(cf, pairs, [None] * len(pairs), [None] * len(pairs)), before, "CONTRAfold model after rejected uploads")
    finally:
        cf.close()


# ---- 7. the device scans on a constrained batch
def test_candidates_of_a_constrained_batch(hotlib):
    pairs, cons, joint = ragged_batch()
    c = vcontext(hybrid=True, max_w=1)
    try:
        res = run(c, pairs, cons, joint)
        found = 0
        for which, th in SCANS:
            rec, first = c.batch_candidates_all(which, th)
            assert len(first) == len(pairs) + 1 and first[0] == 0 and first[-1] == len(rec)
            for p in range(len(pairs)):
                i, j, pr = threshold_scans(res[p], (which, th))
                mine = rec[first[p]:first[p + 1]]
                assert len(mine) == len(i), (which, p)
                assert np.array_equal(mine["i"], i) and np.array_equal(mine["j"], j) and np.array_equal(mine["p"], pr), (which, p)
            found += len(rec)
        assert found > 0
    finally:
        c.close()


# ---- 8. the C++ adapter
@pytest.fixture(scope="module")
def cli(hotlib):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ractip_amd", "host")])
    return CLI


def cli_lines(cli, *args):
    out = subprocess.run([cli] + list(args), check=True, capture_output=True, text=True).stdout.split("\n")
    return [l for l in out if l]


def take(lines, pos, tag):
    hdr = lines[pos].split()
    assert hdr[0] == tag, (hdr, tag)
    dims = [int(x) for x in hdr[1:]]
    cnt = int(np.prod(dims))
    vals = np.array([float(x) for x in lines[pos + 1:pos + 1 + cnt]])
    return vals.reshape(dims) if len(dims) > 1 else vals, pos + 1 + cnt


def test_host_adapter_batch_with_structure_lines(cli):
    """solve_probabilities_default(pairs, structures, ...) == the per-problem members rnafold(seq, str, ...) and
    rnaduplex_cofold(seq1, str1, seq2, str2, ...) on RactIP-style structure lines ('[' ']' 'e' '(' ')' 'x' 'l'), to 1e-10 on the
    float matrices both return (two routes to the same arithmetic)."""
    rng = np.random.RandomState(8)
    lines_in = [("..[[[....(((....)))..eee..xx....ll...", "..((...))....]]]...x..e....l.."),
                ("[[..((...))..x", "l..]]....(...)..e."),
                ("...(((...)))...eee......", "")]
    problems = []
    for t1, t2 in lines_in:
        n1, n2 = len(t1) + 3, max(len(t2), 9) + 2
        s1, s2 = list(rnd(rng, n1)), list(rnd(rng, n2))
        for s, t in ((s1, t1), (s2, t2)):
            for i, j in matched(t):
                s[i], s[j] = "G", "C"
        o1 = [k for k, ch in enumerate(t1) if ch == "["]
        o2 = [k for k, ch in enumerate(t2) if ch == "]"]
        assert len(o1) == len(o2)
        for i, j in zip(o1, reversed(o2)):
            s1[i], s2[j] = "G", "C"
        problems.append(("".join(s1), t1, "".join(s2), t2))
    lines = cli_lines(cli, "solve_default_c", "7", *[x if x else "." for pr in problems for x in pr])
    pos = 0
    for s1, t1, s2, t2 in problems:
        t2 = t2 if t2 else "."
        assert lines[pos].split()[0] == "pair"
        bp, pos = take(lines, pos + 1, "bp")
        up, pos = take(lines, pos, "up")
        hp, pos = take(lines, pos, "hp")
        one = cli_lines(cli, "rnafold", s1, "7", t1)
        _, q = take(one, 0, "offset")
        bp1, q = take(one, q, "bp")
        two = cli_lines(cli, "rnafold", s2, "7", t2)
        _, q = take(two, 0, "offset")
        _, q = take(two, q, "bp")
        up2, q = take(two, q, "up")
        hp1, _ = take(cli_lines(cli, "cofold", s1, s2, t1, t2), 0, "hp")
        assert np.abs(bp - bp1).max() <= 1e-10 and np.abs(up - up2).max() <= 1e-10 and np.abs(hp - hp1).max() <= 1e-10, (t1, t2)
        assert bp.max() > 0.5 and (hp.max() > 0.1 or "[" not in t1)
