"""CPU tests (no GPU) that pin oracle/vienna2x_oracle.c, the polynomial-time restatement of pf_fold / pf_unstru / co_pf_fold under
the ViennaRNA-2.x energy functions with dangles = 2, to oracle/vienna2x.py: its interior-loop energy to E_IntLoop, its partition
function, pair probabilities and accessibilities to enumeration of every structure (brute_fold / brute_cofold), on the loop classes
that enumeration reaches only on sparse-pairable inputs.  PARITY UNPINNED against ViennaRNA (absent).  They also prove, on the
restatement alone, that the inputs of tests/test_gpu_vienna2x_edges.py exercise what they are meant to."""
import math

import numpy as np
import pytest

import _vienna2x_cases as cases
from _oracle import OraclePool, Vienna2xOracle, constraint_mask, tri_offset
from _vienna2x_cases import v2

REL = 1e-9   # log Z, as in tests/test_gpu_vienna2x.py


@pytest.fixture(scope="module")
def T():
    return cases.tables()


@pytest.fixture(scope="module")
def oracle(T):
    return Vienna2xOracle(T)


@pytest.fixture(scope="module")
def opool(T):
    p = OraclePool()
    p.tables2x(cases.TABLES, T)
    yield p
    p.close()


def test_interior_loop_energy_equals_E_IntLoop(T, oracle):
    """all 496 shapes with l1 + l2 <= 30, every pair of pair types, seeded neighbour letters with the unknown letter (code 0) among
    them: integer energies, exact equality"""
    rng = np.random.default_rng(496)
    shapes = [(a, b) for a in range(31) for b in range(31 - a)]
    assert len(shapes) == 496
    checked = 0
    for n1, n2 in shapes:
        for t in range(1, 7):
            for t2 in range(1, 7):
                letters = [tuple(rng.integers(0, 5, 4)) for _ in range(3)] + [(0, 0, 0, 0), tuple(rng.integers(1, 5, 4))]
                for si1, sj1, sp1, sq1 in letters:
                    want = v2.E_IntLoop(T, n1, n2, t, t2, si1, sj1, sp1, sq1)
                    got = oracle.int_loop(n1, n2, t, t2, int(si1), int(sj1), int(sp1), int(sq1))
                    assert got == want, (n1, n2, t, t2, si1, sj1, sp1, sq1, got, want)
                    checked += 1
    assert checked == 496 * 36 * 5


def dense(bp, n):
    want = np.zeros((n + 1) * (n + 2) // 2)
    for (i, j), p in bp.items():
        want[tri_offset(n, i) + j] = p
    return want


def check_fold(T, oracle, s, constraint=None):
    """the restatement against enumeration at the bars of tests/test_gpu_vienna2x.py; returns enumeration's pair probabilities"""
    n = len(s)
    allow = constraint_mask(constraint, n) if constraint is not None else None
    lz, bp, up = v2.brute_fold(T, s, max_w=4, allow=allow)
    r = oracle.fold(s, 4, constraint)
    assert r["logZ"] == pytest.approx(lz, rel=REL, abs=1e-9), s
    assert r["logZ_out"] == pytest.approx(lz, rel=REL, abs=1e-9), s
    want = dense(bp, n)
    assert np.allclose(r["post"], want, rtol=1e-8, atol=1e-12), (s, np.abs(r["post"] - want).max())
    assert np.allclose(r["up"], up, rtol=1e-8, atol=1e-11), (s, np.abs(r["up"] - up).max())
    return bp


def check_cofold(T, oracle, s1, s2, constraint=None):
    allow = constraint_mask(constraint, len(s1) + len(s2)) if constraint is not None else None
    lz, hp = v2.brute_cofold(T, s1, s2, allow=allow)
    r = oracle.cofold(s1, s2, constraint)
    assert r["logZ"] == pytest.approx(lz, rel=REL, abs=1e-9), (s1, s2)
    assert r["logZ_out"] == pytest.approx(lz, rel=REL, abs=1e-9), (s1, s2)
    assert np.allclose(r["hp"], hp, rtol=1e-8, atol=1e-12), (s1, s2, np.abs(r["hp"] - hp).max())
    return hp


def test_the_sequences_of_the_gpu_2x_suite_equal_enumeration(T, oracle):
    rng = np.random.default_rng(13)
    seqs = [cases.rnd(rng, n) for n in (8, 10, 11, 12, 13)]
    seqs += ["GGGGGACUCC", "ACAACGUAGC", "GACAGUACUC", "GGACUUCGGUCAAGCC", "GCGAAGCGAAGCGC"]
    for s in seqs:
        check_fold(T, oracle, s)
    rng = np.random.default_rng(17)
    pairs = [(cases.rnd(rng, a), cases.rnd(rng, b)) for a, b in ((5, 6), (7, 5), (4, 8), (6, 7))] + [("GGGAC", "GUCCC"), ("GGCGAAAGCC", "GGC")]
    for s1, s2 in pairs:
        check_cofold(T, oracle, s1, s2)


def test_seeded_random_sequences_equal_enumeration(T, oracle):
    rng = np.random.default_rng(814)
    for n in (8, 9, 10, 11, 12, 13, 14, 14):
        check_fold(T, oracle, cases.rnd(rng, n))
    for n1, n2 in ((1, 9), (9, 1), (6, 7), (3, 10), (8, 5), (4, 4)):
        check_cofold(T, oracle, cases.rnd(rng, n1), cases.rnd(rng, n2))


def small(l1, l2, middle="AAAA"):
    """the planted construction with 2-bp stems: enumeration stays at hundreds of structures"""
    return cases.planted(l1, l2, outer=2, inner=2, pad=1, middle=middle)


def loop_is_present(bp, s, p, q, l1, l2):
    """the enclosed pair and the pair l1 / l2 letters outside it both have positive probability"""
    return bp.get((p, q), 0.0) > 0 and bp.get((p - l1 - 1, q + l2 + 1), 0.0) > 0


@pytest.mark.parametrize("l1,l2,fits", [(29, 0, True), (30, 0, True), (31, 0, False), (0, 29, True), (0, 30, True), (0, 31, False),
                                        (1, 28, True), (1, 29, True), (1, 30, False), (28, 1, True), (29, 1, True), (30, 1, False),
                                        (2, 3, True), (3, 2, True), (14, 16, True), (15, 16, False)])
def test_sparse_pairable_loops_equal_enumeration(T, oracle, l1, l2, fits):
    """bulges of 29 / 30 / 31, 1xn loops at n = 28 / 29 / 30, 2x3 and 3x2, generic 14x16 and 15x16: a loop over the budget of 30 has no
    single-loop term, so its two stems never occur together: enumeration drops the structures that hold both pairs (there are
    some), and a restatement that gave the loop a weight would miss log Z and both pairs' probabilities"""
    s, p, q = small(l1, l2)
    bp = check_fold(T, oracle, s)
    i, j = p - l1 - 1, q + l2 + 1
    n = len(s)
    S = v2.encode(s)
    both = sum(1 for st in v2.structures(n, S) if (p, q) in st and (i, j) in st)
    assert both > 0 and loop_is_present(bp, s, p, q, l1, l2)
    assert fits == ((l1 + l2) <= v2.MAXLOOP)


SPARSE_FOLDS = {
    "triloop CAACG inside a stem": "AAGCAACGCAA",
    "triloop GUUAC inside a stem": "ACGUUACGA",
    "tetraloop GGGGAC inside a stem": "AAGGGGGACCAA",
    "tetraloop CGAAAG inside a stem": "AGCGAAAGCA",
    "hexaloop CCGAGAGG inside a stem": "AAGCCGAGAGGCAA",
    "hexaloop ACAGUACU inside a stem": "AGACAGUACUCA",
    "hairpin of 33 letters (lxc branch)": "AGG" + "A" * 33 + "CCA",
    "hairpin of 31 letters (lxc branch)": "GG" + "A" * 31 + "CC",
    "three-branch multiloop, unpaired letters before, between and after": "AGGA" + "GAAAAC" + "AA" + "GAAAC" + "A" + "GGAAAACC" + "AAA" + "CCA",
    "unknown letters next to the stem ends": "ANGGAAAACCNA",
    "unknown letters inside the loops": "GNGANAACAC",
    "unknown letters next to an interior loop": "GGNAGGAAAACCANCC",
}


@pytest.mark.parametrize("what", sorted(SPARSE_FOLDS))
def test_sparse_pairable_folds_equal_enumeration(T, oracle, what):
    s = SPARSE_FOLDS[what]
    bp = check_fold(T, oracle, s)
    assert bp, what
    if "loop " in what and "inside a stem" in what:   # the tabulated loop's own pair and the pair around it occur together
        key = what.split()[1]
        a = s.index(key) + 1
        assert bp.get((a, a + len(key) - 1), 0) > 0 and bp.get((a - 1, a + len(key)), 0) > 0 and key in T[what.split()[0].capitalize() + "s"]
    if "multiloop" in what:
        S = v2.encode(s)
        branches = [(5, 10), (13, 17), (19, 26)]
        assert any(all(b in st for b in branches + [(3, 30)]) for st in v2.structures(len(s), S)), "no three-branch multiloop"


def test_sparse_pairable_cofolds_equal_enumeration(T, oracle):
    """the gap loop holds two stems (one on each strand) under a pair across the cut; a cut next to a stem end; unknown letters"""
    hp = check_cofold(T, oracle, "AGGAGAAAACA", "AGAAAACACCA")
    assert hp[2, 10] > 0 and hp[3, 9] > 0
    check_cofold(T, oracle, "GGAAG", "CAAACC")
    check_cofold(T, oracle, "GGNA", "ANCC")
    check_cofold(T, oracle, "G" + "A" * 33, "C")          # a pair of span 34 across the cut: no loop-size rule, no hairpin term
    check_cofold(T, oracle, "GG" + "A" * 31 + "GG", "AAAACCCC")


def test_an_allowed_pair_mask_equals_enumeration_under_the_same_mask(T, oracle):
    """an 'x' run and a forced pair: enumeration keeps the structures whose pairs all pass constraint_mask"""
    s = "AGGAGAAAACAAGGAAACCACCA"
    cons = "..(.xxxx..........)...."
    assert len(cons) == len(s)
    free = check_fold(T, oracle, s)
    masked = check_fold(T, oracle, s, cons)
    assert masked.get((3, 19), 0) > 0 and (5, 10) in free and (5, 10) not in masked
    assert all(not (4 < i <= 8 or 4 < j <= 8) for (i, j) in masked)
    s1, s2 = "AGGAGAAAACA", "AGAAAACACCA"
    cons = "..(.x......" + "........)x."
    hp = check_cofold(T, oracle, s1, s2, cons)
    assert hp[3, 9] > 0 and hp[3].sum() == pytest.approx(hp[3, 9]) and hp[2].sum() == 0 and hp[:, 10].sum() == 0


@pytest.mark.parametrize("n", (300, 520))
def test_self_consistency_at_length(opool, n):
    """inside log Z == outside log Z; every letter pairs or is unpaired with total probability 1; up falls with the width"""
    s = cases.rnd(np.random.default_rng(n), n)
    r = opool.fold2x(cases.TABLES, s, 15).result()
    assert math.isfinite(r["logZ"]) and np.isfinite(r["post"]).all() and np.isfinite(r["up"]).all()
    assert abs(r["logZ"] - r["logZ_out"]) <= 1e-9 * max(1.0, abs(r["logZ"]))
    P = np.zeros((n + 1, n + 1))
    P[np.triu_indices(n + 1, 0)] = r["post"]
    paired = (P + P.T).sum(axis=1)[1:]
    assert np.abs(paired + r["up"][:, 0] - 1.0).max() <= 1e-9
    assert (np.diff(r["up"], axis=1) <= 1e-12).all()
    assert r["post"].min() >= 0 and r["post"].max() <= 1 + 1e-12


# ---- the inputs of tests/test_gpu_vienna2x_edges.py, on the restatement alone
def has_long_range_cell(post, n):
    P = np.zeros((n + 1, n + 1))
    P[np.triu_indices(n + 1, 0)] = post
    i, j = np.nonzero(P > cases.FLOOR)
    return len(i) > 0 and (j - i).max() >= n / 2 and (j - i).min() <= 8


def test_gpu_inputs_have_cells_the_relative_bar_applies_to(opool):
    """assert_prob_close compares relatively only above its floor of 1e-12: every GPU input longer than 8 letters has such cells
    on its longest diagonals (at least one with span >= n / 2) as well as on its short ones"""
    pinned, unpinned = cases.edge_batches()
    seqs = [s for pr in pinned + unpinned for s in pr] + cases.acc_seqs() + [cases.constraint_case()[0]]
    seqs += [x[1] for x in cases.planted_inputs()]
    futures = [(s, opool.fold2x(cases.TABLES, s, 15)) for s in seqs]
    co = [(s1, s2, opool.cofold2x(cases.TABLES, s1, s2)) for s1, s2 in cases.cut_pairs() + [cases.co_constraint_case()[:2]]]
    lens = sorted({len(s) for s in seqs})
    assert all(n in lens for n in (1, 4, 5, 33, 34, 64, 65, 66, 129, 256, 257, 258, 300, 512, 513, 514, 520))
    assert len(pinned) * 2 == 8 and len(unpinned) * 2 % 8 != 0
    for s, f in futures:
        if len(s) > 8:
            assert has_long_range_cell(f.result()["post"], len(s)), len(s)
    for s1, s2, f in co:
        r = f.result()
        if len(s1) + len(s2) > 8:
            assert has_long_range_cell(r["post"], len(s1) + len(s2)), (len(s1), len(s2))
            assert (r["hp"] > cases.FLOOR).any(), (len(s1), len(s2))


# measured on the restatement with the synthetic tables: at the budget the enclosed pair has probability >= 0.985
# (0.981 / 0.939 for 2x3 / 3x2) and >= 0.94 of its letter's pairing probability; one letter past it, <= 3.6e-4.  Asserted with a
# margin: >= 0.9 and >= 0.9 of the letter's at the budget, <= 0.01 past it.
def test_planted_loops_dominate_at_the_budget_and_vanish_past_it(opool):
    futures = [(x, opool.fold2x(cases.TABLES, x[1], 15)) for x in cases.planted_inputs()]
    for (name, s, p, q, at_budget), f in futures:
        r = f.result()
        pq = r["post"][tri_offset(len(s), p) + q]
        paired = 1.0 - r["up"][p - 1, 0]
        print("planted %-16s n=%3d  P(%d,%d) = %.6f   P(letter %d paired) = %.6f" % (name, len(s), p, q, pq, p, paired))
        if at_budget:
            assert pq >= 0.9 and pq >= 0.9 * paired, (name, pq, paired)
        else:
            assert pq <= 0.01, (name, pq)
