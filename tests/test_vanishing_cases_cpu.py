"""What tests/test_gpu_vanishing.py rests on, from the plain double-precision oracles alone (no GPU): the embedding identities of
tests/_vanishing_cases.py against the directly computed oracle, the position of every GPU case's Z~ relative to the flag threshold
of the scaled linear kernels (40 nats on the side its label names, on every exponent its ladder tries), and that no case is vacuous."""
import numpy as np
import pytest

import _vanishing_cases as vc
from _oracle import OraclePool, tri_offset

IDENTITY_FLANKS = ((150, 220), (3, 300), (300, 3))
TOL = 1e-12


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    for f5, f3 in IDENTITY_FLANKS:      # (the longest calls first: they run beside the rest)
        p.mccaskill(vc.flanked(vc.INSERT, f5, f3), vc.MAX_W)
        p.inference(vc.flanked(vc.INSERT, f5, f3))
    yield p
    p.close()


@pytest.fixture(scope="module")
def short(opool):
    s = vc.short_of(vc.INSERT)
    return dict(cf=opool.inference(s).result(), bl=opool.mccaskill(s, vc.MAX_W).result(), B=vc.cf_flank_letter(opool.cf), n=len(s))


def fold_logz(short, case):
    """log Z of a fold case from the short sequence's"""
    return short["cf"]["logZ"] + short["B"] * (case.n - short["n"]) if case.model == "cf" else short["bl"]["logZ"]


def test_poly_a_log_z_is_linear(opool):
    B = vc.cf_flank_letter(opool.cf)
    z40 = opool.inference("A" * 40).result()["logZ"]
    for n in (41, 77, 130, 200):
        assert abs(opool.inference("A" * n).result()["logZ"] - z40 - B * (n - 40)) < 1e-12 * n, n
    assert -0.02 < B < 0.0      # (what makes a long unstructured sequence vanish on s = 0.12)


@pytest.mark.parametrize("f5,f3", IDENTITY_FLANKS)
def test_contrafold_embedding_identity(opool, short, f5, f3):
    L = len(vc.INSERT)
    o = opool.inference(vc.flanked(vc.INSERT, f5, f3)).result()
    block = vc.insert_block_mask(L, f5, f3)
    want = vc.embed_bp(short["cf"]["post"], L, f5, f3)
    assert np.abs(o["post"] - want)[block].max() < TOL
    assert o["post"][~block].sum() < TOL and want[~block].max() == 0.0
    assert abs(o["logZ"] - short["cf"]["logZ"] - short["B"] * (f5 + f3 - 2 * vc.FLANK)) < TOL * (f5 + f3)


@pytest.mark.parametrize("f5,f3", IDENTITY_FLANKS)
def test_vienna_bl_embedding_identity(opool, short, f5, f3):
    L = len(vc.INSERT)
    o = opool.mccaskill(vc.flanked(vc.INSERT, f5, f3), vc.MAX_W).result()
    assert np.abs(o["post"] - vc.embed_bp(short["bl"]["post"], L, f5, f3)).max() < TOL
    assert abs(o["logZ"] - short["bl"]["logZ"]) < TOL
    want = vc.embed_up(short["bl"]["up"], L, f5, f3)
    assert np.abs(o["up"] - want).max() < TOL
    assert (want[:max(0, f5 - vc.FLANK - vc.MAX_W), :] == 1.0).all()      # up is 1 in the flanks


def test_a_flank_of_no_letters_breaks_the_identity(opool, short):
    """why FLANK >= 3 on both sides, in the long and the short sequence alike"""
    L = len(vc.INSERT)
    o = opool.inference(vc.INSERT + "A" * 6).result()
    shifted = np.zeros_like(short["cf"]["post"])
    m = L + 6
    for i in range(1, L + 1):
        shifted[tri_offset(m, i + 3) + i + 3:tri_offset(m, i + 3) + L + 4] = o["post"][tri_offset(m, i) + i:tri_offset(m, i) + L + 1]
    assert np.abs(shifted - short["cf"]["post"]).max() > 1e-6


@pytest.mark.parametrize("k1,k2", [(150, 150), (150, 3), (3, 150)])
def test_two_molecule_embedding_identity(opool, k1, k2):
    """inserts on both sides of the cut: hp, the joint pair matrix's log Z and both folds do not change with the outer flanks"""
    s1s, s2s = vc.cofold_pair(vc.FLANK, vc.FLANK)
    s1, s2 = vc.cofold_pair(k1, k2)
    os_, ol = opool.cofold(s1s, s2s).result(), opool.cofold(s1, s2).result()
    assert abs(ol["logZ"] - os_["logZ"]) < TOL
    assert np.abs(ol["hp"] - vc.embed_hp(os_["hp"], len(s1), len(s2), k1 - vc.FLANK, 0)).max() < TOL
    assert os_["hp"].max() > 0.1
    # the pairs between the inserts enclose the cut: the joint ensemble is not the product of the two folds
    f1, f2 = opool.mccaskill(s1s, 0).result(), opool.mccaskill(s2s, 0).result()
    assert os_["logZ"] > f1["logZ"] + f2["logZ"] + 10.0


# ---- where Z~ of every GPU case lies
@pytest.mark.parametrize("case", vc.fold_cases(), ids=lambda c: "%s-%s-%s" % (c.model, c.label, c.where))
def test_fold_cases_lie_where_their_label_says(short, case):
    lz = fold_logz(short, case)
    s0, down = (vc.CF_S, vc.CF_DOWN) if case.model == "cf" else (vc.BL_S, vc.BL_ORDER)
    first = vc.ln_scaled(lz, s0, case.n)
    print("%s %s %s n = %d: log Z %.3f, ln Z~ %.1f on s = %g" % (case.model, case.label, case.where, case.n, lz, first, s0))
    if case.label == "inside":
        assert vc.inside(first)
        return
    assert first <= vc.LN_LO - vc.MARGIN                       # it VANISHES
    assert down[-1] == 0.0
    for s in down[:-1]:                                        # Vienna-BL: the whole batch tries 0.7 and 1.8 first
        assert vc.outside(vc.ln_scaled(lz, s, case.n))
    assert vc.inside(vc.ln_scaled(lz, 0.0, case.n))            # held by s = 0
    assert len(case.seq) == case.n and case.seq[case.f5:case.f5 + len(vc.INSERT)] == vc.INSERT
    assert min(case.f5, case.f3) >= vc.FLANK and {"5'": case.f5 == vc.FLANK, "3'": case.f3 == vc.FLANK, "mid": abs(case.f5 - case.f3) <= 1}[case.where]


def test_fold_references_are_not_vacuous(short):
    assert short["cf"]["post"].max() > 0.1 and short["bl"]["post"].max() > 0.1
    assert (short["bl"]["up"][vc.FLANK:-vc.FLANK, 0] < 0.9).any()


@pytest.mark.parametrize("case", vc.duplex_cases(), ids=lambda c: "%s-%s" % (c.model, c.label))
def test_duplex_cases_lie_where_their_label_says(opool, case):
    span = len(case.s1) + len(case.s2) + 2
    if case.model == "cf":
        o = opool.duplex(case.s1, case.s2).result()
        lz, hp, s0, order = o["logZ2"][0], o["post"], vc.DX_S, vc.DX_ORDER
    else:
        o = opool.pf_duplex(case.s1, case.s2).result()
        lz, hp, s0, order = o["logZ"], o["pr"], vc.VDX_S, ()
    assert hp.max() > 0.1
    first = vc.ln_scaled(lz, s0, span)
    print("%s duplex %s, %d x %d: log Z %.3f, ln Z~ %.1f on s = %g" % (case.model, case.label, len(case.s1), len(case.s2), lz, first, s0))
    if case.label == "inside":
        assert vc.inside(first)
    elif case.label == "vanishing":
        assert first <= vc.LN_LO - vc.MARGIN
    else:                                                      # held by rung `label`: outside on everything tried before it
        assert first <= vc.LN_LO - vc.MARGIN
        tried = order[:order.index(case.label)]
        for s in tried:
            assert vc.outside(vc.ln_scaled(lz, s, span)), s
        assert vc.inside(vc.ln_scaled(lz, case.label, span))


def test_the_one_pair_and_the_no_pair_duplex(opool):
    s1, s2 = vc.DX_ONE_PAIR
    o = opool.duplex(s1, s2).result()
    span = len(s1) + len(s2) + 2
    assert s1.count("U") == 1 and set(s1) == {"A", "U"} and set(s2) == {"A"}
    assert vc.ln_scaled(o["logZ2"][0], vc.DX_S, span) <= vc.LN_LO - vc.MARGIN       # terms exist, their sum underflows
    for s in vc.DX_ORDER[:-1]:
        assert vc.outside(vc.ln_scaled(o["logZ2"][0], s, span))
    assert vc.inside(o["logZ2"][0])                                                 # held by s = 0
    assert 0.0 < o["post"].max() < 0.1 and (o["post"][:500].max(), o["post"][501:].max()) == (0.0, 0.0)
    a, b = vc.DX_NO_PAIR
    assert set(a) | set(b) == {"A", "G"}
    n = opool.duplex(a, b).result()
    assert n["logZ2"][0] < -1e20 and not n["post"].any()


def test_the_two_molecule_case_vanishes_only_as_a_joint_ensemble(opool):
    c = vc.cofold_case()
    assert len(c.s1) == len(c.s2) == vc.COFOLD_LEN
    s1s, s2s = vc.cofold_pair(vc.FLANK, vc.FLANK)
    joint = opool.cofold(s1s, s2s).result()
    f1, f2 = opool.mccaskill(s1s, vc.MAX_W).result(), opool.mccaskill(s2s, vc.MAX_W).result()
    n = len(c.s1) + len(c.s2)
    print("folds ln Z~ %.1f %.1f, joint ln Z~ %.1f" % (vc.ln_scaled(f1["logZ"], vc.BL_S, len(c.s1)), vc.ln_scaled(f2["logZ"], vc.BL_S, len(c.s2)),
                                                      vc.ln_scaled(joint["logZ"], vc.BL_S, n)))
    assert vc.inside(vc.ln_scaled(f1["logZ"], vc.BL_S, len(c.s1))) and vc.inside(vc.ln_scaled(f2["logZ"], vc.BL_S, len(c.s2)))
    assert vc.ln_scaled(joint["logZ"], vc.BL_S, n) <= vc.LN_LO - vc.MARGIN
    for s in vc.BL_ORDER[:-1]:
        assert vc.outside(vc.ln_scaled(joint["logZ"], s, n))
    assert vc.inside(joint["logZ"]) and vc.inside(f1["logZ"]) and vc.inside(f2["logZ"])
    assert joint["hp"].max() > 0.1 and f1["post"].max() > 0.1 and f2["post"].max() > 0.1
