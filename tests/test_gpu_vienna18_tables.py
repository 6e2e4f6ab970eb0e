"""GPU suite (-m gpu): every kernel family of the ViennaRNA-1.8 semantics under a table set without the symmetries of BL*.

All other GPU parity tests of this model run on the bundled BL* tables, whose mismatchI does not change under a transposition of its
letters nor under type <-> rtype, whose int11 / int22 are constant over most letters and whose dangles are never positive: TXO / TXI and
the FCX decoration of build_vlin_model, the generic weights of span_acc_gaps and the duplex kernels' mmI could mix up the letter order
or the two pairs of a loop and pass them all.  Here the contexts are created on scrambled(18) of
tests/_vienna18_tables.py, written into a tmp dir, and the reference is oracle/vienna_oracle.c on the same file (PARITY UNPINNED against
ViennaRNA; under these tables too the restatement equals its enumeration: tests/test_vienna18_tables_cpu.py, which also proves that
every index mutation of a table moves these very inputs by 100 tolerances or more on the oracle).

Shapes are small: the look-ups are under test, the tiling is not (test_gpu_vienna_edges.py, test_gpu_duplex_edges.py, test_gpu_span_*).
Tolerances are the project's: rel 1e-6 on bp / hp / band, the same with abs_floor 1e-11 on up, 1e-9 * max(1, |log Z|) on log Z."""
import numpy as np
import pytest

import _span_acc_cases as ac
import _vienna18_cases as vc
import test_gpu_duplex_edges as tde
from _oracle import OraclePool, assert_prob_close

pytestmark = pytest.mark.gpu

REL = vc.REL
MODES = [("auto", 0, 1), ("log", 1, 2)]   # name, rh_set_mode, the rh_last_path / rh_last_hybrid_path it must report
FOLD_KERNELS = {"auto": ("vlin_inside_diag<8, 16, false>", "vlin_outside_diag<8, 16, false>"), "log": ("mcv_inside_diag", "mcv_outside_diag")}
FAR_KERNELS = ("lin_far_inside_pk", "lin_far_outside_pk")   # the block products of the "auto" path, on packed 16-letter tiles
CO_KERNEL = {"auto": "vlin_inside_diag<8, 16, true> + vlin_outside_diag<8, 16, true> (s1+s2)", "log": "mcv_inside_diag + mcv_outside_diag (s1+s2)"}


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    return vc.write_tables(tmp_path_factory.mktemp("vienna18"))


@pytest.fixture(scope="module")
def opool(path):
    p = OraclePool(params=path)
    yield p
    p.close()


def new_context(param_file=None):
    import ractip_amd
    return ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL, param_file=param_file)


@pytest.fixture(scope="module", params=MODES, ids=[m[0] for m in MODES])
def vctx(hotlib, path, request):
    """one context per arithmetic path on the scrambled file"""
    name, mode, code = request.param
    c = new_context(path)
    try:
        assert c.vienna_semantics() == 1
        c.set_mode(mode)
        yield c, name, code
    finally:
        c.close()


@pytest.fixture(scope="module")
def vspan(hotlib, path):
    c = new_context(path)
    try:
        assert c.vienna_semantics() == 1
        yield c
    finally:
        c.close()


def logz_close(z, ref):
    return abs(z - ref) <= vc.LOGZ * max(1.0, abs(ref))


def run_folds(c, name, code, pairs, max_w, far=None):
    """far: whether the inside sweep of the batch reaches the block products (None: not asserted).  They start at block diagonal 4,
    one inside launch per block diagonal 4 .. (nmax - 1) // 16 (far_inside_after), so from 65 letters on.  The outside sweep launches
    its products from block diagonal 0 on (far_outside_before): at every length of these tests, and at least as often."""
    c.set_hybrid(False)
    c.set_max_w(max_w)
    c.batch_upload(pairs)
    c.batch_compute()
    assert c.last_path() == code, (c.last_path(), code)
    assert all(c.batch_fallbacks(k) == [] for k in range(4)), [c.batch_fallbacks(k) for k in range(4)]
    k = c.batch_kernels()
    assert (k[0][0], k[1][0]) == FOLD_KERNELS[name], k
    if far is not None and name == "auto":
        inside = max(0, (max(len(s) for pr in pairs for s in pr) - 1) // 16 - 3)
        assert (inside > 0) == far
        assert (k[0][1], k[0][2]) == ((FAR_KERNELS[0], inside) if far else ("", 0)), k
        assert k[1][1] == FAR_KERNELS[1] and k[1][2] >= max(inside, 1), k
    return [c.batch_results(p) for p in range(len(pairs))]


# ---- folds
@pytest.mark.parametrize("max_w", vc.FOLD_WIDTHS)
def test_folds_bp_up_and_log_z(vctx, opool, max_w):
    """random ACGU with one N at 40, 66, 90 and 130 letters (from 66 on through the block products and the decorated FCX / FCB / FCA
    copies), accessibility of 5 and of 33 widths, across the loop budget of 30"""
    c, name, code = vctx
    pairs = vc.fold_pairs()
    assert [len(s) for pr in pairs for s in pr] == list(vc.FOLD_LENGTHS) and all("N" in s for pr in pairs for s in pr)
    for s1, s2 in pairs:
        opool.mccaskill(s1, max_w), opool.mccaskill(s2, max_w)
    res = run_folds(c, name, code, pairs, max_w, far=True)      # 130 letters: five inside launches of the block products
    for (s1, s2), r in zip(pairs, res):
        for s, key, ukey, kz in ((s1, "bp1", "up1", 0), (s2, "bp2", "up2", 1)):
            o = opool.mccaskill(s, max_w).result()
            what = "%s n=%d max_w=%d" % (name, len(s), max_w)
            assert logz_close(r["logZ"][kz], o["logZ"]), (what, r["logZ"][kz], o["logZ"])
            assert_prob_close(r[key], o["post"], rel=REL, what="bp " + what)
            assert r[ukey].shape == (len(s), max_w)
            assert_prob_close(r[ukey], o["up"], rel=REL, abs_floor=vc.UP_FLOOR, what="up " + what)


# ---- planted single loops
def test_planted_single_loops_as_one_batch(vctx, opool):
    """vplanted of tests/_alphabet_cases.py: stack, both 1-bulges, 1x1, 1x2, 2x1, 2x2, 1x3, 1x4, 7x9, 15x15 and a 0x3 bulge; the
    tabulated shapes with every filling of their loop letters (16, 64, 64, 256) between a UA and a CG pair, every shape with all 36
    combinations of closing and enclosed pair type at one filling.  log Z and the posteriors of the closing and of the enclosed pair,
    where the oracle puts more than 0.5 on one of them (at most 5 % of the cases are left out)."""
    c, name, code = vctx
    cases = vc.planted_cases()
    seqs = [x.seq for x in cases]
    for s in seqs:
        opool.mccaskill(s, 1)
    pairs = list(zip(seqs[0::2], seqs[1::2]))
    res = run_folds(c, name, code, pairs, 1, far=False)         # at most 56 letters: no inside block products
    kept, worst = 0, 0.0
    for k, case in enumerate(cases):
        r, which = res[k // 2], k % 2
        o = opool.mccaskill(case.seq, 1).result()
        n = len(case.seq)
        ref = vc.stem_posteriors(o["post"], n, case)
        if ref.max() <= 0.5:
            continue
        kept += 1
        got = vc.stem_posteriors(r["bp2" if which else "bp1"], n, case)
        assert logz_close(r["logZ"][which], o["logZ"]), (name, case.what, r["logZ"][which], o["logZ"])
        worst = max(worst, float((np.abs(got - ref) / ref).max()))
        assert_prob_close(got, ref, rel=REL, what="stem posteriors %s: %s" % (name, case.what))
    print("%s: %d of %d planted loops compared, largest relative error of a stem posterior %.3g" % (name, kept, len(cases), worst))
    assert kept >= (1 - vc.PLANTED_MAY_DROP) * len(cases)


# ---- two-molecule ensemble
def test_two_molecule_ensemble(vctx, opool):
    """set_hybrid(True): hp and log Z of co_pf_fold semantics at 30 + 35 and 70 + 75 letters against vo.cofold (TNC: the stems next to
    the cut)"""
    c, name, code = vctx
    pairs = vc.cofold_pairs()
    for s1, s2 in pairs:
        opool.cofold(s1, s2)
    c.set_max_w(1)
    c.set_hybrid(True)
    try:
        c.batch_upload(pairs)
        c.batch_compute()
        assert c.last_path() == code and c.last_hybrid_path() == code, (c.last_path(), c.last_hybrid_path())
        assert all(c.batch_fallbacks(k) == [] for k in range(4)), [c.batch_fallbacks(k) for k in range(4)]
        assert c.batch_kernels()[2][0] == CO_KERNEL[name], c.batch_kernels()
        res = [c.batch_results(p) for p in range(len(pairs))]
    finally:
        c.set_hybrid(False)
    for (s1, s2), r in zip(pairs, res):
        o = opool.cofold(s1, s2).result()
        what = "%s cofold %d+%d" % (name, len(s1), len(s2))
        assert logz_close(r["logZ"][2], o["logZ"]), (what, r["logZ"][2], o["logZ"])
        assert_prob_close(r["hp"], o["hp"], rel=REL, what="hp " + what)


# ---- pf_duplex
def test_pf_duplex_edge_lengths_and_planted_loops(vctx, opool):
    """dxvl_sweep4<false> ("auto") and dxv_sweep_diag ("log"): hp and log Z of the (61, 9), (62, 62), (63, 64) pairs and of the
    planted duplex loops of tests/test_gpu_duplex_edges.py against vo_pf_duplex"""
    c, name, code = vctx
    pairs = vc.duplex_pairs()
    for _, s1, s2 in pairs:
        opool.pf_duplex(s1, s2)
    c.set_hybrid(False)
    c.set_max_w(1)
    c.batch_upload([(s1, s2) for _, s1, s2 in pairs])
    c.batch_compute()
    tde.assert_ran(c, code, tde.V_KERNEL[name], "scrambled tables")
    for p, (what, s1, s2) in enumerate(pairs):
        r, o = c.batch_results(p), opool.pf_duplex(s1, s2).result()
        assert logz_close(r["logZ"][2], o["logZ"]), (name, what, r["logZ"][2], o["logZ"])
        assert_prob_close(r["hp"], o["pr"], rel=REL, what="hp %s: %s" % (name, what))
        tde.assert_hp_properties(r["hp"])


# ---- span family, against the oracle under the band mask
def check_span(got, ref, what):
    band, up, logz = got
    assert band.shape == ref["band"].shape and up.shape == ref["up"].shape, what
    assert logz_close(logz, ref["logZ"]), (what, logz, ref["logZ"])
    assert_prob_close(band, ref["band"], rel=REL, what=what + " band")
    assert_prob_close(up, ref["up"], rel=REL, abs_floor=vc.UP_FLOOR, what=what + " up")


@pytest.mark.parametrize("n,L,max_w", vc.SPAN_SHAPES)
def test_span_fold(vspan, path, n, L, max_w):
    seq = vc.span_seq(n)
    check_span(vspan.span_fold(seq, L, max_w), ac.masked_acc(seq, L, max_w, params=path), "n=%d L=%d max_w=%d" % (n, L, max_w))


def test_span_fold_batch_of_three_ragged_items(vspan, path):
    lengths, L, max_w = vc.SPAN_BATCH
    seqs = [vc.span_seq(n) for n in lengths]
    for seq, got in zip(seqs, vspan.span_fold_batch(seqs, L, max_w)):
        check_span(got, ac.masked_acc(seq, L, max_w, params=path), "batch item n=%d L=%d max_w=%d" % (len(seq), L, max_w))


def test_planted_single_loops_through_span_fold_batch(vspan, path):
    """every planted loop as one item, L = 40: the outer stems of the longest loops lie beyond the band, in the oracle's mask too"""
    cases = vc.planted_cases()
    L = vc.SPAN_PLANTED_L
    assert min(len(x.seq) for x in cases) < L < max(len(x.seq) for x in cases)
    for case, got in zip(cases, vspan.span_fold_batch([x.seq for x in cases], L, 1)):
        check_span(got, ac.masked_acc(case.seq, L, 1, params=path), "L=%d %s" % (L, case.what))


# ---- sanity of the fixture
def test_the_scrambled_file_was_installed(vctx, hotlib):
    """the same inputs on a BL* context: all three log Z of every pair differ by more than 1e-3"""
    c, name, code = vctx
    pairs = vc.fold_pairs()
    res = run_folds(c, name, code, pairs, 1)
    b = new_context()
    try:
        assert b.vienna_semantics() == 1
        b.set_mode(MODES[[m[0] for m in MODES].index(name)][1])
        b.set_max_w(1)
        b.batch_upload(pairs)
        b.batch_compute()
        for p, r in enumerate(res):
            z, z0 = r["logZ"], b.batch_results(p)["logZ"]
            assert (np.abs(z - z0) > 1e-3).all(), (name, p, z, z0)
    finally:
        b.close()
