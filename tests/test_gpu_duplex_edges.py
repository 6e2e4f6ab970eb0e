"""Duplex (hybridization) sweeps against the CPU oracles at the lengths and loop sizes where their kernels change form.

The scaled linear duplex kernels (duplex_lin.hip, duplex_vlin.hip) are position-dependent in many places: groups of 58 columns with up
to 6 recomputed lanes (dxl_strip8), of 62 columns with two (dxl_sweep4, dxvl_sweep4<S20>), of 64 (dxl_sweep<W>); a grid that counts
from the first group of the pair's own band (kDxBand = 32); a last strip that is partial unless (L1+L2-1) % 8 == 0; a loop budget of
28 unpaired letters (window rows t = 0..28) under the CONTRAfold model and of 30 (kMaxSingle, with skip = t - 27 on the last rows)
under Vienna-BL; log Z by rows of 256 columns per item (dxl_logz_part) or by chunks of 16 rows; posterior tiles of 32 x 32.

Two kinds of input, both checked on the CPU alone first (the tests without the gpu mark):
  * edge_shapes(model): seeded random ACGU at lengths on and next to those constants, ragged behind a (300, 300) dummy pair that
    fixes n1max / n2max, and again alone (n1max = L1: other band-clip and open-end branches);
  * planted(edge, l1, l2): two 8-bp GC stems joined by ONE interior loop of l1 + l2 unpaired letters, a stem end on the column
    edge of a group.  At l1 + l2 = the model's budget the stems hold each other (row sum of hp over a stem letter > 0.9), one letter
    past it the joining loop no longer exists and the row sum falls by more than 15 %: a window that is one tap short or long, or
    displaced by a column at the longest loop, moves hp by tens of percent and not by rounding.

References: oracle/cf_oracle.c (CONTRAfold model), oracle/vienna_oracle.c (Vienna-BL, ViennaRNA-1.8 semantics: PARITY UNPINNED
against ViennaRNA, absent and unversioned; the restatement is pinned to enumeration by tests/test_vienna_oracle.py) and
oracle/vienna2x.py (2.x semantics, pure Python).  Tolerances are the project's: 1e-6 relative on hp above 1e-12, 1e-9 on log Z
(1e-8 at 257 x 300; 1e-9 * max(1, |log Z|) under Vienna-BL), 1e-10 between two organisations of the same arithmetic, 1e-9 between
the linear and the log-space kernels of Vienna-BL, the same bits where only placement changes.  Every GPU test asserts the path
(rh_last_hybrid_path), the absence of fallbacks and the kernel name (rh_batch_kernels) of what it compares."""
import contextlib
import math
import os
import sys

import numpy as np
import pytest

import bench
from _oracle import OraclePool, assert_prob_close, check_pair_properties, threshold_scans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import vienna2x as v2  # noqa: E402

REL = 1e-6
MODES = [("auto", 0, 1), ("log", 1, 2)]   # name, rh_set_mode, the rh_last_hybrid_path it must report
MODE_IDS = [m[0] for m in MODES]
DX_KEYS = ("RH_DX_STRIP", "RH_DX_QUAD", "RH_DX_W")


# ---- 1. the inputs: tests/_duplex_cases.py
from _duplex_cases import (DUMMY, PLANT, STEM_A, STEM_B, batch_pairs, edge_pairs, edge_shapes, planted, planted_pairs, rc, rnd,  # noqa: E402,F401
                           stem_letters, stem_row_sums)


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    yield p
    p.close()


def test_edge_shapes_cover_every_residue_of_the_strips_and_the_groups():
    """The last strip of dxl_strip8 holds (L1+L2-1) % 8 rows (8 if 0), the last launch of the four-diagonal kernels (L1+L2-1) % 4:
    every residue occurs.  First lengths lie on, one below and one above multiples of the group widths; the row count L1 + L2 - 1 of the
    Vienna shapes on both sides of a multiple of 16."""
    cf, vb = edge_shapes("contrafold"), edge_shapes("vienna")
    assert {(a + b - 1) % 8 for a, b in cf} == set(range(8))
    assert {(a + b - 1) % 4 for a, b in cf} == set(range(4))
    assert {(a + b - 1) % 4 for a, b in vb} == set(range(4))
    assert {a % 58 for a, _ in cf} >= {57, 0, 1} and {a % 62 for a, _ in cf} >= {0, 1} and {a % 64 for a, _ in cf} >= {63, 0, 1}
    assert {a % 62 for a, _ in vb} >= {61, 0, 1}
    assert {(a + b - 1) % 16 for a, b in vb} >= {15, 0, 1}
    assert {a for a, _ in cf} >= {1} and {b for _, b in cf} >= {1} and {a for a, _ in vb} >= {1} and {b for _, b in vb} >= {1}
    for shapes in (cf, vb):
        assert all(a <= DUMMY[0] and b <= DUMMY[1] for a, b in shapes) and len(set(shapes)) == len(shapes)
    for model in PLANT:
        for what, s1, s2 in planted_pairs(model):
            assert len(s1) <= DUMMY[0] and len(s2) <= DUMMY[1], what


def test_planted_stems_sit_on_the_column_edges():
    for model, P in PLANT.items():
        for e in P["edges"]:
            for l1, l2 in P["loops"]:
                s1, s2 = planted(e, l1, l2)
                assert s1[e - 8:e] == STEM_A and s1[e:e + l1] == "A" * l1 and s1[e + l1:e + l1 + 8] == STEM_B      # stem A on letters e-7 .. e
                s1, s2 = planted(e, l1, l2, on="B")
                assert s1[e - 1:e + 7] == STEM_B and s1[e - 2 - l1] == "C" and s1[e - 9 - l1:e - 1 - l1] == STEM_A   # stem B from letter e
                assert s2.count("A") == len(s2) - 16


@pytest.mark.parametrize("model", ["contrafold", "vienna"])
def test_edge_shapes_have_cells_the_relative_bar_applies_to(opool, model):
    """Random sequences put little mass on any one cell: every edge shape still has at least 20 reference cells above 1e-6 (thousands
    where both strands have 100 letters or more), far above the 1e-12 floor below which assert_prob_close is an absolute check only."""
    pairs = edge_pairs(model)
    call = opool.duplex if model == "contrafold" else opool.pf_duplex
    for s1, s2 in pairs:
        call(s1, s2)
    for s1, s2 in pairs:
        o = call(s1, s2).result()
        hp = o["post"] if model == "contrafold" else o["pr"]
        n = int((hp > 1e-6).sum())
        assert n >= 20, (len(s1), len(s2), n)
        if min(len(s1), len(s2)) >= 100:
            assert n >= 1000, (len(s1), len(s2), n)


@pytest.mark.parametrize("model", ["contrafold", "vienna"])
def test_planted_loops_jump_at_the_loop_budget_on_the_oracle(opool, model):
    """On the oracles alone: with l1 + l2 at the model's budget (28 / 30) the row sum of hp over a letter of either stem is above
    0.9; one unpaired letter more and the lower of the two is at most 0.85 of what it was.  The planted inputs discriminate."""
    P = PLANT[model]
    call = opool.duplex if model == "contrafold" else opool.pf_duplex
    key = "post" if model == "contrafold" else "pr"
    for e in P["edges"]:
        for at, past in P["jumps"]:
            assert sum(at) == P["budget"] and sum(past) == P["budget"] + 1
            for on in "AB":
                call(*planted(e, *at, on=on)), call(*planted(e, *past, on=on))
    for e in P["edges"]:
        for l1, l2 in P["loops"]:
            if l1 + l2 <= P["budget"]:
                for on in "AB":
                    rows = stem_row_sums(call(*planted(e, l1, l2, on=on)).result()[key], e, l1, on)
                    print("%s edge %d stem %s loop %dx%d: row sums %.4f %.4f" % (model, e, on, l1, l2, rows[0], rows[1]))
                    assert min(rows) > 0.9, (e, on, l1, l2, rows)
        for at, past in P["jumps"]:
            for on in "AB":
                r_at = stem_row_sums(call(*planted(e, *at, on=on)).result()[key], e, at[0], on)
                r_past = stem_row_sums(call(*planted(e, *past, on=on)).result()[key], e, past[0], on)
                print("%s edge %d stem %s: %r %.4f %.4f -> %r %.4f %.4f" % ((model, e, on, at) + tuple(r_at) + (past,) + tuple(r_past)))
                assert min(r_at) > 0.9 and min(r_past) <= 0.85 * min(r_at), (e, on, at, r_at, past, r_past)


# ---- the GPU side
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


HP_TH = dict(bench.SCANS)[2]     # the benchmark's threshold of the hp scan


def assert_ran(c, path, kernel, what):
    """The last compute took the path it claims, flagged nothing, recomputed nothing, and reports the kernel"""
    assert c.last_hybrid_path() == path, (what, c.last_hybrid_path(), path)
    assert c.batch_fallbacks(1) == [] and c.batch_fallbacks(3) == [], (what, c.batch_fallbacks(1), c.batch_fallbacks(3))
    assert c.batch_kernels()[2][0] == kernel, (what, c.batch_kernels()[2][0], kernel)


def run_batch_and_alone(c, pairs, path, kernel, alone=True):
    """The batch on context c, then (alone=True) every pair but the dummy by itself through rh_duplex: dict(res, cand, alone)"""
    seqs = [(s1, s2) for _, s1, s2 in pairs]
    c.batch_upload(seqs)
    c.batch_compute()
    assert_ran(c, path, kernel, "batch")
    out = dict(res=[c.batch_results(p) for p in range(len(seqs))], kernel=c.batch_kernels()[2][0])
    rec, first = c.batch_candidates_all(2, HP_TH)
    out["cand"] = (rec.copy(), first.copy())
    out["alone"] = []
    if alone:
        for what, s1, s2 in pairs[1:]:
            out["alone"].append(c.duplex(s1, s2))
            assert_ran(c, path, kernel, "alone: " + what)
    return out


def assert_hp_properties(hp):
    assert np.isfinite(hp).all() and hp.min() >= 0 and hp.max() <= 1
    assert hp[0].max() == 0 and hp[:, 0].max() == 0
    assert hp.sum(axis=1).max() <= 1 + 1e-9 and hp.sum(axis=0).max() <= 1 + 1e-9


def assert_alone_has_the_batch_bits(pairs, run):
    for (what, s1, s2), r, (hp, z) in zip(pairs[1:], run["res"][1:], run["alone"]):
        assert np.array_equal(hp, r["hp"]) and z == r["logZ"][2], ("alone differs from the batch: " + what, z, r["logZ"][2])


def assert_candidates_are_the_scan_of_the_dense_result(run):
    rec, first = run["cand"]
    assert first[0] == 0 and first[-1] == len(rec) and len(rec) > 0
    for p, r in enumerate(run["res"]):
        i, j, pr = threshold_scans(r, (2, HP_TH))
        mine = rec[first[p]:first[p + 1]]
        assert len(mine) == len(i) and np.array_equal(mine["i"], i) and np.array_equal(mine["j"], j) and np.array_equal(mine["p"], pr), p


# ---- 2. CONTRAfold model: dense parity on the default organisation and on the log-space kernels
CF_KERNEL = {"auto": "dxl_strip8", "log": "dx_sweep_diag"}
# 3. the organisations of the linear sweeps (plan_dx_lin) and the name each must report
CF_ORGS = [
    ({"RH_DX_STRIP": "0"}, "dxl_sweep4"),
    ({"RH_DX_QUAD": "0"}, "dxl_sweep<4>"),
    ({"RH_DX_QUAD": "0", "RH_DX_W": "2"}, "dxl_sweep<2>"),
    ({"RH_DX_W": "8"}, "dxl_sweep<8>"),
]


def cf_context(mode, env):
    import ractip_amd
    with switches(env, clear=DX_KEYS):
        c = ractip_amd.Context(device=0)
    try:
        c.set_mode(mode)
    except Exception:
        c.close()
        raise
    return c


def submit_cf_oracle(opool):
    for _, s1, s2 in batch_pairs("contrafold"):
        opool.duplex(s1, s2)


def check_cf_against_the_oracle(pairs, res, opool, what):
    worst = 0.0
    for (name, s1, s2), r in zip(pairs, res):
        o = opool.duplex(s1, s2).result()
        w = "%s: %s" % (what, name)
        tol = 1e-8 if len(s1) * len(s2) >= 257 * 300 else 1e-9       # (the suite's bar at that size: test_production_lengths_dense_vs_oracle)
        assert abs(r["logZ"][2] - o["logZ2"][0]) < tol, (w, r["logZ"][2], o["logZ2"][0])
        big = o["post"] > 1e-12
        worst = max(worst, float((np.abs(r["hp"] - o["post"])[big] / o["post"][big]).max()))
        assert_prob_close(r["hp"], o["post"], rel=REL, what="hp " + w)
    print("%s: largest relative error of hp over %d pairs %.3g" % (what, len(pairs), worst))


@pytest.fixture(scope="module")
def cf_runs(hotlib, opool):
    """The CONTRAfold batch on the default context, scaled linear ("auto": dxl_strip8) and log-space ("log": dx_sweep_diag)"""
    submit_cf_oracle(opool)
    pairs = batch_pairs("contrafold")
    out = {}
    for name, mode, path in MODES:
        c = cf_context(mode, {})
        try:
            out[name] = run_batch_and_alone(c, pairs, path, CF_KERNEL[name])
        finally:
            c.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_contrafold_edge_batch_dense_vs_oracle(opool, cf_runs, name, mode, path):
    """dxl_strip8 + dxl_logz_part + dxl_posterior ("auto", rh_last_hybrid_path = 1, no fallback) and dx_sweep_diag ("log", 2): hp and
    log Z of every edge shape and planted pair == oracle/cf_oracle.c at 1e-6 / 1e-9, in the ragged batch behind the (300, 300) dummy;
    each pair alone (n1max = L1: the band clips and the open-end lanes differ) has the bits it has in the batch; the properties of
    check_pair_properties; the hp candidates at the benchmark's threshold are the scan of the dense result."""
    pairs, run = batch_pairs("contrafold"), cf_runs[name]
    print("kernel: %s" % run["kernel"])
    assert run["kernel"] == CF_KERNEL[name]
    check_cf_against_the_oracle(pairs, run["res"], opool, name)
    assert_alone_has_the_batch_bits(pairs, run)
    for (what, s1, s2), r in zip(pairs, run["res"]):
        check_pair_properties(s1, s2, r)
    assert_candidates_are_the_scan_of_the_dense_result(run)
    P = PLANT["contrafold"]
    by_name = {what: r for (what, _, _), r in zip(pairs, run["res"])}
    for e in P["edges"]:        # the jump the CPU test pins on the oracle, on the kernel's own hp
        for at, past in P["jumps"]:
            r_at = stem_row_sums(by_name["planted edge %d loop %dx%d stem A" % ((e,) + at)]["hp"], e, at[0])
            r_past = stem_row_sums(by_name["planted edge %d loop %dx%d stem A" % ((e,) + past)]["hp"], e, past[0])
            assert min(r_at) > 0.9 and min(r_past) <= 0.85 * min(r_at), (e, at, r_at, past, r_past)


@pytest.mark.gpu
@pytest.mark.parametrize("env,kernel", CF_ORGS, ids=["+".join("%s=%s" % kv for kv in env.items()) for env, _ in CF_ORGS])
def test_contrafold_organisations_vs_oracle_and_default(opool, cf_runs, env, kernel):
    """dxl_sweep4 (62-column groups, hand-over through LDS), dxl_sweep<4>, dxl_sweep<2>, dxl_sweep<8> (64-column groups) on the edge
    batch: each against oracle/cf_oracle.c at 1e-6 / 1e-9 on its own, and against dxl_strip8 at 1e-10."""
    pairs, base = batch_pairs("contrafold"), cf_runs["auto"]
    c = cf_context(0, env)
    try:
        run = run_batch_and_alone(c, pairs, 1, kernel, alone=False)
    finally:
        c.close()
    print("kernel: %s" % run["kernel"])
    assert run["kernel"] == kernel != base["kernel"]
    check_cf_against_the_oracle(pairs, run["res"], opool, kernel)
    assert_candidates_are_the_scan_of_the_dense_result(run)
    for (what, _, _), r, r0 in zip(pairs, run["res"], base["res"]):
        assert abs(r["logZ"][2] - r0["logZ"][2]) <= 1e-10, (kernel, what)
        assert_prob_close(r["hp"], r0["hp"], rel=1e-10, what="hp %s vs dxl_strip8: %s" % (kernel, what))


# ---- 4. Vienna-BL, ViennaRNA-1.8 semantics: pf_duplex, the hp source of the default command line
V_KERNEL = {"auto": "dxvl_sweep4<false>", "log": "dxv_sweep_diag"}


def vcontext(mode, hybrid=False):
    import ractip_amd
    c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL)
    try:
        c.set_mode(mode)
        c.set_hybrid(hybrid)
    except Exception:
        c.close()
        raise
    return c


def logz_close(z, ref):
    return abs(z - ref) <= 1e-9 * max(1.0, abs(ref))


@pytest.fixture(scope="module")
def v_runs(hotlib, opool):
    pairs = batch_pairs("vienna")
    for _, s1, s2 in pairs:
        opool.pf_duplex(s1, s2)
    out = {}
    for name, mode, path in MODES:
        c = vcontext(mode, hybrid=False)
        try:
            out[name] = run_batch_and_alone(c, pairs, path, V_KERNEL[name])
        finally:
            c.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_vienna_bl_edge_batch_dense_vs_cpu_restatement(opool, v_runs, name, mode, path):
    """dxvl_sweep4<false> + dxvl_logz_part<false> + dxl_posterior ("auto", rh_last_hybrid_path = 1, no fallback) and dxv_sweep_diag
    ("log", 2): hp and log Z of every Vienna edge shape and planted pair (loops of 30 and 31 unpaired letters, the stems on the edges
    of the 62-column groups) == pf_duplex of oracle/vienna_oracle.c (PARITY UNPINNED against ViennaRNA, absent and unversioned; the
    restatement is pinned to enumeration) at 1e-6 / 1e-9 * max(1, |log Z|); each pair alone has the bits it has in the batch."""
    pairs, run = batch_pairs("vienna"), v_runs[name]
    print("kernel: %s" % run["kernel"])
    assert run["kernel"] == V_KERNEL[name]
    worst = 0.0
    for (what, s1, s2), r in zip(pairs, run["res"]):
        o = opool.pf_duplex(s1, s2).result()
        assert logz_close(r["logZ"][2], o["logZ"]), (name, what, r["logZ"][2], o["logZ"])
        big = o["pr"] > 1e-12
        worst = max(worst, float((np.abs(r["hp"] - o["pr"])[big] / o["pr"][big]).max()))
        assert_prob_close(r["hp"], o["pr"], rel=REL, what="hp %s: %s" % (name, what))
        assert_hp_properties(r["hp"])
    print("%s: largest relative error of hp over %d pairs %.3g" % (name, len(pairs), worst))
    assert_alone_has_the_batch_bits(pairs, run)
    assert_candidates_are_the_scan_of_the_dense_result(run)
    P = PLANT["vienna"]
    by_name = {what: r for (what, _, _), r in zip(pairs, run["res"])}
    for e in P["edges"]:
        for at, past in P["jumps"]:
            r_at = stem_row_sums(by_name["planted edge %d loop %dx%d stem A" % ((e,) + at)]["hp"], e, at[0])
            r_past = stem_row_sums(by_name["planted edge %d loop %dx%d stem A" % ((e,) + past)]["hp"], e, past[0])
            assert min(r_at) > 0.9 and min(r_past) <= 0.85 * min(r_at), (e, at, r_at, past, r_past)


@pytest.mark.gpu
def test_vienna_bl_linear_and_log_space_kernels_agree_on_the_edge_batch(v_runs):
    """dxvl_sweep4<false> against dxv_sweep_diag on the same batch: hp to 1e-9, log Z to 1e-10, the bars of
    test_vienna_bl_linear_duplex_path_and_its_fallback (PARITY UNPINNED: both are compared with the CPU restatement above)."""
    pairs = batch_pairs("vienna")
    assert (v_runs["auto"]["kernel"], v_runs["log"]["kernel"]) == (V_KERNEL["auto"], V_KERNEL["log"])
    for (what, _, _), a, b in zip(pairs, v_runs["auto"]["res"], v_runs["log"]["res"]):
        assert abs(a["logZ"][2] - b["logZ"][2]) < 1e-10 * max(1.0, abs(b["logZ"][2])), what
        assert_prob_close(a["hp"], b["hp"], rel=1e-9, what="linear vs log pf_duplex: " + what)


# ---- 5. ViennaRNA-2.x semantics on the linear kernel (dxvl_sweep4<true>), the synthetic all-distinct tables of random_tables(23)
INHERIT, AUTO, LOG, LINEAR = -1, 0, 1, 2
SWEEP_2X = "dxvl_sweep4<true>"
HP_2X = dict(rtol=1e-8, atol=1e-12)      # the bars of test_gpu_duplex2x_linear.py; log Z: rel 1e-9
# the Vienna loops, and the shapes acc1n / acc23 take straight from global memory at a + dir*tw (1xn) and a + 3*dir, 4*dir (2x3): with
# the stems on the column edge those taps lie in the columns of the neighbouring group
LOOPS_2X = PLANT["vienna"]["loops"] + [(29, 1), (2, 3), (3, 2)]
# Which reference: oracle/vienna2x.py's pf_duplex is pure Python (1.3 s at 62 x 62, growing with L1 * L2 * 30^2 on random letters;
# 0.03 s on a planted pair, whose poly-A letters pair with nothing).  It is the reference of every planted pair and of the edge
# shapes of at most ORACLE_2X_CELLS cells: (61, 9), (62, 62), (63, 64), (1, 130), (130, 1), (7, 250), (250, 7), (31, 34), (2, 30),
# (31, 33), (31, 35).  The others -- (123, 200), (124, 62), (125, 40), (186, 187), (248, 249) and the dummy -- are compared
# with the log-space kernels of the same context (dxv_sweep_diag), which test_gpu_vienna2x.py holds against the same oracle.
ORACLE_2X_CELLS = 4100


def planted_pairs_2x():
    return [("planted edge %d loop %dx%d stem %s" % (e, l1, l2, on),) + planted(e, l1, l2, on)
            for e in PLANT["vienna"]["edges"] for l1, l2 in LOOPS_2X for on in "AB"]


def batch_pairs_2x():
    rng = np.random.RandomState(300)
    out = [("dummy",) + (rnd(rng, DUMMY[0]), rnd(rng, DUMMY[1]))]
    out += [("edge shape %d x %d" % (len(a), len(b)), a, b) for a, b in edge_pairs("vienna")]
    return out + planted_pairs_2x()


def test_2x_planted_loops_include_the_tabulated_shapes_and_feel_the_budget():
    """On oracle/vienna2x.py alone: the 1xn and 2x3 loops are planted; every loop within MAXLOOP = 30 holds both stems (row sums
    above 0.9).  Under the synthetic tables a stem is worth far more than under BL*, and one letter past the budget the row sums
    fall only from 0.999998 to 0.997 (other joining structures take over) -- still 1e-3, five orders above the 1e-8 bar of hp."""
    assert {(1, 29), (29, 1), (2, 3), (3, 2)} <= set(LOOPS_2X) and v2.MAXLOOP == PLANT["vienna"]["budget"]
    T = v2.random_tables(23)
    for l1, l2 in LOOPS_2X:
        if l1 + l2 <= v2.MAXLOOP:
            assert min(stem_row_sums(v2.pf_duplex(T, *planted(62, l1, l2))[2], 62, l1)) > 0.9, (l1, l2)
    for at, past in PLANT["vienna"]["jumps"]:
        r_at = stem_row_sums(v2.pf_duplex(T, *planted(62, *at))[2], 62, at[0])
        r_past = stem_row_sums(v2.pf_duplex(T, *planted(62, *past))[2], 62, past[0])
        print("2.x edge 62: %r %.6f %.6f -> %r %.6f %.6f" % ((at,) + tuple(r_at) + (past,) + tuple(r_past)))
        assert min(r_at) > 0.9 and min(r_past) < min(r_at) - 1e-3, (at, r_at, past, r_past)


@pytest.fixture(scope="module")
def runs_2x(hotlib, tmp_path_factory):
    import ractip_amd
    T = v2.random_tables(23)
    path = str(tmp_path_factory.mktemp("par") / "synthetic_v20.par")
    v2.write_par_v20(path, T)
    pairs = batch_pairs_2x()
    c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL, param_file=path, vienna=dict(use_bl_param=False))
    try:
        assert c.vienna_semantics() == 2
        c.set_duplex_mode(LINEAR)
        lin = run_batch_and_alone(c, pairs, 1, SWEEP_2X)
        c.set_duplex_mode(LOG)
        log = run_batch_and_alone(c, pairs, 2, "dxv_sweep_diag", alone=False)
    finally:
        c.close()
    return T, lin, log


def same_logz_2x(a, b):
    return (a < -1e18 and b < -1e18) or a == pytest.approx(b, rel=1e-9)


@pytest.mark.gpu
def test_2x_linear_kernel_planted_loops_and_small_edge_shapes_vs_the_restatement(runs_2x):
    """dxvl_sweep4<true> (rh_set_duplex_mode(LINEAR), rh_last_hybrid_path = 1, no fallback) against pf_duplex of oracle/vienna2x.py
    (PARITY UNPINNED, like the rest of the Vienna model): every planted pair -- the 1xn loops (1, 29), (29, 1) and the 2x3 loops
    (2, 3), (3, 2) among them, stems on columns 62 and 124 -- and the edge shapes of at most ORACLE_2X_CELLS cells."""
    T, lin, _ = runs_2x
    print("kernel: %s" % lin["kernel"])
    assert lin["kernel"] == SWEEP_2X
    n = 0
    for (what, s1, s2), r in zip(batch_pairs_2x(), lin["res"]):
        if not (what.startswith("planted") or len(s1) * len(s2) <= ORACLE_2X_CELLS):
            continue
        efw, ebk, pr = v2.pf_duplex(T, s1, s2)
        assert math.isfinite(efw) and efw == pytest.approx(ebk, rel=1e-10), what
        assert r["logZ"][2] == pytest.approx(efw, rel=1e-9), (what, r["logZ"][2], efw)
        assert np.allclose(r["hp"], pr, **HP_2X), (what, np.abs(r["hp"] - pr).max())
        n += 1
    assert n == len(planted_pairs_2x()) + 11


@pytest.mark.gpu
def test_2x_linear_kernel_vs_log_space_on_the_edge_batch_and_alone(runs_2x):
    """dxvl_sweep4<true> against dxv_sweep_diag of the same context on the whole batch (the reference of the edge shapes the
    pure-Python restatement is too slow for); each pair alone has the bits it has in the batch."""
    _, lin, log = runs_2x
    pairs = batch_pairs_2x()
    assert (lin["kernel"], log["kernel"]) == (SWEEP_2X, "dxv_sweep_diag")
    for (what, _, _), a, b in zip(pairs, lin["res"], log["res"]):
        assert same_logz_2x(a["logZ"][2], b["logZ"][2]), (what, a["logZ"][2], b["logZ"][2])
        assert np.allclose(a["hp"], b["hp"], **HP_2X), (what, np.abs(a["hp"] - b["hp"]).max())
        assert_hp_properties(a["hp"])
    assert_alone_has_the_batch_bits(pairs, lin)
