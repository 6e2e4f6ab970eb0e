"""Every CONTRAfold-model organisation on a context created with rh_create(..., param_file) of a SCRAMBLED weight file.

Everything a context builds from the weights on the host -- build_lin_model, build_dx_lin_model with the fused F[0] / F[1] tables,
strip_weights with its factored A(t) B(|l1 - l2|) form and the residual tables W4 / Bp / Rx, the zero-padded copy of mccaskill_small.hip,
the hairpin length table, the scale exponents -- otherwise has one input in the suite: the bundled file (test_custom_parameter_file
runs one fold and one duplex on the default organisation).  Here every context loads tests/_contrafold_weights.py's scrambled(19) file
(every row moved, the rows that are 0 in the bundled file included) and is compared with oracle/cf_oracle.c under the same file:

  1. the default organisation, "auto" and "log": folds, the 528 loop shapes, the 876 letter fillings, the hairpin / exterior / multiloop
     fillings, in ragged batches of 256 behind the 300-letter dummy; path, no fallback and kernel names as the bundled-file tests assert
     them -- the strip names carry FILT = 1: the factored filter ran, not the silent dense fallback of strip_weights;
  2. every row of test_gpu_contrafold_edges.VARIANTS on class_subset(rot) and the folds (RH_SMALL=1: short_set(); RH_FAR2=1: the 257- and
     273-letter folds), against the oracle and against the default;
  3. the duplex strips and every row of test_gpu_duplex_edges.CF_ORGS on the duplex inputs;
  4. mccaskill_acc.hip against the clone oracle built from the scrambled rows;
  5. two files that differ only in the rows no derivation reads give the same BYTES (the one test that sees a read that lands where the
     bundled file holds 0);
  6. the single-call entries against the batch; 7. a bundled-file context is another model on every input.

Tolerances are the project's: rel 1e-6 above 1e-12 on bp and hp, 1e-9 on log Z, 2e-6 on the float up, rel 1e-6 / floor 1e-11 on up[i][w].
The inputs and the proof that they would notice an index mix-up: tests/_contrafold_weight_cases.py, tests/test_contrafold_weights_cpu.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _contrafold_cases as cc
import _contrafold_weight_cases as wc
import _contrafold_weights as cw
from _cf_clone import region_up
from _oracle import OraclePool, assert_prob_close
from test_gpu_cf_accessibility import FLOOR as ACC_FLOOR, REL as ACC_REL
from test_gpu_contrafold_edges import (FAR_PK, KERNELS, MODE_IDS, MODES, ORG_KEYS, PAIRS as PAIR_KERNELS, REL, STRIPS, VARIANTS, assert_ran,
                                       check_against_the_oracle, run_batches, switches)
from test_gpu_duplex_edges import CF_KERNEL, CF_ORGS, DX_KEYS, assert_ran as assert_dx_ran, check_cf_against_the_oracle

pytestmark = pytest.mark.gpu

assert STRIPS == ("lin_inside_strip<8, 8, 1>", "lin_outside_strip<8, 8, 1>")        # FILT = 1 is the last template argument


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cf_weights")
    rows = cw.scrambled()
    return dict(dir=d, rows=rows, scrambled=cw.write(d / "scrambled.params", rows, seed=1),
                unread=cw.write(d / "scrambled_unread.params", cw.with_unread_moved(rows, 0.3), seed=2))


@pytest.fixture(scope="module")
def opool(files):
    p = OraclePool(cf_params=files["scrambled"])
    yield p
    p.close()


def context(param_file, mode, env=None):
    """a context on `param_file` (None: the bundled file) created under the switches `env`, every other organisation switch unset"""
    import ractip_amd
    with switches(env or {}, clear=ORG_KEYS + DX_KEYS):
        c = ractip_amd.Context(device=0, param_file=param_file)
    try:
        c.set_mode(mode)
    except Exception:
        c.close()
        raise
    return c


def planted():
    """[(family, case, varied pair or None)] of the letter, hairpin, exterior and multiloop fillings"""
    out = [("letters", c, None) for c in wc.letter_cases()]
    for fam, cases in wc.junction_cases().items():
        out += [(fam, c, v) for c, v in cases]
    return out


def default_seqs():
    seen, out = set(), []
    for s in wc.fold_seqs() + [c.seq for c in cc.shape_set()] + [c.seq for _, c, _ in planted()]:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def variant_cases(rot):
    cases = cc.class_subset(rot % 4)
    if "RH_SMALL" in VARIANTS[rot][0]:
        cases = cases + cc.short_set()
    return cases


def variant_folds(rot):
    return wc.fold_seqs() + (wc.fold_seqs(far2=True) if VARIANTS[rot][0].get("RH_FAR2") == "1" else [])


@pytest.fixture(scope="module")
def runs(hotlib, opool, files):
    """The default organisation under the scrambled file: the inputs of (1) on "auto" and "log", and on "auto" also what the organisations
    of (2) are compared with"""
    seqs = default_seqs()
    more = [c.seq for c in cc.class_set() + cc.short_set()] + wc.fold_seqs(far2=True)
    for s in seqs + more:
        opool.inference(s)
    out = {}
    for name, mode, path in MODES:
        c = context(files["scrambled"], mode)
        try:
            out[name] = run_batches(c, seqs + (more if name == "auto" else []), path, KERNELS[name], far=FAR_PK if name == "auto" else None)
        finally:
            c.close()
    return out


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_default_organisation_dense_vs_oracle_under_the_scrambled_file(opool, runs, name, mode, path):
    """lin_inside_strip<8, 8, 1> + lin_outside_strip<8, 8, 1> ("auto": the FACTORED filter, rh_last_path = 1, no fallback, nothing held
    by another scale exponent -- run_batches asserts all of it per batch) and mc_inside_diag + mc_outside_diag ("log"): bp, up and log Z of
    every input == the oracle under the same file; the in-budget shapes keep their stems on the kernel's own posterior, and the kept
    letter cases their closing or enclosed pair."""
    res = runs[name]
    shapes = cc.shape_set()
    check_against_the_oracle(opool, wc.fold_seqs(), res, name + " folds")
    check_against_the_oracle(opool, [c.seq for c in shapes], res, name + " shapes", [c.what for c in shapes])
    for c in shapes:
        if c.l1 + c.l2 <= cc.BUDGET:
            assert min(cc.stem_probs(res[c.seq].bp, c)) >= 0.9, c.what
    per_family = {}
    for fam, c, v in planted():
        per_family.setdefault(fam, []).append(c)
    for fam, cases in per_family.items():
        check_against_the_oracle(opool, [c.seq for c in cases], res, "%s %s" % (name, fam), [c.what for c in cases])
        keep = wc.kept(cases, [opool.inference(c.seq).result()["post"] for c in cases])
        for k in keep:      # (the dense comparison above holds both stem posteriors to 1e-6)
            assert wc.stem_posteriors(res[cases[k].seq].bp, len(cases[k].seq), cases[k]).max() > 0.5, cases[k].what


@pytest.mark.parametrize("rot", range(len(VARIANTS)), ids=["+".join("%s=%s" % kv for kv in v[0].items()) for v in VARIANTS])
def test_organisations_vs_oracle_and_default_under_the_scrambled_file(opool, runs, files, rot):
    """Each organisation on the class set (the column rotates) and the folds: against the oracle at 1e-6 / 1e-9 on its own, against the
    default at 1e-10 (the same bits where only placement or the launch mode changes), with the kernel names it must report.
    RH_STRIP_FILT=0 (dense) against the factored default is the direct check of strip_weights under new numbers; RH_SMALL=1 runs the 528
    short shapes on mccaskill_small.hip's own copy of the weights; RH_FAR2=1 runs the 257- and 273-letter folds."""
    env, kernels, far, kind = VARIANTS[rot]
    cases = variant_cases(rot)
    folds = variant_folds(rot)
    seqs = [c.seq for c in cases] + folds
    names = [c.what for c in cases] + ["n = %d" % len(s) for s in folds]
    c = context(files["scrambled"], 0, env)
    try:
        res = run_batches(c, seqs, 1, kernels, far=far)
    finally:
        c.close()
    print("kernels: %r %r" % (kernels, far))
    check_against_the_oracle(opool, seqs, res, "%r" % (env,), names)
    base = runs["auto"]
    changed = 0
    for s, w in zip(seqs, names):
        a, b = res[s], base[s]
        if kind == "bits":
            assert np.array_equal(a.bp, b.bp) and np.array_equal(a.up, b.up) and a.z == b.z, (env, w)
            continue
        changed += not np.array_equal(a.bp, b.bp)
        assert abs(a.z - b.z) <= 1e-10, (env, w, a.z, b.z)
        assert_prob_close(a.bp, b.bp, rel=1e-10, what="bp %r vs the default: %s" % (env, w))
        assert np.abs(a.up - b.up).max() <= 1e-10, (env, w)
    if kind == "kernels" or "RH_SMALL" in env:
        assert changed > 0, ("another kernel set and not one bit differs", env)


# ---- 3. duplex
def duplex_batch():
    return [wc.duplex_dummy()] + wc.duplex_pairs()


def run_duplex(c, pairs, path, kernel):
    c.batch_upload([(s1, s2) for _, s1, s2 in pairs])
    c.batch_compute()
    assert_dx_ran(c, path, kernel, "batch")
    return [c.batch_results(p) for p in range(len(pairs))]


@pytest.fixture(scope="module")
def dx_runs(hotlib, opool, files):
    pairs = duplex_batch()
    for _, s1, s2 in pairs:
        opool.duplex(s1, s2), opool.inference(s1), opool.inference(s2)
    out = {}
    for name, mode, path in MODES:
        c = context(files["scrambled"], mode)
        try:
            out[name] = run_duplex(c, pairs, path, CF_KERNEL[name])
        finally:
            c.close()
    return out


def check_both_logz(pairs, res, opool, what):
    """the inside and the outside log Z of the oracle against the one the kernels report (the bar of check_cf_against_the_oracle)"""
    for (name, s1, s2), r in zip(pairs, res):
        o = opool.duplex(s1, s2).result()
        tol = 1e-8 if len(s1) * len(s2) >= 257 * 300 else 1e-9
        assert abs(r["logZ"][2] - o["logZ2"][0]) < tol and abs(r["logZ"][2] - o["logZ2"][1]) < tol, (what, name, r["logZ"][2], o["logZ2"])


@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_duplex_dense_vs_oracle_under_the_scrambled_file(opool, dx_runs, name, mode, path):
    """dxl_strip8 with the fused F[0] / F[1] tables ("auto") and dx_sweep_diag ("log"): hp and both log Z of every edge shape and planted
    pair == the oracle under the same file; the folds of the same batch likewise"""
    pairs, res = duplex_batch(), dx_runs[name]
    check_cf_against_the_oracle(pairs, res, opool, name)
    check_both_logz(pairs, res, opool, name)
    for (what, s1, s2), r in zip(pairs, res):
        for s, bp, z in ((s1, r["bp1"], r["logZ"][0]), (s2, r["bp2"], r["logZ"][1])):
            o = opool.inference(s).result()
            assert abs(z - o["logZ"]) < 1e-9, (name, what, len(s))
            assert_prob_close(bp, o["post"], rel=REL, what="bp of %s, n = %d" % (what, len(s)))


@pytest.mark.parametrize("env,kernel", CF_ORGS, ids=["+".join("%s=%s" % kv for kv in env.items()) for env, _ in CF_ORGS])
def test_duplex_organisations_vs_oracle_and_default_under_the_scrambled_file(opool, dx_runs, files, env, kernel):
    pairs, base = duplex_batch(), dx_runs["auto"]
    c = context(files["scrambled"], 0, env)
    try:
        res = run_duplex(c, pairs, 1, kernel)
    finally:
        c.close()
    assert kernel != CF_KERNEL["auto"]
    check_cf_against_the_oracle(pairs, res, opool, kernel)
    check_both_logz(pairs, res, opool, kernel)
    for (what, _, _), r, r0 in zip(pairs, res, base):
        assert abs(r["logZ"][2] - r0["logZ"][2]) <= 1e-10, (kernel, what)
        assert_prob_close(r["hp"], r0["hp"], rel=1e-10, what="hp %s vs dxl_strip8: %s" % (kernel, what))


# ---- 4. accessibility
@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_region_accessibility_vs_the_clone_oracle_of_the_scrambled_rows(hotlib, files, name, mode, path):
    """up[i][w] = exp(logZ_clone(s recoded on i..i+w) - logZ(s)), both under the scrambled rows: every region of the {A,U} and {C,G}
    sequences at 1, 2, 33 and 41 letters for max_w = 1, 15 and 31 (one past the loop budget), and the planted interior loop sides of 29,
    30 and 31 letters at widths up to 32"""
    clones = {fam: wc.CloneOracle(fam, files["dir"], files["rows"], files["scrambled"]) for fam in ("AU", "CG")}
    jobs = wc.acc_jobs()
    c = context(files["scrambled"], mode)
    got = []
    try:
        c.set_region_accessibility(True)
        for fam, seq, W, entries in jobs:
            c.set_max_w(W)
            _, up, _ = c.fold(seq)
            assert c.last_path() == path, (fam, len(seq), W)
            got.append(np.asarray(up).reshape(len(seq), W))
    finally:
        c.close()
    ref = {}
    with ThreadPoolExecutor(max_workers=8) as pool:
        for fam, seq, W, entries in jobs:
            clones[fam].logz(seq)
            missing = [e for e in entries if (fam, seq, e) not in ref]
            for e, v in zip(missing, pool.map(lambda e: region_up(clones[fam], seq, e[0], e[1]), missing)):
                ref[(fam, seq, e)] = v
    for (fam, seq, W, entries), up in zip(jobs, got):
        assert_prob_close(np.array([up[i, w] for i, w in entries]), np.array([ref[(fam, seq, e)] for e in entries]), rel=ACC_REL, abs_floor=ACC_FLOOR,
                          what="%s %s n=%d max_w=%d" % (name, fam, len(seq), W))


# ---- 5. the rows no derivation reads
# (name, rh_set_mode, switches, region accessibility with fifteen widths, rh_last_path, fold kernels, block products, duplex path and kernel)
BYTES_CONFIGS = [
    ("auto", 0, {}, True, 1, STRIPS, FAR_PK, 1, CF_KERNEL["auto"]),
    ("log", 1, {}, True, 2, KERNELS["log"], None, 2, CF_KERNEL["log"]),
    ("RH_SMALL=1", 0, {"RH_SMALL": "1"}, False, 1, STRIPS, FAR_PK, 1, CF_KERNEL["auto"]),
    ("RH_DX_STRIP=0", 0, {"RH_DX_STRIP": "0"}, True, 1, STRIPS, FAR_PK, 1, "dxl_sweep4"),
]
assert ({"RH_DX_STRIP": "0"}, "dxl_sweep4") in CF_ORGS


def bytes_batch():
    """the duplex inputs (behind their dummy), then 64 letter fillings and six folds as 35 pairs"""
    letters = [c.seq for c in wc.letter_cases()]
    picked = letters[::14] + letters[-1:] + wc.fold_seqs() + wc.fold_seqs(far2=True)[:1]
    assert len(picked) == 64 + 6
    return [(s1, s2) for _, s1, s2 in duplex_batch()] + [(picked[q], picked[q + 1]) for q in range(0, len(picked), 2)]


def bytes_run(param_file, mode, env, acc, path, kernels, far, dx_path, dx_kernel, what):
    """the batch on a fresh context, with the path, the kernel names and the empty fallback lists asserted: (results, launch counts)"""
    pairs = bytes_batch()
    c = context(param_file, mode, env)
    try:
        if acc:
            c.set_region_accessibility(True)
            c.set_max_w(15)
        c.batch_upload(pairs)
        c.batch_compute()
        assert_ran(c, path, kernels, what, far)
        assert_dx_ran(c, dx_path, dx_kernel, what)
        return [c.batch_results(p) for p in range(len(pairs))], tuple(c.batch_timings()[1])
    finally:
        c.close()


@pytest.mark.parametrize("what,mode,env,acc,path,kernels,far,dx_path,dx_kernel", BYTES_CONFIGS, ids=[b[0] for b in BYTES_CONFIGS])
def test_moving_the_never_read_rows_changes_no_byte(hotlib, files, what, mode, env, acc, path, kernels, far, dx_path, dx_kernel):
    """372 rows (160 terminal_mismatch, 40 + 40 dangle, 115 helix_stacking, 10 helix_closing, 7 base_pair) have non-complementary
    letters in a pair slot; the oracle never reads them (tests/test_contrafold_weights_cpu.py).  A kernel that did -- a wrong letter in
    a pair slot, an unmasked non-pair -- computes exp(0) = 1 under the bundled file and is invisible there.  Two contexts whose files
    differ by 0.3 in exactly those rows: bp1, bp2, up1, up2, hp and log Z of every pair have the same bytes, with the path and the
    kernel names of each configuration asserted (RH_DX_STRIP=0 must report dxl_sweep4).

    Region accessibility with fifteen widths is on except under RH_SMALL=1: a context with accessibility on and max_w > 1 keeps every
    sequence in the sweeps (staging.hip puts none on the small-fold list), so that configuration runs with the option off, and that
    lin_small_fold ran is asserted against a default context on the same batch: other launch counts, and other bits of bp on sequences
    of 8..109 letters (the kernel names are the default's: the sweeps still run for the longer sequences)."""
    pairs = bytes_batch()
    assert len(pairs) >= len(duplex_batch()) + 32
    a_res, a_launches = bytes_run(files["scrambled"], mode, env, acc, path, kernels, far, dx_path, dx_kernel, what)
    b_res, b_launches = bytes_run(files["unread"], mode, env, acc, path, kernels, far, dx_path, dx_kernel, what + ", never-read rows moved")
    assert a_launches == b_launches
    for p, (a, b) in enumerate(zip(a_res, b_res)):
        for key in ("bp1", "bp2", "up1", "up2", "hp", "logZ"):
            assert a[key].tobytes() == b[key].tobytes(), (what, "pair %d (%d x %d letters)" % ((p,) + tuple(len(s) for s in pairs[p])), key)
        assert a["up1"].shape == ((len(pairs[p][0]), 15) if acc else (len(pairs[p][0]),))
    if "RH_SMALL" in env:
        d_res, d_launches = bytes_run(files["scrambled"], mode, {}, acc, path, kernels, far, dx_path, dx_kernel, "default, accessibility off")
        small = [(p, k) for p, pr in enumerate(pairs) for k in (0, 1) if 8 <= len(pr[k]) <= 109]
        changed = sum(not np.array_equal(a_res[p]["bp%d" % (k + 1)], d_res[p]["bp%d" % (k + 1)]) for p, k in small)
        print("RH_SMALL=1: launches %r against %r, %d of %d small sequences with other bits of bp" % (a_launches, d_launches, changed, len(small)))
        assert len(small) >= 64 and a_launches != d_launches and changed > 0, "lin_small_fold did not run"
        for p, k in small:      # (and it is the same model: 1e-10 against the sweeps, as in (2))
            assert_prob_close(a_res[p]["bp%d" % (k + 1)], d_res[p]["bp%d" % (k + 1)], rel=1e-10, what="lin_small_fold against the sweeps, pair %d" % p)


# ---- 6. the single-call entries
@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_single_call_entries_build_their_tables_from_the_same_file(opool, runs, dx_runs, files, name, mode, path):
    """rh_bpp, rh_duplex and rh_fold with widths on one letter filling and one fold, against the batch results of (1) and (3).  Those
    batches ran at width 1, so they pin bp, log Z and column 0 of up; widths 2..15 of the single call are compared with a batch of the
    same context and option (rel 1e-6, floor 1e-11), which the accessibility test above pins to the clone oracle."""
    seqs = [wc.letter_cases()[500].seq, wc.fold_seqs()[2]]
    pairs = duplex_batch()
    c = context(files["scrambled"], mode)
    try:
        for s in seqs:
            bp, z = c.bpp(s)
            assert_ran(c, path, KERNELS[name] if name == "log" or len(s) >= 40 else PAIR_KERNELS, "alone, n = %d" % len(s))
            assert abs(z - runs[name][s].z) < 1e-9
            assert_prob_close(bp, runs[name][s].bp, rel=REL, what="rh_bpp against the batch, n = %d" % len(s))
        for k in (2, len(pairs) - 1):       # an edge shape and a planted pair
            _, s1, s2 = pairs[k]
            hp, z = c.duplex(s1, s2)
            assert abs(z - dx_runs[name][k]["logZ"][2]) < 1e-9
            assert_prob_close(hp, dx_runs[name][k]["hp"], rel=REL, what="rh_duplex against the batch: " + pairs[k][0])
        c.set_region_accessibility(True)
        c.set_max_w(15)
        for s in seqs:
            bp, up, z = c.fold(s)
            assert c.last_path() == path and abs(z - runs[name][s].z) < 1e-9
            assert_prob_close(bp, runs[name][s].bp, rel=REL, what="rh_fold against the batch, n = %d" % len(s))
            assert np.abs(up[:, 0] - runs[name][s].up).max() < 2e-6, len(s)
            assert abs(z - opool.inference(s).result()["logZ"]) < 1e-9
            c.batch_upload([(s, s)])
            c.batch_compute()
            assert up.shape == (len(s), 15) and c.last_path() == path
            assert_prob_close(up, c.batch_results(0)["up1"], rel=ACC_REL, abs_floor=ACC_FLOOR, what="rh_fold widths against the batch, n = %d" % len(s))
    finally:
        c.close()


# ---- 7. param_file is not ignored
def test_a_bundled_file_context_is_another_model_on_every_input(runs, hotlib):
    seqs = default_seqs()
    c = context(None, 0)
    try:
        res = run_batches(c, seqs, 1, KERNELS["auto"], far=FAR_PK)
    finally:
        c.close()
    lo = min(abs(res[s].z - runs["auto"][s].z) for s in seqs)
    print("smallest |d log Z| between a bundled-file and a scrambled-file context over %d inputs: %.3g" % (len(seqs), lo))
    assert lo > 1e-3
