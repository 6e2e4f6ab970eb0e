"""CPU suite: the scrambled ViennaRNA-1.8 table set of tests/_vienna18_tables.py and the inputs of tests/test_gpu_vienna18_tables.py.

  1  the generator keeps what a table file must keep, is reproducible, and all three readers load its file
  2  the product's loader holds the written value of sampled entries of every table (code-0 rows, a positive dangle, every loop length)
  3  the two CPU restatements survive such tables: the oracle's DP equals its enumeration (the cases of tests/test_vienna_oracle.py) and
     ractip_amd/energy.py summed over every structure equals the oracle (the cases of tests/test_energy.py)
  4  the inputs notice: on the very inputs of the GPU tests every index mutation moves a compared quantity of every family that reads
     the table by 100 x the GPU tolerance or more -- the reference alone, so a condition on the inputs
  5  the gap this closes, as a test: under plain BL* the two mismatchI mutations leave every result of the oracle bit-identical"""
import ctypes
import math
import os

import numpy as np
import pytest

import _span_acc_cases as ac
import _span_cases as sc
import _vienna18_cases as vc
import _vienna18_tables as vt
import test_energy as ten
import test_vienna_oracle as tvo
from _oracle import ViennaOracle
from ractip_amd import energy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT = energy.KT


def w(E):
    return -E * 10.0 / KT


@pytest.fixture(scope="module")
def tables():
    return vt.scrambled(vc.SEED)


@pytest.fixture(scope="module")
def path(tables, tmp_path_factory):
    return vc.write_tables(tmp_path_factory.mktemp("vienna18"), tables)


@pytest.fixture(scope="module")
def vo(path):
    return ViennaOracle(path)


# ---- 1
def test_scrambled_tables_keep_sizes_infinities_type_7_and_the_symmetries(tables):
    B = vt.read(vt.BL)
    assert vt.symmetry_violations(B) == dict(stack=0, int11=0, int22=0), "the bundled file has the symmetries to begin with"
    assert vt.symmetry_violations(tables) == dict(stack=0, int11=0, int22=0)
    for name, shape in vt.SHAPES:
        assert tables[name].shape == shape
        assert np.array_equal(tables[name] == vt.INF, B[name] == vt.INF), name
    for name in ("stack37", "int11_37", "int21_37", "int22_37"):
        assert np.array_equal(tables[name][6], B[name][6]) and np.array_equal(tables[name][:, 6], B[name][:, 6]), name
    for name in ("mismatchH37", "mismatchI37"):
        assert np.array_equal(tables[name][6], B[name][6]), name
    for name in ("dangle5_37", "dangle3_37"):
        assert np.array_equal(tables[name][7], B[name][7]) and np.array_equal(tables[name][0], B[name][0]), name
    assert [sq for sq, _ in tables["tetraloops"]] == [sq for sq, _ in B["tetraloops"]]
    # int21 and the mismatch tables have no symmetric partner, and the scrambled ones are not accidentally symmetric either
    assert (tables["int21_37"][:6, :6] != tables["int21_37"][:6, :6].transpose(1, 0, 2, 3, 4)).mean() > 0.8    # (t1 == t2: a sixth)
    for name in ("mismatchH37", "mismatchI37"):
        assert (tables[name][:6] != tables[name][:6].transpose(0, 2, 1)).mean() > 0.7, name
        assert (tables[name][:6] != tables[name][vt.RT0[:6]]).mean() > 0.9, name


def test_scrambled_tables_are_nowhere_constant_where_bl_star_is(tables):
    B = vt.read(vt.BL)
    for name in ("stack37", "mismatchH37", "mismatchI37", "int11_37", "int21_37", "int22_37"):
        moved = tables[name][:6] != B[name][:6] if tables[name].ndim == 3 else tables[name][:6, :6] != B[name][:6, :6]
        assert moved.mean() > 0.95, (name, moved.mean())
    # the code-0 rows and columns (unknown letter) of the tables that have them
    for name in ("mismatchH37", "mismatchI37"):
        assert (tables[name][:6, 0, :] != B[name][:6, 0, :]).mean() > 0.9 and (tables[name][:6, :, 0] != B[name][:6, :, 0]).mean() > 0.9, name
    assert (tables["int11_37"][:6, :6, 0] != B["int11_37"][:6, :6, 0]).mean() > 0.9
    assert (tables["int21_37"][:6, :6, 0] != B["int21_37"][:6, :6, 0]).mean() > 0.9
    for name in ("hairpin37", "bulge37", "internal_loop37"):       # every length
        finite = B[name] != vt.INF
        assert (tables[name][finite] != B[name][finite]).mean() > 0.9, name
        assert np.abs(tables[name][finite] - B[name][finite]).max() <= 40
    assert not np.array_equal(tables["MLparams"], B["MLparams"]) and not np.array_equal(tables["ninio"], B["ninio"])
    assert sum(1 for (_, a), (_, b) in zip(tables["tetraloops"], B["tetraloops"]) if a != b) >= 25
    m, cap = tables["ninio"]
    assert 1 <= -(-cap // m) <= 30 and 30 * m > cap, "the ninio cap is reached inside an asymmetry of 30"
    for name in ("dangle5_37", "dangle3_37"):
        d = tables[name][1:7, 1:]
        assert (d < -9).any() and ((d > 0) & (d < 12.28)).any(), (name, "identity part and positive ramp of SMOOTH")
    both = np.concatenate([tables["dangle5_37"][1:7, 1:].ravel(), tables["dangle3_37"][1:7, 1:].ravel()])
    assert ((both > -8.66) & (both < 0)).any(), "the negative ramp"
    assert (both > 12.28).any(), "a dangle past the ramp, where SMOOTH and the clip agree on 0"


def test_scrambled_tables_are_reproducible_and_round_trip(tables, path):
    assert vt.same(tables, vt.scrambled(vc.SEED)) and not vt.same(tables, vt.scrambled(vc.SEED + 1))
    assert vt.same(vt.read(path), tables)
    assert vt.same(vt.read(vt.BL), vt.read(vt.write(os.path.join(os.path.dirname(path), "bl_again.params"), vt.read(vt.BL))))


@pytest.fixture(scope="module")
def hooks(hotlib):
    lib = ctypes.CDLL(os.path.join(ROOT, "ractip_amd", "libractip_hot.so"))
    lib.rh_debug_vienna_value.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int] + [ctypes.c_int] * 5 + [
        ctypes.POINTER(ctypes.c_double)]
    lib.rh_debug_vienna_value.restype = ctypes.c_int
    lib.rh_debug_vienna_cell.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_double)]
    lib.rh_debug_vienna_cell.restype = ctypes.c_int

    def value(param, table, i=0, j=0, k=0, l=0, use_bl=True):
        """as a context created with param_file installs it: the bundled BL* file, then the file on top"""
        out = ctypes.c_double()
        rc = lib.rh_debug_vienna_value(None, 1 if use_bl else 0, vt.BL.encode(), param.encode(), 0, table, i, j, k, l, ctypes.byref(out))
        assert rc == 0, (rc, table, i, j, k, l)
        return out.value

    def cell(param, table, *idx):
        out = ctypes.c_double()
        idx = tuple(idx) + (0,) * (6 - len(idx))
        assert lib.rh_debug_vienna_cell(param.encode(), table, *idx, ctypes.byref(out)) == 0, (table, idx)
        return out.value
    return value, cell


def test_all_three_readers_load_the_file(tables, path, vo, hooks):
    value, _ = hooks
    assert vo.m
    M = energy.Model(path)
    assert np.array_equal(M.mmI[1:], tables["mismatchI37"]) and np.array_equal(M.int21[1:, 1:], tables["int21_37"])
    assert (M.ml_base, M.ml_closing, M.ml_intern, M.tau) == tuple(tables["MLparams"]) and (M.ninio, M.max_ninio) == tuple(tables["ninio"])
    assert value(path, 22) == 1 and value(path, 22, use_bl=False) == 1, "a flat dump keeps the 1.8 semantics, with or without BL* below it"


# ---- 2
def test_the_loader_holds_the_written_value_of_every_table(tables, path, hooks):
    """rh_debug_vienna_value (the hook of tests/test_vienna_par.py) and rh_debug_vienna_cell (of tests/test_bl_cells.py, int21 / int22):
    a seeded sample of every table plus the entries named above; log Boltzmann weights -E * 10 / kT, dangles clipped for the duplex
    ends (tables 26 / 27) and smoothed for the stems (table 15)."""
    value, cell = hooks
    T = tables
    rng = np.random.RandomState(5)
    close = lambda got, want: got == pytest.approx(want, abs=1e-12)
    for tab, name in ((10, "mismatchI37"), (11, "mismatchH37")):
        cells = [tuple(c) for c in rng.randint([1, 0, 0], [7, 5, 5], (40, 3))] + [(t, 0, b) for t in (1, 4, 6) for b in range(5)] + [(t, a, 0) for t in (2, 3, 5) for a in range(5)]
        for t, a, b in cells:
            assert close(value(path, tab, t, a, b), w(T[name][t - 1, a, b])), (name, t, a, b)
    for t, t2 in [tuple(c) for c in rng.randint(1, 7, (30, 2))]:
        assert close(value(path, 24, t, t2), w(T["stack37"][t - 1, t2 - 1])), (t, t2)
        assert close(value(path, 23, 7, t, t2), w(T["bulge37"][1] + T["stack37"][t - 1, t2 - 1])), (t, t2)
        for a, b in [tuple(c) for c in rng.randint(0, 5, (4, 2))] + [(0, 3), (2, 0)]:
            assert close(value(path, 25, t, t2, a, b), w(T["int11_37"][t - 1, t2 - 1, a, b])), (t, t2, a, b)
        for a, b, c in [tuple(x) for x in rng.randint(0, 5, (6, 3))] + [(0, 1, 2), (3, 0, 4), (2, 4, 0)]:
            assert cell(path, 2, t, t2, a, b, c) == pytest.approx(T["int21_37"][t - 1, t2 - 1, a, b, c], abs=1e-9), (t, t2, a, b, c)
        for a, b, c, d in [tuple(x) for x in rng.randint(1, 5, (8, 4))]:
            assert cell(path, 3, t, t2, a, b, c, d) == pytest.approx(T["int22_37"][t - 1, t2 - 1, a - 1, b - 1, c - 1, d - 1], abs=1e-9), (t, t2, a, b, c, d)
    positive = 0
    tau = int(T["MLparams"][3])
    for t in range(1, 7):
        for a in range(1, 5):
            d5, d3 = int(T["dangle5_37"][t, a]), int(T["dangle3_37"][t, a])
            positive += d5 > 0
            assert close(value(path, 26, t, a), w(min(d5, 0))) and close(value(path, 27, t, a), w(min(d3, 0))), (t, a)
            for b in range(1, 5):
                d3b = int(T["dangle3_37"][t, b])
                want = (energy._smooth(-float(d5)) + energy._smooth(-float(d3b))) * 10.0 / KT + (w(tau) if t > 2 else 0.0)
                assert close(value(path, 15, t, a, b), want) and close(value(path, 16, t, a, b), want), (t, a, b)
        assert close(value(path, 15, t, 0, 0), w(tau) if t > 2 else 0.0), "code 0 is no neighbour"
    assert positive >= 3
    m, cap = (int(x) for x in T["ninio"])
    for l1 in range(31):
        for l2 in range(31 - l1):
            nl, ns = max(l1, l2), min(l1, l2)
            if nl <= 2 and not (ns == 0 and nl == 2):
                continue
            E = T["bulge37"][nl] if ns == 0 else T["internal_loop37"][l1 + l2] + min(cap, (nl - ns) * m)
            assert close(value(path, 17, l1, l2), w(E)), (l1, l2)
    for u in range(3, 31):
        assert close(value(path, 23, 6, u), w(T["hairpin37"][u])), u
    ml = [int(x) for x in T["MLparams"]]
    assert close(value(path, 23, 4), w(ml[0])) and close(value(path, 23, 2), w(ml[1] + ml[2])) and close(value(path, 23, 3), w(ml[2]))
    assert close(value(path, 23, 0), w(ml[3]))
    for sq, e in T["tetraloops"]:
        code = 0
        for ch in sq:
            code = code * 4 + "ACGU".index(ch)
        assert close(value(path, 19, code), w(e)), sq


# ---- 3
def test_log_z_per_letter_stays_inside_the_scale_ladder(vo):
    """log Z per letter within 0.2 .. 0.5, what the scale-exponent ladder of the linear kernels is built for: on random ACGU of 100,
    200 and 300 letters and on every fold input of the GPU tests (40 .. 130 letters: 0.26 .. 0.37).  The figure grows with the length:
    a random sequence of 40 letters can lie just below 0.2 (0.19 measured on one, where BL* gives 0.13), so the lower bound is not
    asserted for random sequences shorter than 100 letters, only for the 40-letter input that is used; the upper bound, the one the
    ladder depends on, holds at every length."""
    rng = np.random.RandomState(0)
    for n in (40, 66, 100, 200, 300):
        for _ in range(3):
            z = vo.mccaskill("".join(rng.choice(list("ACGU"), n)))["logZ"] / n
            assert (0.2 if n >= 100 else 0.0) <= z <= 0.5, (n, z)
    for s1, s2 in vc.fold_pairs():
        for s in (s1, s2):
            z = vo.mccaskill(s)["logZ"] / len(s)
            print("fold input of %d letters: log Z per letter %.3f" % (len(s), z))
            assert 0.2 <= z <= 0.5, (len(s), z)


def test_oracle_dp_equals_its_enumeration_under_the_scrambled_tables(vo):
    """the cases of tests/test_vienna_oracle.py: pf_duplex, fold (with accessibility), cofold, constraints"""
    tvo.test_dp_equals_bruteforce_enumeration(vo)
    tvo.test_mccaskill_equals_bruteforce_enumeration(vo)
    tvo.test_cofold_equals_bruteforce_enumeration(vo)
    tvo.test_structure_constraints_equal_bruteforce(vo)


@pytest.mark.parametrize("s,W", tvo.WIDE_WIDTH_CASES, ids=["%d-w%d" % (len(s), W) for s, W in tvo.WIDE_WIDTH_CASES])
def test_oracle_wide_widths_equal_enumeration_under_the_scrambled_tables(vo, s, W):
    tvo.test_mccaskill_wide_widths_equal_bruteforce_enumeration(vo, s, W)


def test_energy_summed_over_every_structure_is_the_oracle_under_the_scrambled_tables(vo, path):
    """the cases of tests/test_energy.py with energy.Model(path)"""
    M = energy.Model(path)
    rng = np.random.RandomState(2)
    seqs = ["GGGAAACCC", "GGCGAAAGCC", "GGGAAACCCAGG"] + ["".join(rng.choice(list("ACGU"), n, p=[.15, .35, .35, .15])) for n in (8, 11, 13)]
    kT = KT / 1000.0
    for s in seqs:
        z = sum(math.exp(-e / kT) for e in (energy.energy_of_structure(s, st, model=M) for st in ten.all_structures(len(s))) if math.isfinite(e))
        assert abs(math.log(z) - vo.mccaskill(s)["logZ"]) < 1e-10, s
    for s1, s2 in (("GGGAC", "GUCCC"), ("GGGAAACC", "GGUCCC"), ("GCGCA", "UGCGCAA")):
        z = sum(math.exp(-e / kT) for e in (energy.energy_of_structure(s1 + s2, st, cut=len(s1), model=M) for st in ten.all_structures(len(s1 + s2)))
                if math.isfinite(e))
        assert abs(math.log(z) - vo.cofold(s1, s2)["logZ"]) < 1e-10, (s1, s2)


def test_the_span_reference_cache_is_keyed_by_the_table_file(path, tmp_path):
    seq = vc.span_seq(40)
    a, b = sc.masked(seq, 20, params=path), sc.masked(seq, 20)
    assert abs(a["logZ"] - b["logZ"]) > 1e-3
    assert sc.masked(seq, 20, params=path) is a and sc.masked(seq, 20) is b and sc.oracle(path) is not sc.oracle()
    # ... and by what the file holds: another table set written under one name is another reference
    M, _ = vt.mutants(vt.scrambled(vc.SEED))["ML_closing <-> ML_intern"]
    again = vc.write_tables(tmp_path, name="one_name.params")
    first = sc.masked(seq, 20, params=again)
    assert first["logZ"] == a["logZ"]
    assert vc.write_tables(tmp_path, M, "one_name.params") == again
    second, wide = sc.masked(seq, 20, params=again), ac.masked_acc(seq, 20, 3, params=again)
    assert second is not first and abs(second["logZ"] - first["logZ"]) > 1e-6 and wide["logZ"] == second["logZ"]


# ---- 4
@pytest.fixture(scope="module")
def base(path):
    return vc.oracle_results(path)


@pytest.fixture(scope="module")
def kept(base):
    cases = vc.planted_cases()
    return vc.planted_kept(cases, [r["post"] for _, r in base["planted"]])


def test_the_half_rule_leaves_out_at_most_five_percent_of_the_planted_loops(base, kept):
    """a planted case is compared where the oracle puts more than 0.5 on the closing or the enclosed pair; every shape and every
    pair type keeps cases"""
    cases = vc.planted_cases()
    print("planted loops: %d of %d kept" % (len(kept), len(cases)))
    assert len(kept) >= (1 - vc.PLANTED_MAY_DROP) * len(cases)
    whats = [cases[k].what for k in kept]
    for l1, l2 in vc.LOOPS:
        assert sum(1 for x in whats if " %dx%d " % (l1, l2) in x and x.startswith("pair types")) >= 24, (l1, l2)
    for l1, l2 in vc.TABULATED:
        assert sum(1 for x in whats if " %dx%d " % (l1, l2) in x and x.startswith("filling")) >= 0.9 * 4 ** (l1 + l2), (l1, l2)


FAMILIES = {"fold": ("fold", "planted", "cofold", "span", "span planted"), "duplex": ("duplex",)}
MUTANT_NAMES = sorted(vt.mutants(vt.read(vt.BL)))


def family_movement(a, b, fam, kept):
    keep = set(kept)
    return max(vc.movement(x[1], y[1]) for k, (x, y) in enumerate(zip(a[fam], b[fam])) if fam != "planted" or k in keep)


@pytest.mark.parametrize("name", MUTANT_NAMES)
def test_the_inputs_notice_every_index_mutation(tables, path, base, kept, name):
    """The oracle under the scrambled tables against the oracle under the mutated scrambled tables, on the inputs of
    tests/test_gpu_vienna18_tables.py: in every family that reads the table, log Z or a probability of at least 1e-6 moves by
    MARGIN = 100 tolerances of the GPU test or more.  A family's figure is the largest movement over its inputs and quantities
    (vc.movement); the smallest of all families and mutants measured is 6.1e5 tolerances, int21 letters 1 <-> 3 on the two-molecule
    ensemble (DESIGN.md 5.1m lists the smallest family of every mutant).  Every mutant has a file of its own: the span references
    are cached per file."""
    M, reads = vt.mutants(tables)[name]
    assert not vt.same(M, tables)
    families = [f for r in reads for f in FAMILIES[r]]
    own = "mutant_%s.params" % "".join(ch if ch.isalnum() else "_" for ch in name)      # a file of its own
    got = vc.oracle_results(vc.write_tables(os.path.dirname(path), M, own), families=families)
    for fam in families:
        mv = family_movement(base, got, fam, kept)
        print("%-28s %-8s moves by %.3g tolerances" % (name, fam, mv))
        assert mv >= vc.MARGIN, (name, fam, mv)


def test_the_mutant_list_is_the_one_the_gap_was_measured_with(tables):
    names = set(vt.mutants(tables))
    assert len(names) == 15 and set(vt.MISMATCH_I_MUTANTS) <= names
    assert sum(n.startswith("int21") for n in names) == 4 and sum(n.startswith("int22") for n in names) == 4
    assert {"mismatchH letter swap", "mismatchH type <-> rtype", "dangle5 <-> dangle3", "int11 letter swap", "ML_closing <-> ML_intern"} <= names


# ---- 5
def test_under_bl_star_the_mismatch_i_mutations_change_no_bit(tmp_path):
    """The gap, recorded: BL*'s mismatchI is invariant under the transposition of its letters and under type <-> rtype, so on the same
    inputs the oracle's results under the mutated BL* file are the bits of the plain one.  TXO / TXI, the FCX decoration of the far
    products, the generic weights of span_acc_gaps and the duplex kernels' mmI could have mixed these up under every BL* test."""
    B = vt.read(vt.BL)
    plain = vc.oracle_results(vt.BL)
    muts = vt.mutants(B)
    for name in vt.MISMATCH_I_MUTANTS:
        M, _ = muts[name]
        real = (slice(0, 6), slice(1, 5), slice(1, 5))     # pair types 1..6 on the letters A..U: all these inputs read but for one N
        assert np.array_equal(M["mismatchI37"][real], B["mismatchI37"][real]), name
        got = vc.oracle_results(vc.write_tables(tmp_path, M, "bl_%s.params" % "".join(ch if ch.isalnum() else "_" for ch in name)))
        for fam in plain:
            for (what, a), (_, b) in zip(plain[fam], got[fam]):
                for key in a:
                    assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (name, what, key)
    for name in ("mismatchH letter swap", "int11 letter swap", "dangle5 <-> dangle3"):
        assert not vt.same(muts[name][0], B), name
