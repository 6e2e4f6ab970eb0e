"""CPU tests (no GPU) behind tests/test_gpu_unknown_letters.py: the references that the kernels are compared with are themselves pinned on
inputs with letters other than A, C, G and U, and every such input is proven to move its reference by at least 100 x the GPU tolerance.

  * oracle/cf_oracle.c == the reference's own engines in double precision (tests/golden/contrafold_unknown_letters.npz, written by
    oracle/gen_golden.py with GOLDEN_ONLY=unknown_letters; live as well where oracle/_ref has been built);
  * oracle/vienna_oracle.c and oracle/vienna2x_oracle.c == enumeration of every structure on role inputs of at most 16 letters (PARITY
    UNPINNED against ViennaRNA, which is absent: enumeration under the same energy functions is the reference);
  * discrimination: per role and model, how far the substitution moves log Z and the posteriors;
  * the product's two encodings (a stand-alone host program, tools/letter_codes_check.cpp) == the encodings of the oracles on all 256
    byte values."""
import collections
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import _alphabet_cases as ac
import _contrafold_cases as cf
import _vienna2x_cases as v2cases
from _oracle import OraclePool, Reference, Vienna2xOracle, tri_offset
from _vienna2x_cases import v2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "contrafold_unknown_letters.npz")
TS = v2cases.TABLES


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    p.tables2x(TS, v2cases.tables())
    yield p
    p.close()


# ---- 1. the inputs are what their names say
def test_every_input_differs_from_its_planted_base_in_the_named_letters_only():
    sets = {"cf": ac.cf_role_set(), "cf short": ac.cf_short_set(), "bl": ac.bl_role_set(), "2.x": ac.v2_role_set(),
            "toy bl": ac.toy_role_set(ac.BL_CODED), "toy 2.x": ac.toy_role_set(ac.V2_CODED)}
    for name, subs in sets.items():
        assert len({s.seq for s in subs}) == len(subs), name
        for s in subs:
            assert len(s.seq) == len(s.base) <= 449 and set(s.base) <= set("ACGU"), s.what
            assert [k + 1 for k in range(len(s.seq)) if s.seq[k] != s.base[k]] == sorted(s.pos) and len(s.pos) >= 1, s.what
            assert {s.seq[p - 1] for p in s.pos} == {s.letter} and s.letter in "NTnX-", s.what
            assert len(s.pos) == 1 or s.role == "loop sides", s.what
        letters = collections.Counter(s.letter for s in subs)
        assert letters["N"] > letters["T"] > 0 and letters["n"] > 0, (name, letters)
    assert collections.Counter(s.letter for s in sets["bl"])["X"] == 1 and collections.Counter(s.letter for s in sets["bl"])["-"] == 1
    for name in ("cf", "cf short", "bl", "2.x"):       # every role on every loop it exists on
        seen = collections.defaultdict(set)
        for s in sets[name]:
            seen[s.role].add((s.case.l1, s.case.l2))
        for role in ("hairpin first", "hairpin last", "before the outer stem", "after the outer stem", "outer stem middle",
                     "inner stem middle", "lead 0, after the outer stem", "tail 0, before the outer stem"):
            assert seen[role] == set(ac.LOOPS), (name, role)
        assert seen["closing pair, 5' inside"] == {lp for lp in ac.LOOPS if lp[0]}, name
        assert seen["closing pair, 3' inside"] == {lp for lp in ac.LOOPS if lp[1]}, name
        assert seen["enclosed pair, 5' outside"] >= {lp for lp in ac.LOOPS if lp[0] > 1}, name      # (l1 = 1: the same letter)
        assert seen["enclosed pair, 3' outside"] >= {lp for lp in ac.LOOPS if lp[1] > 1}, name
        assert seen["loop sides"] >= {lp for lp in ac.LOOPS if sum(lp) > 1 and min(lp) > 0}, name
    for name, coded in (("bl", ac.BL_CODED), ("2.x", ac.V2_CODED)):
        roles = {s.role for s in sets[name]}
        assert roles >= {"hairpin letter %d of %d" % (k + 1, len(hp)) for _, hp, _ in coded for k in range(len(hp))}, name
    assert {len(hp) for _, hp, _ in ac.V2_CODED} == {3, 4, 6} and {len(hp) for _, hp, _ in ac.BL_CODED} == {4}
    for name in ("bl", "2.x"):
        assert sum(s.role.startswith("multiloop, ") for s in sets[name]) == 3, name


def test_contrafold_inputs_sit_on_the_strip_edges_and_at_the_small_kernel_lengths():
    """The closing pair on columns 57 and 58, its diagonal in a strip (d >= 32) on every residue mod 8, both tails; lead = 0 puts the
    outer stem on letter 1.  The short set: 41..79 letters."""
    subs = ac.cf_role_set()
    placed = [s for s in subs if s.case.lead]
    assert {cf.coords(s.case)["a"] for s in placed} == {57, 58} and {cf.coords(s.case)["a"] for s in subs if not s.case.lead} == {8}
    assert {cf.coords(s.case)["d"] % cf.KD for s in placed} == set(range(8))
    assert min(cf.coords(s.case)["d"] for s in subs) >= cf.BOOT
    assert {s.case.tail for s in placed} >= {0, cf.SHORT_TAIL, cf.LONG_TAIL}
    for s in subs:
        assert cf.planted(s.case.lead, s.case.l1, s.case.l2, s.case.h, s.case.tail) == s.base and len(s.base) <= cf.NMAX, s.what
        g = cf.coords(s.case)
        n = len(s.seq)
        full = cf.inside_group(n, g["i"], g["d"])[2]
        assert full == (s.case.tail >= 119), s.what         # the long tail: an interior group, the unmasked staging path
    short = ac.cf_short_set()
    assert min(len(s.seq) for s in short) >= 41 and max(len(s.seq) for s in short) <= 79
    assert {s.role for s in short} == {s.role for s in subs}
    for rot in range(4):
        assert {s.role for s in ac.thinned(subs, rot)} == {s.role for s in subs}, rot


def test_vienna_inputs_are_the_planted_inputs_of_the_2x_cases():
    for l1, l2 in ac.LOOPS:
        assert ac.vplanted(2, l1, l2).seq == v2cases.planted(l1, l2)[0]
        c = ac.vplanted(2, l1, l2, stems=ac.AU_LOOP)
        g = ac.vcoords(c)
        s = " " + c.seq
        assert s[g["a"]] + s[g["b"]] == "AU" and s[g["a2"]] + s[g["b2"]] == "AU" and len(c.seq) == len(ac.vplanted(2, l1, l2).seq)
        assert s[g["h1"]:g["hn"] + 1] == "AAAA" and s[g["end"]] == "C" and g["end"] == len(c.seq) - 2
    T = v2cases.tables()
    for i5, hp, i3 in ac.V2_CODED:
        assert i5[-1] + hp + i3[0] in {**T["Triloops"], **T["Tetraloops"], **T["Hexaloops"]}
    par = open(os.path.join(ROOT, "ractip_amd", "data", "vienna_bl_star.params")).read()
    for i5, hp, i3 in ac.BL_CODED:
        assert "\n%s " % (i5[-1] + hp + i3[0]) in par


def test_mixed_and_n_run_generators():
    s = "".join(ac.mixed_seqs(1, [4000]))
    up = s.upper()
    assert set(up) == set("ACGUNT") and 0.05 < up.count("N") / 4000 < 0.07 and 0.02 < up.count("T") / 4000 < 0.04
    assert 0.07 < sum(ch.islower() for ch in s) / 4000 < 0.09
    assert ac.mixed_seqs(1, [50, 60]) == ac.mixed_seqs(1, [50, 60])
    for n, a, b in ((420, 110, 310), (420, 1, 200), (130, 40, 75)):
        r = ac.n_run(n, a, b)
        assert len(r) == n and r[a - 1:b] == "N" * (b - a + 1) and set(r[:a - 1] + r[b:]) <= set("ACGU") and r == ac.n_run(n, a, b)


# ---- 2. oracle/cf_oracle.c against the reference's engines
def sparse(post, idx):
    return post.ravel()[idx]


def test_contrafold_oracle_matches_the_reference_engines_on_unknown_letters(opool):
    """log Z to 1e-9 and the recorded posteriors to 1e-9 relative: every role x loop input (both stem posteriors), 12 mixed sequences
    of 40..160 letters and 6 mixed pairs (the entries above 1e-3)."""
    gold = np.load(FIXTURE, allow_pickle=False)
    subs, seqs, pairs = ac.fixture_inputs()
    assert [s.decode() for s in gold["role/seq"]] == [s.seq for s in subs]
    assert [s.decode() for s in gold["mixed/seq"]] == seqs and len(seqs) == 12 and 40 == min(map(len, seqs)) and max(map(len, seqs)) == 160
    assert [(a.decode(), b.decode()) for a, b in zip(gold["pair/s1"], gold["pair/s2"])] == pairs and len(pairs) == 6
    for s in subs:
        opool.inference(s.seq)
    for s in seqs:
        opool.inference(s)
    for a, b in pairs:
        opool.duplex(a, b)
    worst_z = worst_p = 0.0
    for k, s in enumerate(subs):
        o = opool.inference(s.seq).result()
        p = cf.stem_probs(o["post"], s.case)
        assert abs(o["logZ"] - gold["role/logZ"][k]) < 1e-9, s.what
        for got, want in zip(p, (gold["role/outer"][k], gold["role/inner"][k])):
            assert abs(got - want) <= 1e-9 * want, (s.what, got, want)
            worst_p = max(worst_p, abs(got - want) / want if want else 0.0)
        worst_z = max(worst_z, abs(o["logZ"] - gold["role/logZ"][k]))
    for k, s in enumerate(seqs):
        o = opool.inference(s).result()
        idx, val = gold["mixed/%d/idx" % k], gold["mixed/%d/val" % k]
        assert abs(o["logZ"] - gold["mixed/logZ"][k]) < 1e-9, k
        assert len(idx) >= 20 and np.array_equal(np.flatnonzero(o["post"] > 1e-3), idx), k
        assert (np.abs(sparse(o["post"], idx) - val) <= 1e-9 * val).all(), k
    for k, (a, b) in enumerate(pairs):
        o = opool.duplex(a, b).result()
        idx, val = gold["pair/%d/idx" % k], gold["pair/%d/val" % k]
        assert np.abs(o["logZ2"] - gold["pair/logZ2"][k]).max() < 1e-9, k
        assert len(idx) >= 20 and (np.abs(sparse(o["post"], idx) - val) <= 1e-9 * val).all(), k
    print("oracle against the reference on %d role inputs: max |dlogZ| %.3g, max relative error of a stem posterior %.3g"
          % (len(subs), worst_z, worst_p))


def test_contrafold_oracle_matches_the_reference_engines_live_where_they_are_built(opool):
    """the same against oracle/_ref itself (built where the reference's sources are): a thinned role set, the mixed sequences and pairs"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref_contrafold.so")):
        pytest.skip("oracle/_ref is not built here; the fixture test covers the same inputs")
    ref = Reference()       # (a library that is there and does not load is an error, not a skip)
    subs, seqs, pairs = ac.fixture_inputs()
    for s in [x.seq for x in subs[::7]] + seqs:
        o, r = opool.inference(s).result(), ref.inference(s)
        assert abs(o["logZ"] - r["logZ"]) < 1e-9
        big = r["post"] > 1e-12
        assert (np.abs(o["post"] - r["post"])[big] <= 1e-9 * r["post"][big]).all() and np.abs(o["post"] - r["post"])[~big].max() <= 1e-12
    for a, b in pairs:
        o, r = opool.duplex(a, b).result(), ref.duplex(a, b)
        assert np.abs(o["logZ2"] - r["logZ2"]).max() < 1e-9
        big = r["post"] > 1e-12
        assert (np.abs(o["post"] - r["post"])[big] <= 1e-9 * r["post"][big]).all()


# ---- 3. the Vienna restatements against enumeration
CO_TOYS = [("GGGAAN", "CCCAG"), ("GGGAA", "NCCCAG"), ("GGGAN", "NCCC"), ("GGCAN", "TGCCA"), ("nGGGA", "ACCCn"), ("GGGAAACN", "NGUCCC")]
DX_TOYS = [("NGGGAN", "NUCCCN"), ("NGGCGAN", "NCGCCN"), ("GGGN", "NCCC"), ("NGGG", "CCCN"), ("TGGGAN", "nCCCAX"), ("GNGAG", "CUNC")]


def test_vienna_bl_restatement_equals_enumeration_on_unknown_letters(opool):
    """oracle/vienna_oracle.c: log Z, bp and up at width 4 of every toy role input, the two-molecule ensemble with N as the last letter
    of s1, as the first of s2 and both, and pf_duplex with N at both ends of both strands == enumeration, to 1e-10"""
    vo = opool.vo
    subs = ac.toy_role_set(ac.BL_CODED)
    for s in subs:
        a, b = vo.mccaskill(s.seq, max_w=4), vo.fold_bruteforce(s.seq, max_w=4)
        assert abs(a["logZ"] - b["logZ"]) < 1e-10 and abs(a["logZ_out"] - b["logZ"]) < 1e-10, s.what
        assert np.abs(a["post"] - b["post"]).max() < 1e-10 and np.abs(a["up"] - b["up"]).max() < 1e-10, s.what
        for p in s.pos:
            if s.letter != "T":      # an unknown letter is never paired
                assert a["up"][p - 1, 0] > 1 - 1e-12, s.what
    for s1, s2 in CO_TOYS:
        a, b = vo.cofold(s1, s2), vo.cofold(s1, s2, bruteforce=True)
        assert abs(a["logZ"] - b["logZ"]) < 1e-10 and np.abs(a["post"] - b["post"]).max() < 1e-10, (s1, s2)
        assert np.abs(a["hp"] - b["hp"]).max() < 1e-10 and b["hp"].max() > 1e-3, (s1, s2)
    for s1, s2 in DX_TOYS:
        a, b = vo.pf_duplex(s1, s2), vo.bruteforce(s1, s2)
        assert abs(a["logZ"] - b["logZ"]) < 1e-10 and np.abs(a["pr"] - b["pr"]).max() < 1e-10 and b["pr"].max() > 1e-3, (s1, s2)


def dense(bp, n):
    want = np.zeros((n + 1) * (n + 2) // 2)
    for (i, j), p in bp.items():
        want[tri_offset(n, i) + j] = p
    return want


def test_vienna_2x_restatement_equals_enumeration_on_unknown_letters(opool):
    """oracle/vienna2x_oracle.c and vienna2x.pf_duplex on the random table set (row 0 of every mismatch table has its own values):
    the toy role inputs with N at each position of a tri-, tetra- and hexaloop, the co-fold and duplex toys == vienna2x.brute_*"""
    T = v2cases.tables()
    for name in v2.MISMATCH_SECTIONS.values():      # an unknown neighbour selects values that no known letter selects
        for t in range(1, 8):
            assert all(not np.array_equal(T[name][t, 0], T[name][t, k]) and not np.array_equal(T[name][t, :, 0], T[name][t, :, k])
                       for k in range(1, 5)) and T[name][t, 0].any() and T[name][t, :, 0].any(), (name, t)
    o2 = Vienna2xOracle(T)
    for s in ac.toy_role_set(ac.V2_CODED):
        lz, bp, up = v2.brute_fold(T, s.seq, max_w=4)
        r = o2.fold(s.seq, 4)
        assert abs(r["logZ"] - lz) < 1e-10 and abs(r["logZ_out"] - lz) < 1e-10, s.what
        assert np.abs(r["post"] - dense(bp, len(s.seq))).max() < 1e-10 and np.abs(r["up"] - up).max() < 1e-10, s.what
    for s1, s2 in CO_TOYS:
        lz, hp = v2.brute_cofold(T, s1, s2)
        r = o2.cofold(s1, s2)
        assert abs(r["logZ"] - lz) < 1e-10 and np.abs(r["hp"] - hp).max() < 1e-10, (s1, s2)
    for s1, s2 in DX_TOYS:
        lz, pr = v2.brute_duplex(T, s1, s2)
        efw, ebk, p = v2.pf_duplex(T, s1, s2)
        assert math.isfinite(lz) and abs(efw - lz) < 1e-10 and abs(ebk - lz) < 1e-10 and np.abs(p - pr).max() < 1e-10, (s1, s2)


# ---- 4. discrimination
Z_MARGIN, P_MARGIN = 1e-7, 1e-4      # 100 x the GPU tolerances: 1e-9 * max(1, |log Z|) and 1e-6 relative


def movement(o, b):
    """(relative movement of log Z, largest relative movement of a posterior above 1e-3 in either output)"""
    dz = abs(o["logZ"] - b["logZ"]) / max(1.0, abs(b["logZ"]))
    big = (o["post"] > 1e-3) | (b["post"] > 1e-3)
    dp = float((np.abs(o["post"] - b["post"])[big] / np.maximum(o["post"], b["post"])[big]).max()) if big.any() else 0.0
    return dz, dp


def least_moved(subs, call):
    """role -> (dz, dp, what) of the input the substitution moves least; [] of the inputs under the margin"""
    for s in subs:
        call(s.seq), call(s.base)
    worst, below = {}, []
    for s in subs:
        dz, dp = movement(call(s.seq).result(), call(s.base).result())
        if s.role not in worst or max(dz / Z_MARGIN, dp / P_MARGIN) < max(worst[s.role][0] / Z_MARGIN, worst[s.role][1] / P_MARGIN):
            worst[s.role] = (dz, dp, s.what)
        if dz < Z_MARGIN and dp < P_MARGIN:
            below.append((s, dz, dp))
    return worst, below


def report(name, worst):
    print("%s: the input of each role that its substitution moves least (log Z relative to max(1, |log Z|); posteriors above 1e-3, relative)" % name)
    for role, (dz, dp, what) in worst.items():
        print("  %-32s log Z %.3g  posterior %.3g   [%s]" % (role, dz, dp, what))


def test_every_role_moves_the_reference_by_100_times_the_gpu_tolerance(opool):
    """A kernel that read an unknown letter as A, as U or as "no letter" computes the unsubstituted input (or something as far from it):
    for every role x loop input of the GPU tests the reference's log Z moves by at least 1e-7 * max(1, |log Z|) or a posterior above
    1e-3 by 1e-4 relative.  CONTRAfold model and the random 2.x tables: every input.  BL*: every input that is not named in
    BL_BELOW_MARGIN, which may hold the two sentinel-neighbour roles and the letter after the closing pair only -- measured: none
    is under the margin once the loop's pairs are A-U (the CG / GC rows of BL*'s interior mismatch are 0 next to A . A, as row 0 is)."""
    worst, below = least_moved(ac.cf_role_set() + ac.cf_short_set(), opool.inference)
    report("CONTRAfold model", worst)
    assert not below, [(s.what, dz, dp) for s, dz, dp in below]
    worst, below = least_moved(ac.v2_role_set(), lambda s: opool.fold2x(TS, s))
    report("2.x semantics, random tables", worst)
    assert not below, [(s.what, dz, dp) for s, dz, dp in below]
    worst, below = least_moved(ac.bl_role_set(), opool.mccaskill)
    report("Vienna-BL, BL* tables", worst)
    assert set(ac.BL_BELOW_MARGIN) <= set(ac.MAY_BE_BELOW_MARGIN), ac.BL_BELOW_MARGIN
    assert {s.role for s, _, _ in below} == set(ac.BL_BELOW_MARGIN), [(s.what, dz, dp) for s, dz, dp in below]
    kept = {s.role for s in ac.bl_gpu_set()}
    assert kept >= {"outer stem middle", "inner stem middle", "lead 0, after the outer stem", "tail 0, before the outer stem"} - set(ac.BL_BELOW_MARGIN)
    assert kept >= {"outer stem middle", "inner stem middle"} | {"hairpin letter %d of 4" % k for k in (1, 2, 3, 4)}


# ---- 5. the encodings
def test_product_encodings_equal_the_oracles_on_every_byte(tmp_path, opool):
    """nuc_code and vienna_code (ractip_amd/csrc/constraint_prepass.cpp) in a stand-alone host program, all 256 byte values, against
    cf_oracle.c: nuc_code and vienna_oracle.c: vcode; the letter the helper context re-derives from a Vienna code ("NACGU"[code])
    encodes to that code again (checked by the program)."""
    exe = str(tmp_path / "letter_codes_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ractip_amd", "csrc"),
                           os.path.join(ROOT, "tools", "letter_codes_check.cpp"),
                           os.path.join(ROOT, "ractip_amd", "csrc", "constraint_prepass.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("\n0 failures\n"), r.stdout[-500:]
    rows = [tuple(map(int, line.split())) for line in r.stdout.splitlines()[:256]]
    assert [b for b, _, _ in rows] == list(range(256))
    cfo, vo = opool.cf.L, opool.vo.L
    cfo.cfo_nuc_code.argtypes = vo.vo_code.argtypes = [ctypes.c_int]
    for b, nc, vc in rows:
        signed = b - 256 if b > 127 else b
        assert nc == cfo.cfo_nuc_code(signed) and vc == vo.vo_code(signed), (b, nc, vc)
    for b, nc, vc in rows:      # and what the models say about them: 8 / 10 letters are known, everything else is unknown
        assert (nc != 4) == (chr(b) in "ACGUacgu") and (vc != 0) == (chr(b) in "ACGUTacgut"), b
    assert [rows[ord(ch)][1] for ch in "ACGUTN"] == [0, 1, 2, 3, 4, 4] and [rows[ord(ch)][2] for ch in "ACGUTN"] == [1, 2, 3, 4, 4, 0]
    for b, _, vc in rows:       # oracle/vienna2x.py, the enumeration's encoding (ASCII letters; it upper-cases)
        if b < 128 and len(chr(b).upper()) == 1:
            assert v2.encode(chr(b))[1] == vc, b
