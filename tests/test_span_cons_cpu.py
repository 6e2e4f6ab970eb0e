"""CPU suite of span folds under structure constraints (rh_span_fold_constrained, rh_span_fold_batch_constrained).

  1  the reference checks itself: under band_mask & constraint_mask the oracle's DP equals its own enumeration on the short cases
     (1e-12 on log Z, the posteriors and up at three widths)
  2  the cases of the GPU suite are worth running: every reference differs from the unconstrained band reference by more than 1e-3
     in log Z and has at least 10 band cells above 1e-6, so neither a kernel that ignores the constraint nor a floor that hides
     everything can pass.  L = 2 is the one span limit for which no input can meet this -- a pair needs three letters inside, so
     the ensemble is the open chain with log Z = 0 and an empty band whatever the constraint says; there the condition is that
     the reference is exactly that.  Items of one or two letters of the ragged batch have no pair either
  3  tools/span_cons_check.cpp, built with the host sanitizers: the packed per-letter records decide every pair as allow_pair does
     on the unpacked arrays (every pair of the shared strings up to 64 letters, whose mask is also that of tests/_oracle.py's
     constraint_mask; random and forced pairs at n = 10^6 with indices that need 20 bits), and every refusal that needs no GPU
     comes back with its code and its text."""
import os
import subprocess

import numpy as np
import pytest

import _span_cases as sc
import _span_cons_cases as cc
from _oracle import constraint_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")
RH_ERR_ARG = -1
NONCOMP = "a forced pair of non-complementary letters (pair type 7) is not supported"


# ---- 1
@pytest.mark.parametrize("k", range(len(cc.SHORT)))
def test_the_oracle_dp_equals_its_enumeration_under_the_combined_mask(k):
    seq, cons, L = cc.SHORT[k]
    assert len(seq) <= 18
    for max_w in (1, 4, 9):
        dp, bf = cc.masked_cons(seq, L, cons, max_w), cc.masked_cons(seq, L, cons, max_w, bruteforce=True)
        assert abs(dp["logZ"] - bf["logZ"]) <= 1e-12
        assert np.abs(dp["band"] - bf["band"]).max() <= 1e-12 and np.abs(dp["up"] - bf["up"]).max() <= 1e-12
    mask = cc.combined_mask(len(seq), L, cons)
    band = cc.masked_cons(seq, L, cons)["band"]
    for i in range(len(seq)):
        for d in range(1, band.shape[1]):
            if band[i, d] > 0:
                assert mask[i + 1, i + 1 + d], "a pair the mask excludes has a probability"


def test_the_short_cases_feel_their_constraints():
    moved = [abs(cc.masked_cons(s, L, t)["logZ"] - cc.masked_cons(s, L, None)["logZ"]) for s, t, L in cc.SHORT if L > 4]
    assert min(moved) > 1e-3, moved


# ---- 2
@pytest.mark.parametrize("n,L", cc.SINGLE)
def test_the_gpu_cases_are_worth_running(n, L):
    seq, cons = cc.case(n, L)
    ref, free = cc.masked_cons(seq, L, cons, 15), cc.masked_cons(seq, L, None, 15)
    print("n=%d L=%d: log Z %.6f under the constraint, %.6f without; %d band cells above 1e-6" % (n, L, ref["logZ"], free["logZ"], (ref["band"] > 1e-6).sum()))
    if L == 2:
        assert ref["logZ"] == 0.0 and not ref["band"].any() and (ref["up"][:, 0] == 1.0).all()
        return
    assert abs(ref["logZ"] - free["logZ"]) > 1e-3
    assert (ref["band"] > 1e-6).sum() >= 10


def test_the_cases_hold_the_edges_they_are_named_for():
    s300, c300 = cc.case(300, 60)
    assert len(c300) == 271 < len(s300), "a constraint shorter than the sequence"
    assert c300[61:67] == "xxxxxx" and c300[99:103] == "<<<<" and c300[119:123] == ">>>>"
    assert c300[252:258] == "((((((" and c300[265:271] == "))))))"            # letters 253..258 and 266..271: both sides of column 256
    assert c300[149] == "(" and c300[149 + 59] == ")" and c300[199:202] == "(.)"
    m = constraint_mask(c300, 300)
    assert m[150, 209] and m[253, 271] and m[258, 266] and not m[252, 260] and not m[257, 268] and not m[199, 201]
    _, c20 = cc.case(300, 20)
    assert c20[149] == "(" and c20[149 + 19] == ")" and c20[252:258] == "(((((("      # the helix spans 18 < 20
    _, c257 = cc.case(257, 20)
    assert c257[242:246] == "((((" and c257[253:257] == "))))" and len(c257) == 257
    _, c2 = cc.case(300, 2)
    assert c2[149:151] == "()" and c2.count("(") == 1
    _, c70 = cc.case(70, 70)
    assert c70[0] == "(" and c70[69] == ")" and "x" in c70 and "<" in c70 and ">" in c70


# ---- 3
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "span_cons_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "span_cons_check.cpp"), os.path.join(CSRC, "span_cons.cpp"), os.path.join(CSRC, "span_fold.cpp"),
                           os.path.join(CSRC, "constraint_prepass.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def shared_strings():
    out = [(s, t) for s, t, _ in cc.SHORT]
    for n, L in ((64, 20), (63, 64), (40, 13), (13, 5)):
        out.append(cc.case(n, L))
    s = sc.random_seq(64, seed=3, plant_n=False)
    for t in ("((((((....))))))..<<<>>>xx((..((...))..))|||.(.)..()", "<" * 64, ">" * 64, "x" * 64, "(" * 32 + ")" * 32, ""):
        out.append((cc.plant(s, t), t))
    return out


def test_the_records_decide_every_pair_as_allow_pair_does(exe):
    for seq, cons in shared_strings():
        n = len(seq)
        assert n <= 64
        lines = run(exe, "rule", seq, cons).splitlines()
        assert lines[0] == "ok %d" % n, lines[0]
        got = np.array([[int(ch) for ch in row] for row in lines[1:]], dtype=np.uint8).reshape(n, n)
        assert (got == constraint_mask(cons, n)[1:, 1:]).all(), "the mask of the records is constraint_mask's: %r" % cons


def test_a_million_letters_with_indices_of_20_bits(exe):
    head, tested, allowed, max_index = run(exe, "big").split()
    assert head == "ok" and int(tested) > 2 * 10 ** 6 and 0 < int(allowed) < int(tested) and int(max_index) >= 2 ** 19


@pytest.mark.parametrize("args,text", [
    (("single", 20, "GGGAAACCC", "((("), "span fold: unbalanced '(' in the structure constraint"),
    (("single", 20, "GGGAAACCC", "..)"), "span fold: unbalanced ')' in the structure constraint"),
    (("single", 20, "GGGAAACCC", "(...)"), "span fold: " + NONCOMP),
    (("single", 8, "GGGAAACCC", "(.......)"), "span fold: the constraint pairs letters 1 and 9, which max_span 8 excludes (a pair (a, b) needs b - a < max_span)"),
    (("single", 2, "GGGAAACCC", ".(....)"), "span fold: the constraint pairs letters 2 and 7, which max_span 2 excludes (a pair (a, b) needs b - a < max_span)"),
    (("batch", 20, "GGGAAACCC", "null", "GGGAAACCC", "(((", "GGGAAACCC", ")"), "span fold batch: item 1: unbalanced '(' in the structure constraint"),
    (("batch", 20, "GGGAAACCC", "(.......)", "GGGAAACCC", "(...)"), "span fold batch: item 1: " + NONCOMP),
    (("batch", 6, "GGGAAACCC", "..(...)", "GGGAAACCC", "..", "GGGAAACCC", ".(.....)"),
     "span fold batch: item 2: the constraint pairs letters 2 and 8, which max_span 6 excludes (a pair (a, b) needs b - a < max_span)"),
])
def test_every_refusal_with_its_code_and_text(exe, args, text):
    assert run(exe, *args) == "err %d %s\n" % (RH_ERR_ARG, text)


def test_what_is_accepted_and_what_restricts(exe):
    assert run(exe, "single", 9, "GGGAAACCC", "(.......)") == "ok 1 11\n"            # b - a = 8 = L - 1
    assert run(exe, "single", 20, "GGGAAACCC", "(.......)..xx((") == "ok 1 11\n"      # the surplus behind letter n is not read
    assert run(exe, "single", 20, "GGGAAACCC", "null") == "ok 0 0\n"
    assert run(exe, "single", 20, "GGGAAACCC", "..|..") == "ok 0 0\n"
    assert run(exe, "single", 20, "GGGAAACCC", "") == "ok 0 0\n"
    assert run(exe, "single", 20, "GGGAAACCC", "....x") == "ok 1 11\n"
    assert run(exe, "batch", 20, "GGGAAACCC", "null", "GGGAAACCCC", "<", "GG", "..") == "ok\nitem 0 0\nitem 1 12\nitem 2 0\n"
    assert run(exe, "batch", 20, "nullcons", "GGGAAACCC", "GG") == "ok\nitem 0 0\nitem 1 0\n"
