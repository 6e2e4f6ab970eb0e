"""The inputs of tests/test_gpu_contrafold_weights.py, shared with tests/test_contrafold_weights_cpu.py, which proves on the oracle alone
that every name-level mutation of tests/_contrafold_weights.py moves a compared quantity of these very inputs by 100 GPU tolerances.

Shapes are small: the look-ups and the host-built tables are under test, not the tiling (tests/test_gpu_contrafold_edges.py,
tests/test_gpu_duplex_edges.py).  Families:

  fold       seeded random ACGU at 40, 66, 97, 145, 209 letters (the smallest lengths at which tests/test_gpu_far_wave.py reaches every
             block-product form) and 257, 273 for the two-level form (RH_FAR2=1);
  shapes     shape_set() / short_set() / class_subset(rot) of _contrafold_cases.py, unchanged: GC stems, poly-A loops;
  letters    frame(l1, l2, closing, enclosed, fill) =
                 AAA GGCGCGC c5 fill[:l1] e5 CCGGCGG GAAAA CCGCCGG e3 fill[l1:] c3 GCGCGCC AAA
             all 36 combinations of closing pair c5 c3 and enclosed pair e5 e3 at one seeded filling of LOOPS, and every filling of the
             shapes with single-nucleotide tables or explicit terms at closing UA / enclosed CG: 876 inputs of at most 73 letters;
  hairpin    the frame with loop (1, 1), the hairpin's closing pair h5 h3 of each of the six types and the two loop letters next to it
             over all 16 fillings (TJB / E_hairpin: helix_closing + terminal_mismatch);
  exterior   the frame with loop (1, 1), the outermost pair o5 o3 of each type and the letters outside it over all 16 fillings (TJA in
             the F5 sums: helix_closing + dangle_left + dangle_right);
  multiloop  a helix closing two hairpins with single A between the branches: the closing pair of each type, and the outermost pair of
             the first branch of each type (TJA inside and outside a multiloop, multi_base / multi_paired / multi_unpaired);
  duplex     the CONTRAfold edge pairs and planted pairs of _duplex_cases.py;
  access     the families and generators of tests/test_gpu_cf_accessibility.py, the clone oracle built from the rows under test.

The compared stem quantities of a planted case are the posteriors of its closing and of its enclosed pair (of a hairpin / exterior case
also of the pair whose type varies).  A case is kept when the oracle puts more than 0.5 on either (planted_kept of _vienna18_cases.py);
at most 5 % of a family may be left out (measured: 1 of 876 letter cases under the bundled file, 1 of 876 under the committed scrambled
file, none of the 96 + 96 + 11 junction cases under either)."""
import itertools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _cf_clone
import _contrafold_cases as cc
import _duplex_cases as dc
from _oracle import ORACLE_WORKERS, Oracle
from _vienna18_cases import PLANTED_MAY_DROP, Planted, planted_kept, stem_posteriors

PAIRS = ("CG", "GC", "GU", "UG", "AU", "UA")
LOOPS = ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2), (1, 4), (3, 5), (7, 9), (15, 15), (0, 3), (0, 12))
TABULATED = ((0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2))
FILL_PAIRS = ("UA", "CG")                  # closing and enclosed pair of the fillings
FOLD_LENGTHS, FAR2_LENGTHS = (40, 66, 97, 145, 209), (257, 273)


def rc(s):
    return cc.rc(s)


# ---- folds
def fold_seqs(far2=False):
    rng = np.random.RandomState(1902)
    s = [cc.rnd(rng, n) for n in FOLD_LENGTHS + FAR2_LENGTHS]
    return s[len(FOLD_LENGTHS):] if far2 else s[:len(FOLD_LENGTHS)]


# ---- the frame
def frame(l1, l2, closing, enclosed, fill, what, outer="GC", hairpin="GC", out5="A", out3="A", hp5="G", hp3="A"):
    """closing / enclosed / outer / hairpin: two letters, 5' and 3' letter of the pair; fill: the l1 + l2 loop letters, 5' side first"""
    assert len(fill) == l1 + l2
    seq = ("AA" + out5 + outer[0] + "GCGCGC" + closing[0] + fill[:l1] + enclosed[0] + "CCGGCG" + hairpin[0] + hp5 + "AAA" + hp3 + hairpin[1]
           + "CGCCGG" + enclosed[1] + fill[l1:] + closing[1] + "GCGCGC" + outer[1] + out3 + "AA")
    a = 11
    a2 = a + l1 + 1
    b2 = a2 + 20
    b = b2 + l2 + 1
    assert len(seq) == 43 + l1 + l2 and seq[a - 1] + seq[b - 1] == closing and seq[a2 - 1] + seq[b2 - 1] == enclosed
    return Planted(what, seq, (a, b), (a2, b2))


def letter_cases():
    """all 36 pair-type combinations of every loop at one seeded filling, then every filling of the tabulated shapes"""
    out = []
    rng = np.random.RandomState(1903)
    for l1, l2 in LOOPS:
        fill = "".join(rng.choice(list("ACGU"), l1 + l2))
        for closing in PAIRS:
            for enclosed in PAIRS:
                out.append(frame(l1, l2, closing, enclosed, fill, "pair types: %dx%d %s..%s fill %s" % (l1, l2, closing, enclosed, fill or "-")))
    for l1, l2 in TABULATED:
        for fill in itertools.product("ACGU", repeat=l1 + l2):
            fill = "".join(fill)
            out.append(frame(l1, l2, FILL_PAIRS[0], FILL_PAIRS[1], fill, "filling: %dx%d %s..%s fill %s" % ((l1, l2) + FILL_PAIRS + (fill,))))
    assert len(out) == 36 * len(LOOPS) + 4 + 4 + 16 + 64 + 64 + 256 == 876 and max(len(c.seq) for c in out) == 73
    return out


def hairpin_cases():
    """[(case, varied pair)]"""
    out = []
    for t in PAIRS:
        for x, y in itertools.product("ACGU", repeat=2):
            c = frame(1, 1, "CG", "GC", "AA", "hairpin: closing pair %s letters %s%s" % (t, x, y), hairpin=t, hp5=x, hp3=y)
            i = c.enclosed[0] + 7
            assert c.seq[i - 1] + c.seq[i + 5] == t and c.seq[i] + c.seq[i + 4] == x + y
            out.append((c, (i, i + 6)))
    return out


def exterior_cases():
    out = []
    for t in PAIRS:
        for x, y in itertools.product("ACGU", repeat=2):
            c = frame(1, 1, "CG", "GC", "AA", "exterior: outer pair %s letters %s%s" % (t, x, y), outer=t, out5=x, out3=y)
            i, j = 4, len(c.seq) - 3
            assert c.seq[i - 1] + c.seq[j - 1] == t and c.seq[i - 2] + c.seq[j] == x + y
            out.append((c, (i, j)))
    return out


BRANCHES = ("GCCGGCGG", "GGCCGCGG")


def multiloop_cases():
    """AAA GGCGCG m5 A [b5 CCGGCGG GAAAA CCGCCGG b3] A [GGCCGCGG GAAAA CCGCGGCC] A m3 CGCGCC AAA: the closing pair m5 m3 of each type at
    b5 b3 = GC, and the first branch's outermost pair b5 b3 of each type at m5 m3 = CG; closing = the multiloop's closing pair, enclosed
    = the first branch's outermost pair"""
    out = []
    for m, b1 in [(t, "GC") for t in PAIRS] + [("CG", t) for t in PAIRS if t != "GC"]:
        br1 = b1[0] + BRANCHES[0][1:] + "GAAAA" + rc(BRANCHES[0])[:-1] + b1[1]
        br2 = BRANCHES[1] + "GAAAA" + rc(BRANCHES[1])
        seq = "AAA" + "GGCGCG" + m[0] + "A" + br1 + "A" + br2 + "A" + m[1] + "CGCGCC" + "AAA"
        a, a2 = 10, 12
        b2, b = a2 + 20, len(seq) - 9
        assert seq[a - 1] + seq[b - 1] == m and seq[a2 - 1] + seq[b2 - 1] == b1 and len(seq) == 65
        c = Planted("multiloop: closing pair %s first branch %s" % (m, b1), seq, (a, b), (a2, b2))
        out.append((c, (a2 + 22, a2 + 42)))       # the second branch's outermost pair
    return out


def junction_cases():
    """family -> [(case, varied pair)]"""
    return {"hairpin": hairpin_cases(), "exterior": exterior_cases(), "multiloop": multiloop_cases()}


def stems3(post, case, varied):
    n = len(case.seq)
    extra = Planted(case.what, case.seq, varied, varied)
    return np.concatenate([stem_posteriors(post, n, case), stem_posteriors(post, n, extra)[:1]])


def kept(cases, posts):
    """indices kept by the 0.5 rule, and the assertion of its cap"""
    k = planted_kept(cases, posts)
    assert len(cases) - len(k) <= PLANTED_MAY_DROP * len(cases), "the 0.5 rule leaves out %d of %d cases" % (len(cases) - len(k), len(cases))
    return k


# ---- duplex
def duplex_pairs():
    """[(what, s1, s2)] without the (300, 300) dummy of batch_pairs"""
    return dc.batch_pairs("contrafold")[1:]


def duplex_dummy():
    return dc.batch_pairs("contrafold")[0]


SMALL_DUPLEX = 62 * 66      # the pairs the mutants run on in the CPU test: the planted ones and the edge shapes up to this many cells


# ---- accessibility: clone oracles from the rows under test
ACC_LENGTHS = (1, 2, 33, 41)        # the two smallest of test_gpu_cf_accessibility.py, and one on either side of kStripMinN = 40
ACC_WIDTHS = (1, 15, cc.BUDGET + 1)


class CloneOracle(_cf_clone.CloneOracle):
    """_cf_clone.CloneOracle on a weight file other than the bundled one: `params` the file of `rows`"""

    def __init__(self, family, tmpdir, rows, params):
        self.family = _cf_clone.FAMILIES[family]
        self.o = Oracle(params=params)
        path = os.path.join(str(tmpdir), "clone_%s_%s" % (family, os.path.basename(params)))
        with open(path, "w") as f:
            for name, v in _cf_clone.clone_params(self.family, rows):
                f.write("%s %r\n" % (name, v))
        self.clone = self.o.L.cfo_load_params(path.encode())
        assert self.clone, "the oracle does not take the clone file " + path
        self._logz = {}


def acc_seq(fam, n):
    return _cf_clone.random_seq(np.random.default_rng(1000 + n + 7 * len(fam)), n, _cf_clone.FAMILIES[fam].alphabet)     # (seq_of of the GPU module)


def acc_jobs():
    """[(family, seq, max_w, [(i, w)])]: every region of the {A,U} and {C,G} sequences at ACC_LENGTHS for each max_w of ACC_WIDTHS, and
    the planted loop sides at widths up to 32 (the entries of test_planted_interior_loop_sides_at_the_loop_budget)"""
    jobs = [(fam, acc_seq(fam, n), W, [(i, w) for i in range(n) for w in range(W) if i + w < n])
            for fam in ("AU", "CG") for n in ACC_LENGTHS for W in ACC_WIDTHS]
    for seq, i0, side in acc_planted():
        jobs.append(("CG", seq, 32, [(i, w) for i in range(i0 - 1, i0 + side) for w in (1, 7, 14, 27, 28, 29, 30, 31) if i + w < len(seq)]))
    return jobs


def acc_planted():
    """the planted interior loop sides at the loop budget of test_gpu_cf_accessibility.py: (seq, i0, side)"""
    inner = "GCGGC" + "GGGG" + "GCCGC"
    return [("GCGGCGC" + "G" * side + inner + "GCGCCGC", 7, side) for side in (29, 30, 31)]


# ---- the oracle on all of it
FAMILIES = ("fold", "shapes", "letters", "hairpin", "exterior", "multiloop", "duplex")


def oracle_results(params, families=FAMILIES, small_duplex=False, shapes=None, far2=True):
    """family -> list of (what, {quantity: array}) of the oracle under a weight file; the quantities are what the GPU tests compare
    (`post`, the whole posterior, which the GPU tests compare densely, rides along for the keep rule and the same-bits checks; movement()
    skips it, so a mutant is weighed by log Z and the stem posteriors of a planted case).  shapes: the cases of the "shapes" family
    (None: shape_set()); far2: the 257- and 273-letter folds too"""
    o = Oracle(params)
    out = {}
    with ThreadPoolExecutor(max_workers=ORACLE_WORKERS) as pool:
        jobs = {}
        if "fold" in families:
            jobs["fold"] = [("fold n=%d" % len(s), None, None, pool.submit(o.inference, s)) for s in fold_seqs() + (fold_seqs(far2=True) if far2 else [])]
        if "shapes" in families:
            jobs["shapes"] = [(c.what, c, None, pool.submit(o.inference, c.seq)) for c in (cc.shape_set() if shapes is None else shapes)]
        if "letters" in families:
            jobs["letters"] = [(c.what, c, None, pool.submit(o.inference, c.seq)) for c in letter_cases()]
        for fam, cases in junction_cases().items():
            if fam in families:
                jobs[fam] = [(c.what, c, v, pool.submit(o.inference, c.seq)) for c, v in cases]
        if "duplex" in families:
            prs = [p for p in duplex_pairs() if not small_duplex or p[0].startswith("planted") or len(p[1]) * len(p[2]) <= SMALL_DUPLEX]
            out["duplex"] = [(what, dict(logZ=r["logZ2"][0], logZ_out=r["logZ2"][1], hp=r["post"]))
                             for what, r in [(what, f.result()) for what, f in [(w, pool.submit(o.duplex, s1, s2)) for w, s1, s2 in prs]]]
        for fam, js in jobs.items():
            out[fam] = []
            for what, c, varied, f in js:
                r = f.result()
                if fam == "fold":
                    out[fam].append((what, dict(logZ=r["logZ"], bp=r["post"])))
                elif fam == "shapes":
                    out[fam].append((what, dict(logZ=r["logZ"], stems=np.array(cc.stem_probs(r["post"], c)), post=r["post"])))
                elif varied is None:
                    out[fam].append((what, dict(logZ=r["logZ"], stems=stem_posteriors(r["post"], len(c.seq), c), post=r["post"])))
                else:
                    out[fam].append((what, dict(logZ=r["logZ"], stems=stems3(r["post"], c, varied), post=r["post"])))
    return out
