"""Inputs shared by tests/test_vienna2x_oracle.py (CPU: they are proven fit on the restatement) and tests/test_gpu_vienna2x_edges.py
(GPU: the kernels of mccaskill_vienna.hip under RH_VIENNA_SEM_20 against the restatement).  Everything is seeded; the table set is
the synthetic one of tests/test_gpu_vienna2x.py, vienna2x.random_tables(23), in which every entry the 2.x energy functions can reach
has its own value."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import vienna2x as v2  # noqa: E402

TABLES = "synthetic"   # the name of the table set in OraclePool.tables2x
SEED = 23
FLOOR = 1e-12          # assert_prob_close's floor: the relative bar applies to cells above it


def tables():
    return v2.random_tables(SEED)


def rnd(rng, n):
    return "".join("ACGU"[k] for k in rng.integers(0, 4, n))


# ---- planted loops: a 6-bp GC stem and a 3-bp GC stem with a 4-letter hairpin, joined by one interior loop of l1 + l2 letters 'A'
def planted(l1, l2, outer=6, inner=3, pad=2, middle="AAAA"):
    """(sequence, p, q): (p, q) is the inner stem's first pair, the pair the loop encloses"""
    s = "A" * pad + "G" * outer + "A" * l1 + "G" * inner + middle + "C" * inner + "A" * l2 + "C" * outer + "A" * pad
    p = pad + outer + l1 + 1
    return s, p, p + 2 * inner + len(middle) - 1


# (at the budget, one letter past it): a bulge of 30 / 31 on either side, 1xn at n = 29 / 30 (kind 3), generic 14x16 / 15x16
PLANTED_EDGES = (((30, 0), (31, 0)), ((0, 30), (0, 31)), ((1, 29), (1, 30)), ((29, 1), (30, 1)), ((14, 16), (15, 16)))
PLANTED_23 = ((2, 3), (3, 2))   # kind 4; no budget edge
PLANTED_LONG = (1, 29)          # the 1xn loop again, closed by a pair of span 513 in a 520-letter sequence


def planted_long():
    """520 letters: GGGG A G^8 [466 letters: hairpins GCGCAAAAGCGC one A apart] C^8 A^29 CCCC.  The loop's closing pair (4, 517) has
    span 513, so its cell streams more than 512 FM2 terms while its single-loop lanes take the 1xn shapes; the enclosed pair
    (6, 487) closes a multiloop of some thirty branches."""
    l1, l2 = PLANTED_LONG
    middle = ("GCGCAAAAGCGCA" * 36)[:466 - 4] + "AAAA"
    s, p, q = planted(l1, l2, outer=4, inner=8, pad=0, middle=middle)
    assert len(s) == 520 and (p, q) == (6, 487)
    return s, p, q


def planted_inputs():
    """[(name, sequence, p, q, at_budget)]"""
    out = []
    for at, past in PLANTED_EDGES:
        out.append(("%dx%d" % at, *planted(*at), True))
        out.append(("%dx%d" % past, *planted(*past), False))
    for sh in PLANTED_23:
        out.append(("%dx%d" % sh, *planted(*sh), True))
    out.append(("%dx%d span 513" % PLANTED_LONG, *planted_long(), True))
    return out


# ---- single folds at the stream and budget edges
# 1, 4, 5: below and at the first hairpin; 33, 34: the first diagonals a 30-letter loop fits on, and one past; 64 .. 66, 129: lanes
# of one wavefront; 256 .. 258: a second iteration of the 4-wide streams (F5, XP, XS) and its partial last one; 300; 512 .. 514, 520:
# the same for the 8-wide FM2 stream
EDGE_PINNED = ((513, 66), (129, 256), (5, 33), (64, 1))                     # 8 sequences: the pinned grid
EDGE_UNPINNED = ((520, 4), (512, 34), (514, 65), (257, 258), (300, 9))      # 10 sequences


def edge_batches():
    rng = np.random.default_rng(520)
    return tuple([(rnd(rng, a), rnd(rng, b)) for a, b in lens] for lens in (EDGE_PINNED, EDGE_UNPINNED))


# ---- two-molecule ensemble: the cut after letter 1, after letter 64, one letter before the end, and the iteration edges of the XP
# stream (n2 = 256 .. 258 terms) and of the XS stream (n1 = 256 .. 258)
CUT_PAIRS = ((1, 70), (64, 40), (70, 1), (65, 256), (65, 257), (65, 258), (256, 65), (257, 65), (258, 65))


def cut_pairs():
    rng = np.random.default_rng(65)
    return [(rnd(rng, a), rnd(rng, b)) for a, b in CUT_PAIRS]


# ---- accessibility
WIDTHS = (1, 15, 16, 31, 64)
ACC_LENS = (1, 17, 64, 65, 300)


def acc_seqs():
    rng = np.random.default_rng(64)
    return [rnd(rng, n) for n in ACC_LENS]


# ---- constraints
CONS_N = 130
CONS_X = (60, 70)         # 'x' over letters 60 .. 70, across letter 64
CONS_FORCED = (20, 110)   # a forced pair of span 90
CO_LENS = (66, 40)
CO_FORCED = (60, 12)      # s1[60] pairs s2[12]


def put(s, letter, ch):
    return s[:letter - 1] + ch + s[letter:]


def constraint_case():
    """(sequence, constraint): an 'x' run and a forced pair in one string"""
    rng = np.random.default_rng(130)
    seq = put(put(rnd(rng, CONS_N), CONS_FORCED[0], "G"), CONS_FORCED[1], "C")
    c = list("." * CONS_N)
    c[CONS_X[0] - 1:CONS_X[1]] = "x" * (CONS_X[1] - CONS_X[0] + 1)
    c[CONS_FORCED[0] - 1], c[CONS_FORCED[1] - 1] = "(", ")"
    return seq, "".join(c)


def co_constraint_case():
    """(s1, s2, constraint over s1+s2): a forced pair across the cut"""
    rng = np.random.default_rng(106)
    n1, n2 = CO_LENS
    s1, s2 = put(rnd(rng, n1), CO_FORCED[0], "G"), put(rnd(rng, n2), CO_FORCED[1], "C")
    c = list("." * (n1 + n2))
    c[CO_FORCED[0] - 1], c[n1 + CO_FORCED[1] - 1] = "(", ")"
    return s1, s2, "".join(c)
