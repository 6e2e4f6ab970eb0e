"""Inputs whose scaled partition function Z~ VANISHES, and their cheap references.

The scaled linear kernels store Q * exp(-s * span); a problem whose Z~ leaves (1e-200, 1e200) is recomputed with another exponent
before the log-space kernels are tried.  The inputs here drive those ladders DOWNWARDS: a short structured insert over {A, C, G} (only
G-C pairs form) inside poly-A flanks that cannot pair.  Every structure then lives inside the insert, so

  * bp of the long sequence, restricted to the insert, equals bp of the same insert with 3-letter flanks, shifted; it is 0 elsewhere;
  * CONTRAfold log Z grows by a constant B per extra flank letter, B = logZ("A" * 41) - logZ("A" * 40);
  * Vienna-BL log Z does not change; a window of unpaired letters has the probability of its part inside the short sequence (a flank
    letter is unpaired in every structure), 1 if it lies in a flank.

The reference of an n = 3950 problem is therefore a 96-letter call of the plain double-precision oracles.  tests/test_vanishing_cases_cpu.py
pins the identities against the directly computed oracle and the position of every case relative to the flag threshold; the duplex
cases are compared with the oracle on the full pair and need no embedding."""
import math
from collections import namedtuple

import numpy as np

from _oracle import tri_offset, tri_size

# ---- the exponents of include/ractip_hot.h (rh_batch_fallbacks) and the flag threshold of the finish kernels
LN_LO, LN_HI = math.log(1e-200), math.log(1e200)
MARGIN = 40.0                                  # nats a case keeps from the threshold, on the side its label names
CF_S, CF_DOWN = 0.12, (0.0,)                   # CONTRAfold folds: default, then the rungs a vanishing sequence is given in turn
BL_S, BL_ORDER = 0.28, (0.7, 1.8, 0.0)         # Vienna-BL folds / two-molecule ensemble: the whole batch, every rung in this order
DX_S, DX_ORDER = 0.65, (1.3, 2.2, 0.3, 0.0)    # CONTRAfold duplex: every rung in this order
VDX_S = 0.27                                   # Vienna-BL pf_duplex: no ladder
FLANK = 3                                      # letters the short sequence keeps on both sides (0 breaks the identity)
MAX_W = 15

COMP = {"A": "A", "C": "G", "G": "C"}          # (A has no partner: there is no U)


def _letters(seed, n):
    return "".join(np.random.RandomState(seed).choice(list("ACG"), n))


INSERT = _letters(1, 90)
# second molecule: the reverse complement of the first insert's 3' half, then letters of its own
INSERT2 = "".join(COMP[ch] for ch in reversed(INSERT[45:])) + _letters(2, 30)
# duplex strands: 60 letters and their reverse complement (A against A: interior loops)
DX_INSERT = _letters(3, 60)
DX_INSERT2 = "".join(COMP[ch] for ch in reversed(DX_INSERT))


def flanked(ins, f5, f3):
    return "A" * f5 + ins + "A" * f3


def short_of(ins):
    return flanked(ins, FLANK, FLANK)


def flanks_at(where, n, ins=INSERT):
    """(f5, f3) that put the insert at the 5' end (FLANK letters before it), in the middle or at the 3' end of n letters."""
    free = n - len(ins)
    assert free >= 2 * FLANK
    f5 = {"5'": FLANK, "mid": free // 2, "3'": free - FLANK}[where]
    return f5, free - f5


# ---- references of the long sequence from the short one
def embed_bp(short_post, ins_len, f5, f3):
    """bp (triangular, reference layout) of flanked(ins, f5, f3) from that of short_of(ins)"""
    m, n, sh = ins_len + 2 * FLANK, f5 + ins_len + f3, f5 - FLANK
    out = np.zeros(tri_size(n))
    for i in range(FLANK + 1, FLANK + ins_len + 1):
        o, O = tri_offset(m, i), tri_offset(n, i + sh)
        out[O + i + sh:O + FLANK + ins_len + sh + 1] = short_post[o + i:o + FLANK + ins_len + 1]
    return out


def insert_block_mask(ins_len, f5, f3):
    """True on the cells (i, j) of the triangular layout with both letters inside the insert"""
    n = f5 + ins_len + f3
    mask = np.zeros(tri_size(n), dtype=bool)
    for i in range(f5 + 1, f5 + ins_len + 1):
        O = tri_offset(n, i)
        mask[O + i:O + f5 + ins_len + 1] = True
    return mask


def embed_up(short_up, ins_len, f5, f3, max_w=MAX_W):
    """up[a-1][w] = P(letters a .. a+w unpaired) of the long sequence: the window's part inside the short sequence's letters (the
    flank letters beyond are unpaired in every structure); 1 when nothing is left, 0 where the window runs off the end"""
    n, sh = f5 + ins_len + f3, f5 - FLANK
    lo, hi = sh + 1, sh + ins_len + 2 * FLANK          # the letters of the long sequence the short one holds
    out = np.zeros((n, max_w))
    for a in range(1, n + 1):
        for w in range(max_w):
            b = a + w
            if b > n:
                break
            ca, cb = max(a, lo), min(b, hi)
            out[a - 1, w] = 1.0 if ca > cb else short_up[ca - sh - 1, cb - ca]
    return out


def embed_hp(short_hp, n1, n2, shift1, shift2):
    """hp (n1+1) x (n2+1) of a long pair from that of the short pair whose letters sit shift1 / shift2 further along"""
    out = np.zeros((n1 + 1, n2 + 1))
    m1, m2 = short_hp.shape[0] - 1, short_hp.shape[1] - 1
    out[1 + shift1:m1 + 1 + shift1, 1 + shift2:m2 + 1 + shift2] = short_hp[1:, 1:]
    return out


def cf_flank_letter(oracle):
    """B: what one more flank letter adds to the CONTRAfold log Z"""
    return oracle.inference("A" * 41)["logZ"] - oracle.inference("A" * 40)["logZ"]


# ---- the cases
Fold = namedtuple("Fold", "model label where n seq f5 f3")            # model: "cf" / "bl"; label: "inside" / "vanishing"
Duplex = namedtuple("Duplex", "model label s1 s2")                    # label: "inside", "vanishing", or the rung that holds the pair
Cofold = namedtuple("Cofold", "label s1 s2 k1")                       # k1: the 5' flank of s1 (s2 keeps FLANK letters before its insert)

CF_N_INSIDE, CF_N_VANISHING = 3200, 3950
BL_N_INSIDE, BL_N_VANISHING = 1500, 1900
POSITIONS = ("5'", "mid", "3'")


def fold_case(model, label, where, n):
    f5, f3 = flanks_at(where, n)
    return Fold(model, label, where, n, flanked(INSERT, f5, f3), f5, f3)


def fold_cases():
    out = []
    for model, n_in, n_van in (("cf", CF_N_INSIDE, CF_N_VANISHING), ("bl", BL_N_INSIDE, BL_N_VANISHING)):
        out += [fold_case(model, "inside", w, n_in) for w in POSITIONS]
        out += [fold_case(model, "vanishing", w, n_van) for w in POSITIONS]
    return out


def dx_pair(a, b):
    """the duplex inserts in the middle of a and b letters"""
    return flanked(DX_INSERT, *flanks_at("mid", a, DX_INSERT)), flanked(DX_INSERT2, *flanks_at("mid", b, DX_INSERT2))


def duplex_cases():
    return [Duplex("cf", "inside", *dx_pair(350, 350)), Duplex("cf", 0.3, *dx_pair(550, 550)), Duplex("cf", 0.0, *dx_pair(1000, 1000)),
            Duplex("bl", "inside", *dx_pair(700, 700)), Duplex("bl", "vanishing", *dx_pair(1025, 1025))]


# one U in a poly-A strand against poly-A: the sum over closing pairs has terms (any != 0), one pair deep, and underflows
DX_ONE_PAIR = ("A" * 499 + "U" + "A" * 500, "A" * 1000)
# no complementary letter at all: the -2e20 sentinel and a zero hp, not flagged
DX_NO_PAIR = ("".join(np.random.RandomState(4).choice(list("AG"), 500)), "".join(np.random.RandomState(5).choice(list("AG"), 500)))


def cofold_pair(k1, k2):
    """inserts at the 3' end of the first and the 5' end of the second molecule: the pairs between them enclose the cut"""
    return flanked(INSERT, k1, FLANK), flanked(INSERT2, FLANK, k2)


COFOLD_LEN = 1010


def cofold_case():
    k1, k2 = COFOLD_LEN - len(INSERT) - FLANK, COFOLD_LEN - len(INSERT2) - FLANK
    return Cofold("vanishing only as a joint ensemble", *cofold_pair(k1, k2), k1)


def ln_scaled(logz, s, span):
    """ln Z~ of a problem with log partition function logz on exponent s (span: n of a fold, L1 + L2 + 2 of a duplex sweep)"""
    return logz - s * span


def inside(x):
    return LN_LO + MARGIN <= x <= LN_HI - MARGIN


def outside(x):
    return x <= LN_LO - MARGIN or x >= LN_HI + MARGIN
