"""Inputs that drive the exponent ladder of the span folds DOWNWARDS or off its end, and their cheap references.

The band tables of a span fold hold Q * exp(-s * d): Q the weight of everything the pair of cell (i, d) closes, s the scale
exponent, d the cell's column in the band (the pair's letters are d apart; the table row is d - 1, which moves a cell by s <= 1.8
nats, inside every margin below).  A closed cell outside (kSpanTiny, kSpanHuge) = (1e-280, 1e280) raises the item's flag and the
item is recomputed on the next exponent: 0.28, then 0.7, 1.8, 0.0 under Vienna-BL; 0.12, then 0.45, 1.5, 0.0 under CONTRAfold.

Every case DESIGNATES one cell (i, d), the pair of the first letter with the last one of a tail of A's (A pairs with neither A,
C nor G), whose raw weight ln Q = log Z + ln P(cell) is known from a cheap reference.  On exponent s the cell lies in one of
four zones (zone()):

  "huge"          ln Q - s d >= ln 1e280 + MARGIN
  "in range"      ln 1e-280 + MARGIN <= ln Q - s d <= ln 1e280 - MARGIN
  "flagged-tiny"  ln 5e-324 + MARGIN <= ln Q - s d <= ln 1e-280 - MARGIN: a nonzero double below kSpanTiny
  "hole"          ln Q - s d < ln 5e-324 - HOLE_MARGIN: the product is exactly 0.0, whatever factors of order one the kernel's
                  weights add (the 20 nats are a condition on the input, not a tolerance)

and in none of them (None) in the margins between.  5e-324 is the smallest double.  A hole is what the flag did not see before
the sweeps flagged a pairable cell that comes out exactly 0: the pair was dropped and the call answered RH_OK.

References.  The sequences have few possible pairs, so the oracle's enumeration (tests/_span_cases.py, bruteforce=True) is fast
where its DP is not: 0.13 s for the lone pair at 2700 letters, 1.7 s for the two-hairpin multiloop at 3100 (DP: 25 s at 1300).
The CONTRAfold case has ONE possible pair and a closed form, Z = exp(n eu) + exp(S) (cf_closed_form).  The lengths are the
smallest that meet their condition; tests/test_span_ladder_cases_cpu.py pins every zone, on every rung a case meets, and that one
letter less misses the condition."""
import math
from collections import namedtuple

import numpy as np

import _contrafold_weights as cw

LN_TINY, LN_HUGE, LN_ZERO = math.log(1e-280), math.log(1e280), math.log(5e-324)
MARGIN, HOLE_MARGIN = 40.0, 20.0
BL_LADDER = (0.28, 0.7, 1.8, 0.0)              # the order span_ladder tries them in from the default exponent (scale_order.h)
CF_LADDER = (0.12, 0.45, 1.5, 0.0)
ACC_W = 5                                      # widths of the accessibility runs
RH_OK, RH_ERR_ARG, RH_ERR_UNSUPPORTED = 0, -1, -5


def zone(x):
    """the zone of a scaled cell ln Q - s d = x, or None in the margins between two zones"""
    if x >= LN_HUGE + MARGIN:
        return "huge"
    if LN_TINY + MARGIN <= x <= LN_HUGE - MARGIN:
        return "in range"
    if LN_ZERO + MARGIN <= x <= LN_TINY - MARGIN:
        return "flagged-tiny"
    if x < LN_ZERO - HOLE_MARGIN:
        return "hole"
    return None


def zones(ln_q, d, ladder):
    return tuple(zone(ln_q - s * d) for s in ladder)


# ---- the sequences
def lone(d):
    """one possible pair, letters 1 and d + 1: cell (0, d)"""
    return "G" + "A" * (d - 1) + "C"


HAIRPIN = "CCAAAAGG"                           # two pairs deep: the enumeration stays fast


def multi(tail):
    """two hairpins and `tail` A's inside the pair of the first and the last letter: that pair closes a multiloop or a hairpin loop.
    BL* gives an unpaired letter of a multiloop a BONUS, so the multiloop's weight grows with the tail and log Z with it."""
    return "GA" + HAIRPIN + "AA" + HAIRPIN + "A" * tail + "C"


def hairpin_chain(n):
    """the chain of stable GC hairpins of tests/test_gpu_span_fold.py: it overflows small exponents"""
    rs = np.random.RandomState(9)
    comp = {"G": "C", "C": "G"}
    seq = ""
    while len(seq) < n:
        stem = "".join(rs.choice(list("GC"), 10))
        seq += stem + "AAAA" + "".join(comp[x] for x in reversed(stem)) + "AA"
    return seq[:n]


def chain_then_lone(chain_n, d):
    """the chain, a spacer, then the lone pair d apart: the chain wants a larger exponent than the lone pair can bear"""
    return hairpin_chain(chain_n) + "AAAAA" + lone(d)


# ---- the cases.  d: the band column of the designated cell, which is the pair of letters (n - d, n), 1-based; L: max_span of the call
Case = namedtuple("Case", "name seq L d")

D_LONE_FLAG, D_LONE_HOLE = 2395, 2679          # smallest d: flagged-tiny on 0.28; a hole on 0.28
TAIL_MULTI_HOLE = 3043                         # smallest tail: the multiloop's closing cell is a hole on 0.28
BL_CHAIN, D_EXHAUST_FLAG, D_EXHAUST_HOLE = 1300, 961, 1074      # smallest d: flagged-tiny on 0.7; a hole on 0.7
CF_CHAIN, D_CF_EXHAUST_FLAG, D_CF_EXHAUST_HOLE = 1560, 1506, 1683   # bundled CONTRAfold weights: the same on 0.45
D_CF_HOLE = 1724                               # the custom weight file: a hole on 0.12


def _whole(name, seq):
    return Case(name, seq, len(seq), len(seq) - 1)


LONE_FLAG = _whole("LONE_FLAG", lone(D_LONE_FLAG))
LONE_HOLE = _whole("LONE_HOLE", lone(D_LONE_HOLE))
MULTI_HOLE = _whole("MULTI_HOLE", multi(TAIL_MULTI_HOLE))
DESCENT = (LONE_FLAG, LONE_HOLE, MULTI_HOLE)
EXHAUST_FLAG = Case("EXHAUST_FLAG", chain_then_lone(BL_CHAIN, D_EXHAUST_FLAG), BL_CHAIN, D_EXHAUST_FLAG)
EXHAUST_HOLE = Case("EXHAUST_HOLE", chain_then_lone(BL_CHAIN, D_EXHAUST_HOLE), BL_CHAIN, D_EXHAUST_HOLE)
# the constrained twin of LONE_FLAG: 'x' on the far C leaves no pairable cell
TWIN_CONSTRAINT = "." * (len(LONE_FLAG.seq) - 1) + "x"
# CONTRAfold, bundled weights: L reaches over the whole chain, whose cells are then those of the chain folded alone at L = n
CF_EXHAUST_FLAG = Case("CF_EXHAUST_FLAG", chain_then_lone(CF_CHAIN, D_CF_EXHAUST_FLAG), max(CF_CHAIN, D_CF_EXHAUST_FLAG + 1), D_CF_EXHAUST_FLAG)
CF_EXHAUST_HOLE = Case("CF_EXHAUST_HOLE", chain_then_lone(CF_CHAIN, D_CF_EXHAUST_HOLE), max(CF_CHAIN, D_CF_EXHAUST_HOLE + 1), D_CF_EXHAUST_HOLE)
CF_HOLE = _whole("CF_HOLE", lone(D_CF_HOLE))


def ln_q(ref, d):
    """ln Q of the designated cell (the last letter's pair d letters back) from a reference dict(logZ, band)"""
    n = ref["band"].shape[0]
    return ref["logZ"] + math.log(ref["band"][n - 1 - d, d])


def multi_bonus(logz_a, tail_a, logz_b, tail_b):
    """b: what one more tail letter adds to log Z where the multiloop holds all the weight; the closing cell decays by s - b a letter"""
    return (logz_b - logz_a) / (tail_b - tail_a)


# ---- CONTRAfold on a custom weight file: a hairpin of 30 letters and more costs 550 nats and an unpaired exterior letter 0.325, so
# that the one pair of lone(d) has a probability of about 0.95, neither 0 nor 1, at the length where its weight, about exp(-557.6),
# is a hole on 0.12 (the unpaired chain weighs exp(-0.325 * 1725) = exp(-560.6))
CF_HAIRPIN_30, CF_EXTERNAL_UNPAIRED = -550.0, -0.325
CF_SHORT = 34                                  # d of the short sequence S is read from: the hairpin has 33 >= 30 letters


def cf_custom_rows():
    """the bundled file with two rows changed"""
    new = {"hairpin_length_at_least_30": CF_HAIRPIN_30, "external_unpaired": CF_EXTERNAL_UNPAIRED}
    rows = [(name, new.get(name, v)) for name, v in cw.read()]
    assert sum(name in new for name, _ in rows) == 2
    return rows


def cf_pair_weight(oracle):
    """S: the log weight of lone(d)'s paired structure, from the oracle (on the custom file) at CF_SHORT.  A hairpin's length score
    stops changing at 30 letters and the structure has no unpaired exterior letter, so S is that of every d >= 31."""
    n = CF_SHORT + 1
    r = oracle.inference(lone(CF_SHORT))
    from _oracle import tri_offset
    return r["logZ"] + math.log(r["post"][tri_offset(n, 1) + n])


def cf_closed_form(S, d, eu=CF_EXTERNAL_UNPAIRED):
    """dict(logZ, band, up) of lone(d) at L = n: the unpaired chain weighs exp(n eu), the one other structure exp(S)"""
    n = d + 1
    logz = float(np.logaddexp(n * eu, S))
    p = math.exp(S - logz)
    band, up = np.zeros((n, n)), np.ones((n, 1))
    band[0, d] = p
    up[0, 0] = up[n - 1, 0] = 1.0 - p
    return dict(logZ=logz, band=band, up=up)
