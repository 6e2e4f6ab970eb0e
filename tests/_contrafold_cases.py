"""The inputs of tests/test_gpu_contrafold_edges.py: sequences that isolate ONE interior loop between two GC stems, placed on the strip
and group edges of the CONTRAfold-model McCaskill kernels, and seeded random sequences at the lengths where the launch sequence changes
form.  Shared with oracle/gen_golden.py, which records the reference's engines on shape_set() (tests/golden/contrafold_planted_loops.npz).
What each generator is for: the docstring of the test module; the tests there without the gpu mark pin their properties."""
import collections

import numpy as np

GS, KD, BOOT = 57, 8, 32        # columns a strip group owns, diagonals per strip, bootstrap diagonals (mccaskill_strip.hip, inside_strips)
BUDGET = 30                     # kMaxSingle
NMAX = 300                      # the dummy sequence of every batch: fixes nmax, and so the table layout and the grids
OUTER, INNER = "GGCGCGCC", "GCCGGCGG"
COLUMNS = (57, 58, 59, 115)     # closing pair on the last owned column of group 0, the first of group 1, one past it, the first of group 2
SHORT_TAIL, LONG_TAIL = 10, 150


# ---- the generators
def rc(s):
    return "".join({"A": "U", "C": "G", "G": "C", "U": "A"}[ch] for ch in reversed(s))


def planted(lead, l1, l2, h, tail):
    return "A" * lead + OUTER + "A" * l1 + INNER + "G" + "A" * (h - 1) + rc(INNER) + "A" * l2 + rc(OUTER) + "A" * tail


Case = collections.namedtuple("Case", "what seq lead l1 l2 h tail")


def case(kind, lead, l1, l2, h, tail):
    what = "%s loop %dx%d h %d column %d tail %d" % (kind, l1, l2, h, lead + 8, tail)
    return Case(what, planted(lead, l1, l2, h, tail), lead, l1, l2, h, tail)


def coords(c):
    """Letters (1-based) and table cells of the loop: a, b the closing pair (innermost pair of the outer stem), a2, b2 the enclosed pair
    (outermost pair of the inner stem); cell (i, d) = (a, b - a - 1), (i2, d2) = (a2, b2 - a2 - 1); mid, mid2 a middle letter of either stem"""
    a = c.lead + 8
    b = a + c.l1 + c.l2 + c.h + 17
    a2, b2 = a + c.l1 + 1, b - c.l2 - 1
    return dict(a=a, b=b, a2=a2, b2=b2, i=a, d=b - a - 1, i2=a2, d2=b2 - a2 - 1, mid=c.lead + 4, mid2=a2 + 3)


def h_for(t, residue, strips=False):
    """the hairpin length in 4..11 that puts the closing diagonal d = t + h + 16 on `residue` mod 8; strips: 8 or 16 letters more where
    that diagonal would lie under the first strip (t < 12), so that the strip kernels compute the closing pair: d = 32..39 then"""
    h = 4 + (residue - (t + 20)) % 8
    while strips and t + h + 16 < BOOT:
        h += 8
    return h


def filter_class(l1, l2):
    """the code path of filt_factored a shape takes"""
    t = l1 + l2
    if t > BUDGET:
        return "past the budget"
    if l1 == 0 or l2 == 0:
        return "bulge" if t >= 2 else "stack or 1-bulge"         # (0,0), (0,1), (1,0) are not filter taps
    if l1 == l2:
        return "centre"
    if l1 <= 4 and l2 <= 4:
        return "explicit"
    return "generic even" if t % 2 == 0 else "generic odd"


def shape_set():
    """Every (l1, l2) with l1 + l2 <= 31; inside each filter class the residue of d mod 8 and the column rotate with the shape's rank"""
    rank = collections.Counter()
    out = []
    for t in range(BUDGET + 2):
        for l1 in range(t + 1):
            l2 = t - l1
            k = filter_class(l1, l2)
            out.append(case("shape", COLUMNS[(rank[k] // 8 + rank[k]) % 3] - 8, l1, l2, h_for(t, rank[k] % 8), SHORT_TAIL))
            rank[k] += 1
    return out


CLASS_LOOPS = [
    (0, 30), (30, 0), (0, 29), (0, 1), (1, 0),      # bulges
    (1, 29), (29, 1),                               # next to the bulge
    (15, 15), (14, 14), (1, 1),                     # centre taps
    (14, 15), (15, 14),                             # both parities at the top
    (7, 23), (23, 7),                               # generic
    (1, 4), (4, 1), (2, 3), (4, 4),                 # the residual table Rx (l1, l2 <= 4)
    (15, 16), (0, 31), (31, 0),                     # past the budget
]


def long_tail(lead, t, h):
    """150 letters, or what the 300 letters of the dummy leave (column 115: 119 letters or more)"""
    return min(LONG_TAIL, NMAX - (lead + 32 + t + h))


def class_set():
    out = []
    for l1, l2 in CLASS_LOOPS:
        for residue in range(8):
            for col in COLUMNS:
                h = h_for(l1 + l2, residue, strips=True)
                out.append(case("class masked", col - 8, l1, l2, h, SHORT_TAIL))
                out.append(case("class interior", col - 8, l1, l2, h, long_tail(col - 8, l1 + l2, h)))
    return out


def class_subset(rot):
    """The class set thinned for one organisation: every loop, every residue, both tails; the column rotates with loop, residue and `rot`"""
    out = []
    for q, (l1, l2) in enumerate(CLASS_LOOPS):
        for residue in range(8):
            col = COLUMNS[(q + residue + rot) % 4]
            h = h_for(l1 + l2, residue, strips=True)
            out.append(case("class masked", col - 8, l1, l2, h, SHORT_TAIL))
            out.append(case("class interior", col - 8, l1, l2, h, long_tail(col - 8, l1 + l2, h)))
    return out


SMALL_LOOPS = [(0, 1), (1, 0), (1, 1), (0, 2), (2, 0), (1, 2), (2, 1), (2, 2), (1, 4), (4, 1), (2, 3), (3, 3)]


def inner_set():
    """Small loops over long hairpins (h = 17..28): the enclosed pair on diagonal h + 14 = 31..42"""
    out = []
    for q, (l1, l2) in enumerate(SMALL_LOOPS):
        for h in range(17, 29):
            col = COLUMNS[(q + h) % 4]
            tail = SHORT_TAIL if (q + h // 4) % 2 else long_tail(col - 8, l1 + l2, h)
            out.append(case("inner", col - 8, l1, l2, h, tail))
    return out


BOOT_LOOPS = [(0, 1), (1, 0), (1, 1), (1, 4), (4, 1), (2, 3), (4, 4), (0, 10), (10, 0), (5, 5), (3, 7), (1, 9)]


def boot_set():
    """h = 4 and l1 + l2 <= 10: the closing diagonal l1 + l2 + 20 is below 32 (lin_inside_diag<4, 16, 3> alone computes it)"""
    return [case("boot", col - 8, l1, l2, 4, tail(col - 8, l1 + l2, 4))
            for l1, l2 in BOOT_LOOPS for col in COLUMNS for tail in (lambda *a: SHORT_TAIL, long_tail)]


def short_set():
    """The shape set again with two letters in front and three behind: 41..79 letters, one group, and under RH_SMALL=1 the lengths that
    lin_small_fold (mccaskill_small.hip, sequences of 8..109 letters) computes with its own copy of the weights"""
    return [case("short", 2, c.l1, c.l2, c.h, 3) for c in shape_set()]


def inner_pair_home(c):
    """Where the inside strip finds the enclosed pair: the strip's own rows (chain phase, LDS), rows staged from earlier strips, the
    bootstrap diagonals; "bootstrap only" if the closing diagonal itself is below 32"""
    g = coords(c)
    if g["d"] < BOOT:
        return "bootstrap only"
    if g["d2"] < BOOT:
        return "bootstrap"
    return "own rows" if c.l1 + c.l2 + 2 <= g["d"] % KD else "earlier strips"


def inside_group(n, i, d):
    """(group, groups, full) of cell (i, d) in lin_inside_strip: slot = (i - 1) / GS, i0 = 1 + slot * GS, ngroup over the strip's first
    diagonal d0, full = i0 + 96 <= n - d0"""
    d0 = d - d % KD
    slot = (i - 1) // GS
    ngroup = (max(n - 1 - d0, 0) + GS - 1) // GS
    return slot, ngroup, 1 + slot * GS + 96 <= n - d0


def outside_group(n, i, d):
    """the same of lin_outside_strip: the strip d0 - 7 .. d0 with d0 = d | 7, i0 = 1 + slot * GS - 7, ngroup over its longest diagonal"""
    d0 = d | (KD - 1)
    slot = (i - 1) // GS
    i0 = 1 + slot * GS - (KD - 1)
    ngroup = (max(n - 1 - (d0 - (KD - 1)), 0) + GS - 1) // GS
    return slot, ngroup, i0 >= 33 and i0 + 96 <= n - d0 and i0 + d0 - (KD - 1) >= 1


EDGE_LENGTHS = (list(range(31, 51)) + [63, 64, 65, 66, 79, 80, 81] + list(range(88, 93)) + [96, 97] + list(range(145, 150))
                + list(range(202, 207)))


def rnd(rng, n):
    return "".join(rng.choice(list("ACGU"), n))


def edge_seqs():
    rng = np.random.RandomState(57)
    return [rnd(rng, n) for n in EDGE_LENGTHS]


def dummy_seq():
    return rnd(np.random.RandomState(NMAX), NMAX)


def planted_cases():
    """shape set, class set, inner and bootstrap inputs: one case per distinct sequence"""
    seen, out = set(), []
    for c in shape_set() + class_set() + inner_set() + boot_set():
        if c.seq not in seen:
            seen.add(c.seq)
            out.append(c)
    return out


def dense(post, n):
    P = np.zeros((n + 1, n + 1))
    P[np.triu_indices(n + 1)] = post
    return P


def stem_probs(post, c):
    """P(letter paired) of a middle letter of the outer and of the inner stem"""
    P = dense(post, len(c.seq))
    g = coords(c)
    return tuple(float(P[x].sum() + P[:, x].sum()) for x in (g["mid"], g["mid2"]))


def past_budget_pairs():
    """[(at, past)]: every shape with l1 + l2 = 31 at h = 4, 7, 11 next to the shape one letter shorter (on the longer side) in the same place"""
    out = []
    for l1 in range(32):
        l2 = 31 - l1
        at = (l1, l2 - 1) if l2 > l1 else (l1 - 1, l2)
        for k, h in enumerate((4, 7, 11)):
            lead = COLUMNS[(l1 + k) % 3] - 8
            out.append((case("at", lead, at[0], at[1], h, SHORT_TAIL), case("past", lead, l1, l2, h, SHORT_TAIL)))
    return out
