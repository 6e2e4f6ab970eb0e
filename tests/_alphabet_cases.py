"""Inputs with letters that are not A, C, G or U, shared by tests/test_unknown_letters_cpu.py (the references are proven to notice each
substitution), tests/test_gpu_unknown_letters.py (the kernels against the references) and oracle/gen_golden.py (the reference's engines
on the CONTRAfold inputs: tests/golden/contrafold_unknown_letters.npz).

Two encodings meet such letters ("Unknown letters"):
  * CONTRAfold model: everything but ACGUacgu is code 4, T included; code 4 never pairs, selects slot 4 of the 5-wide tables and is
    also the sentinel at positions 0 and n + 1;
  * Vienna model: T is U, lower case is upper case, everything else is code 0; code 0 never pairs, is row 0 of the mismatch / int11 /
    int21 / int22 tables, counts as "no neighbour" in the exterior and multiloop stems, and keeps a hairpin out of the tri- / tetra- /
    hexaloop tables.

A ROLE names one letter of a planted single-loop input by what the energy model reads it for; a Sub replaces exactly that letter (all
of them for "loop sides").  The planted inputs hold G, C and A only, so in the unsubstituted input no letter of a loop can pair and
the substituted letter changes one table look-up (or removes one pair), nothing else."""
import collections
import zlib

import numpy as np

import _contrafold_cases as cf

# the shapes with nucleotide terms or tables of their own (stack, 1-bulge, 1x1, 1x2, 2x2, 1xn, 2x3), one past each (1x4), a generic loop
# and the largest centre tap
LOOPS = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (2, 3), (3, 2), (1, 4), (7, 9), (15, 15)]
TOY_LOOPS = [lp for lp in LOOPS if max(lp) <= 2]        # what enumeration reaches with a 3-bp stem inside 16 letters
STRIP_COLUMNS = cf.COLUMNS[:2]                          # 57: the last owned column of group 0; 58: the first of group 1

Sub = collections.namedtuple("Sub", "what role letter seq base pos case")


def put(s, pos, ch):
    """s with its 1-based letters `pos` replaced by ch"""
    t = list(s)
    for p in pos:
        assert 1 <= p <= len(s), (p, len(s))
        t[p - 1] = ch
    return "".join(t)


def rotation(k, extra=()):
    """the substituted letter of the k-th input of a set: N, with T and lower-case n once in every five; `extra` letters take the
    first plain-N places"""
    plain = [q for q in range(k + 1) if q % 5 not in (2, 4)]
    if k % 5 == 2:
        return "T"
    if k % 5 == 4:
        return "n"
    rank = plain.index(k)
    return extra[rank] if rank < len(extra) else "N"


# ---- CONTRAfold model: the planted inputs of _contrafold_cases.py
def cf_roles(c):
    """role -> 1-based letters of a _contrafold_cases.Case.  The hairpin's inner letters and the inner letters of a long loop side
    carry no nucleotide term in this model: only its first and last letter are roles."""
    g = cf.coords(c)
    a, b, a2, b2 = g["a"], g["b"], g["a2"], g["b2"]
    r = collections.OrderedDict()
    if c.l1:
        r["closing pair, 5' inside"] = (a + 1,)
        r["enclosed pair, 5' outside"] = (a2 - 1,)
    if c.l2:
        r["closing pair, 3' inside"] = (b - 1,)
        r["enclosed pair, 3' outside"] = (b2 + 1,)
    r["hairpin first"] = (a2 + 8,)
    r["hairpin last"] = (b2 - 8,)
    if c.lead:
        r["before the outer stem"] = (a - 8,)
    if c.tail:
        r["after the outer stem"] = (b + 8,)
    r["outer stem middle"] = (g["mid"],)
    r["inner stem middle"] = (g["mid2"],)
    if c.l1 + c.l2:
        r["loop sides"] = tuple(range(a + 1, a2)) + tuple(range(b2 + 1, b))
    return r


SENTINEL_ROLES = {"lead 0": "after the outer stem", "tail 0": "before the outer stem"}


def subs_of(c, k0, keep=None, tag=""):
    """one Sub per role of case c (distinct sequences only); the letter rotates from rank k0"""
    out, seen = [], set()
    for role, pos in cf_roles(c).items():
        if keep is not None and role not in keep:
            continue
        letter = rotation(k0 + len(out))
        s = put(c.seq, pos, letter)
        if s.upper().replace("T", "N") in seen:       # (1, x): the letter inside the closing pair is the one outside the enclosed pair
            continue
        seen.add(s.upper().replace("T", "N"))
        out.append(Sub("%s%s <- %s: %s" % (tag, role, letter, c.what), tag + role, letter, s, c.seq, pos, c))
    return out


def strip_case(q, l1, l2, lead=None, tail=None):
    """the q-th loop on the strip edges: the closing pair on column 57 or 58, its diagonal on residue q mod 8 and in a strip
    (h_for(..., strips=True)), the short tail (masked staging) and the long one (an interior group) in turn"""
    col = STRIP_COLUMNS[q % 2]
    h = cf.h_for(l1 + l2, q % 8, strips=True)
    lead = col - 8 if lead is None else lead
    if tail is None:
        tail = cf.SHORT_TAIL if (q // 2) % 2 else cf.long_tail(lead, l1 + l2, h)
    return cf.case("unknown letter", lead, l1, l2, h, tail)


def cf_role_set():
    """Every role x loop on the strip edges, then per loop the two sentinel-neighbour inputs: no letter before the outer stem and an
    unknown one after it, and the other way round"""
    out = []
    for q, (l1, l2) in enumerate(LOOPS):
        out += subs_of(strip_case(q, l1, l2), len(out))
        out += subs_of(strip_case(q, l1, l2, lead=0, tail=cf.SHORT_TAIL), len(out), keep=("after the outer stem",), tag="lead 0, ")
        out += subs_of(strip_case(q, l1, l2, tail=0), len(out), keep=("before the outer stem",), tag="tail 0, ")
    return out


def cf_short_set():
    """The same roles at 41..79 letters (two letters in front, three behind): what lin_small_fold takes under RH_SMALL=1"""
    out = []
    for q, (l1, l2) in enumerate(LOOPS):
        h = cf.h_for(l1 + l2, q % 8)
        out += subs_of(cf.case("unknown letter, short", 2, l1, l2, h, 3), len(out))
        out += subs_of(cf.case("unknown letter, short", 0, l1, l2, h, 5), len(out), keep=("after the outer stem",), tag="lead 0, ")
        out += subs_of(cf.case("unknown letter, short", 5, l1, l2, h, 0), len(out), keep=("before the outer stem",), tag="tail 0, ")
    return out


def thinned(subs, rot, step=4):
    """every `step`-th input, starting at rot mod step: what one organisation runs"""
    return subs[rot % step::step]


# ---- Vienna model: the planted inputs of _vienna2x_cases.py with a free lead, tail and hairpin
VCase = collections.namedtuple("VCase", "what seq lead l1 l2 hairpin tail outer5 outer3 inner5 inner3")


GC = ("GGGGGG", "CCCCCC", "GGG", "CCC")      # outer and inner stem of _vienna2x_cases.planted
# BL*'s interior mismatch of a CG / GC pair next to A . A is 0, the value of an unknown letter: the loop's two pairs are A-U here, whose
# mismatch rows (63, 13, 18) differ from row 0.  (tests/test_gpu_vienna_edges.py has no planted stems to take: its inputs are seeded
# random sequences; its switches and block-edge lengths are what tests/test_gpu_unknown_letters.py takes from it.)
AU_LOOP = ("GGGGGA", "UCCCCC", "AGG", "CCU")


def vplanted(lead, l1, l2, hairpin="AAAA", tail=None, stems=GC):
    """_vienna2x_cases.planted(l1, l2, 6, 3, pad, hairpin) when lead == tail == pad and stems == GC"""
    tail = lead if tail is None else tail
    outer5, outer3, inner5, inner3 = stems
    seq = "A" * lead + outer5 + "A" * l1 + inner5 + hairpin + inner3 + "A" * l2 + outer3 + "A" * tail
    what = "loop %s %dx%d %s hairpin %s%s%s lead %d tail %d" % (outer5[-1] + outer3[0], l1, l2, inner5[0] + inner3[-1], inner5[-1], hairpin,
                                                               inner3[0], lead, tail)
    return VCase(what, seq, lead, l1, l2, hairpin, tail, outer5, outer3, inner5, inner3)


def vcoords(c):
    a = c.lead + len(c.outer5)
    a2 = a + c.l1 + 1
    h1 = a2 + len(c.inner5)
    b2 = h1 + len(c.hairpin) + len(c.inner3) - 1
    b = b2 + c.l2 + 1
    return dict(a=a, b=b, a2=a2, b2=b2, h1=h1, hn=h1 + len(c.hairpin) - 1, end=b + len(c.outer3) - 1,
                mid=c.lead + (len(c.outer5) + 1) // 2, mid2=a2 + len(c.inner5) // 2)


def v_roles(c, hairpin_code=False):
    g = vcoords(c)
    a, b, a2, b2 = g["a"], g["b"], g["a2"], g["b2"]
    r = collections.OrderedDict()
    if hairpin_code:      # every letter of a hairpin that is in the tri- / tetra- / hexaloop table
        for k in range(len(c.hairpin)):
            r["hairpin letter %d of %d" % (k + 1, len(c.hairpin))] = (g["h1"] + k,)
        return r
    if c.l1:
        r["closing pair, 5' inside"] = (a + 1,)
        r["enclosed pair, 5' outside"] = (a2 - 1,)
    if c.l2:
        r["closing pair, 3' inside"] = (b - 1,)
        r["enclosed pair, 3' outside"] = (b2 + 1,)
    r["hairpin first"] = (g["h1"],)
    r["hairpin last"] = (g["hn"],)
    if c.lead:
        r["before the outer stem"] = (c.lead,)
    if c.tail:
        r["after the outer stem"] = (g["end"] + 1,)
    r["outer stem middle"] = (g["mid"],)
    r["inner stem middle"] = (g["mid2"],)
    if c.l1 + c.l2:
        r["loop sides"] = tuple(range(a + 1, a2)) + tuple(range(b2 + 1, b))
    return r


def v_subs(c, k0, extra=(), keep=None, tag="", hairpin_code=False):
    out, seen = [], set()
    for role, pos in v_roles(c, hairpin_code).items():
        if keep is not None and role not in keep:
            continue
        letter = rotation(k0 + len(out), extra)
        s = put(c.seq, pos, letter)
        if s in seen:
            continue
        seen.add(s)
        out.append(Sub("%s%s <- %s: %s" % (tag, role, letter, c.what), tag + role, letter, s, c.seq, pos, c))
    return out


# hairpins that are in a table, closed by the inner stem's last pair: (inner5, hairpin, inner3)
BL_CODED = (("GGG", "GAAA", "CCC"),)                                          # GGAAAC, a tetraloop of BL*; BL* has no triloops
V2_CODED = (("GGG", "GGGA", "CCC"), ("GGC", "AAC", "GCC"), ("GGA", "CAGUAC", "UCC"))   # GGGGAC, CAACG, ACAGUACU of random_tables


def v_role_set(loops, coded, extra=(), lead=2, tail=2, stems=GC):
    """Every role x loop, per loop the two sentinel-neighbour inputs, every letter of each table hairpin (the loop rotates), then the
    three unpaired letters of a two-branch multiloop"""
    out = []
    for l1, l2 in loops:
        out += v_subs(vplanted(lead, l1, l2, tail=tail, stems=stems), len(out), extra)
        out += v_subs(vplanted(0, l1, l2, tail=tail, stems=stems), len(out), extra, keep=("after the outer stem",), tag="lead 0, ")
        out += v_subs(vplanted(lead, l1, l2, tail=0, stems=stems), len(out), extra, keep=("before the outer stem",), tag="tail 0, ")
    for q, (i5, hp, i3) in enumerate(coded):
        l1, l2 = loops[(3 + q) % len(loops)]
        out += v_subs(vplanted(lead, l1, l2, hp, tail, stems[:2] + (i5, i3)), len(out), extra, hairpin_code=True)
    out += multiloop_subs(len(out), extra)
    return out


def multiloop_subs(k0, extra=()):
    """Two hairpins inside a 6-bp stem, one letter in front of, between and behind the branches: each is the 3' neighbour of one
    stem and the 5' neighbour of the next (stemM / mismatchM with one unknown neighbour)"""
    branch = "GGGAAAACCC"
    seq = "AA" + "GGGGGG" + "A" + branch + "A" + branch + "A" + "CCCCCC" + "AA"
    c = VCase("multiloop of two hairpins", seq, 2, 0, 0, "AAAA", 2, "GGGGGG", "CCCCCC", "GGG", "CCC")
    out = []
    for name, pos in (("multiloop, after the closing pair", 9), ("multiloop, between the branches", 20), ("multiloop, before the closing pair", 31)):
        assert seq[pos - 1] == "A" and seq[pos - 2] in "GC" and seq[pos] in "GC"
        letter = rotation(k0 + len(out), extra)
        out.append(Sub("%s <- %s: %s" % (name, letter, c.what), name, letter, put(seq, (pos,), letter), seq, (pos,), c))
    return out


def bl_role_set():
    """Vienna-BL (1.8 semantics, BL* tables): X and - once each among the substituted letters"""
    return v_role_set(LOOPS, BL_CODED, extra=("X", "-"), stems=AU_LOOP)


def v2_role_set():
    """2.x semantics on the random table set: tri-, tetra- and hexaloop letters, every loop kind (1xn: kind 3, 2x3: kind 4)"""
    return v_role_set(LOOPS, V2_CODED)


def toy_role_set(coded):
    """At most 16 letters, for enumeration: a 3-bp outer stem, one enclosed pair closing a 3-letter hairpin, loops up to (2, 2), one
    letter in front and behind only for the roles that read it; then the table hairpins inside a 3-bp stem"""
    out = []
    for l1, l2 in TOY_LOOPS:
        kw = dict(stems=("GGG", "CCC", "G", "C"), hairpin="AAA")
        frame = ("before the outer stem", "after the outer stem")
        out += [s for s in v_subs(vplanted(0, l1, l2, tail=0, **kw), len(out)) if s.role not in frame]
        if l1 + l2 < 4:
            out += v_subs(vplanted(1, l1, l2, tail=1, **kw), len(out), keep=frame)
        out += v_subs(vplanted(0, l1, l2, tail=1, **kw), len(out), keep=frame, tag="lead 0, ")
        out += v_subs(vplanted(1, l1, l2, tail=0, **kw), len(out), keep=frame, tag="tail 0, ")
    for i5, hp, i3 in coded:
        c = VCase("hairpin %s%s%s in a 3-bp stem" % (i5[-1], hp, i3[0]), "A" + i5 + hp + i3 + "A", 1, 0, 0, hp, 1, "", "", i5, i3)
        out += [Sub("hairpin letter %d of %d <- N: %s" % (k + 1, len(hp), c.what), "hairpin letter %d of %d" % (k + 1, len(hp)), "N",
                    put(c.seq, (1 + len(i5) + k + 1,), "N"), c.seq, (1 + len(i5) + k + 1,), c) for k in range(len(hp))]
    assert max(len(s.seq) for s in out) <= 16
    return out


# the Vienna-BL roles whose substitution moves the restatement by less than 100 x the GPU tolerance under the BL* tables, with the
# measured largest movement of log Z / of a posterior above 1e-3 (relative): left out of the Vienna-BL GPU set only.  Filled from
# test_every_role_moves_the_reference (tests/test_unknown_letters_cpu.py), which fails if a role that is not named here misses the
# margin or if a name other than the three the margin may excuse appears.
BL_BELOW_MARGIN = {}
MAY_BE_BELOW_MARGIN = ("lead 0, after the outer stem", "tail 0, before the outer stem", "closing pair, 3' inside")


def bl_gpu_set():
    return [s for s in bl_role_set() if s.role not in BL_BELOW_MARGIN]


# ---- random inputs
def mixed(rng, n, p_unknown=0.06):
    """ACGU with about 6 % N and 3 % T; about 8 % of the letters in lower case"""
    letters = rng.choice(list("ACGUNT"), n, p=[(1 - 1.5 * p_unknown) / 4] * 4 + [p_unknown, p_unknown / 2])
    lower = rng.random_sample(n) < 0.08
    return "".join(ch.lower() if lo else ch for ch, lo in zip(letters, lower))


def mixed_seqs(seed, lengths):
    rng = np.random.RandomState(seed)
    return [mixed(rng, n) for n in lengths]


def n_run(n, a, b):
    """a seeded ACGU sequence whose letters a .. b (1-based) are N"""
    rng = np.random.RandomState(zlib.crc32(b"%d %d %d" % (n, a, b)) & 0x7FFFFFFF)
    s = cf.rnd(rng, n)
    return s[:a - 1] + "N" * (b - a + 1) + s[b:]


# (mostly short: a mixed sequence has some five posterior entries above 1e-3 per letter, and the fixture records them all)
FIXTURE_MIXED_LENGTHS = (40, 40, 41, 41, 42, 43, 45, 57, 58, 64, 65, 160)
FIXTURE_PAIR_LENGTHS = ((40, 44), (41, 45), (58, 62), (64, 65), (40, 57), (57, 41))


def fixture_inputs():
    """(role subs, 12 mixed sequences, 6 mixed pairs): what tests/golden/contrafold_unknown_letters.npz records"""
    seqs = mixed_seqs(160, FIXTURE_MIXED_LENGTHS)
    rng = np.random.RandomState(161)
    pairs = [(mixed(rng, a), mixed(rng, b)) for a, b in FIXTURE_PAIR_LENGTHS]
    return cf_role_set() + cf_short_set(), seqs, pairs
