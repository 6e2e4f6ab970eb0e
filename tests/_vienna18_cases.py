"""The inputs of tests/test_gpu_vienna18_tables.py, shared with tests/test_vienna18_tables_cpu.py, which proves on the oracle alone that
every index mutation of tests/_vienna18_tables.py moves a compared quantity of these very inputs by 100 x the GPU tolerance or more.

Shapes are small: the table look-ups are under test, not the tiling (tests/test_gpu_vienna_edges.py, test_gpu_duplex_edges.py)."""
import collections
import itertools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _alphabet_cases as ab
import _duplex_cases as dc
import _span_acc_cases as ac
import _vienna18_tables as vt
from _oracle import ORACLE_WORKERS, ViennaOracle, tri_offset

SEED = 18                      # of the scrambled table set
REL, UP_FLOOR = 1e-6, 1e-11    # the project's tolerances: rel 1e-6 on bp / hp / band, the same with abs_floor 1e-11 on up,
LOGZ = 1e-9                    # 1e-9 * max(1, |log Z|) on log Z
MARGIN = 100                   # a mutant must move a compared quantity by this many tolerances


def write_tables(directory, T=None, name="scrambled18.params"):
    return vt.write(os.path.join(str(directory), name), vt.scrambled(SEED) if T is None else T)


def rnd(rng, n, plant_n=True):
    s = list(rng.choice(list("ACGU"), n))
    if plant_n:
        s[n // 3] = "N"
    return "".join(s)


# ---- folds: 66 letters and more reach the block products (the decorated FCX / FCB / FCA copies); widths on both sides of the loop budget
FOLD_LENGTHS = (40, 66, 90, 130)
FOLD_WIDTHS = (5, 33)


def fold_pairs():
    rng = np.random.RandomState(1866)
    s = [rnd(rng, n) for n in FOLD_LENGTHS]
    return [(s[0], s[1]), (s[2], s[3])]


# ---- planted single loops (vplanted of _alphabet_cases.py): an outer stem of six pairs, the loop, an inner stem of three pairs on AAAA
PAIRS = ("CG", "GC", "GU", "UG", "AU", "UA")                      # pair types 1 .. 6
LOOPS = ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (1, 4), (7, 9), (15, 15), (0, 3))
TABULATED = ((1, 1), (1, 2), (2, 1), (2, 2))                      # every filling of the loop letters: 16, 64, 64, 256
FILL_PAIRS = ("UA", "CG")                                          # closing and enclosed pair of the fillings: types 6 and 1
PLANTED_MAY_DROP = 0.05                                            # share of the cases the 0.5 rule may leave out

Planted = collections.namedtuple("Planted", "what seq closing enclosed")


def planted_case(l1, l2, closing, enclosed, fill, what):
    """closing / enclosed: two letters, 5' and 3' letter of the pair; fill: the l1 + l2 loop letters, 5' side first"""
    stems = ("GGGGG" + closing[0], closing[1] + "CCCCC", enclosed[0] + "GG", "CC" + enclosed[1])
    c = ab.vplanted(2, l1, l2, stems=stems)
    g = ab.vcoords(c)
    pos = list(range(g["a"] + 1, g["a2"])) + list(range(g["b2"] + 1, g["b"]))
    assert len(pos) == len(fill) == l1 + l2
    seq = list(c.seq)
    for p, ch in zip(pos, fill):
        seq[p - 1] = ch
    return Planted("%s: %dx%d %s..%s fill %s" % (what, l1, l2, closing, enclosed, fill or "-"), "".join(seq), (g["a"], g["b"]), (g["a2"], g["b2"]))


def planted_cases():
    """every filling of the tabulated shapes at one pair-type combination, then all 36 combinations of closing and enclosed pair of
    every shape at one seeded filling"""
    out = []
    for l1, l2 in TABULATED:
        for fill in itertools.product("ACGU", repeat=l1 + l2):
            out.append(planted_case(l1, l2, FILL_PAIRS[0], FILL_PAIRS[1], "".join(fill), "filling"))
    rng = np.random.RandomState(1837)
    for l1, l2 in LOOPS:
        fill = "".join(rng.choice(list("ACGU"), l1 + l2))
        for closing in PAIRS:
            for enclosed in PAIRS:
                out.append(planted_case(l1, l2, closing, enclosed, fill, "pair types"))
    assert len(out) == 16 + 64 + 64 + 256 + 36 * len(LOOPS)
    return out


def stem_posteriors(post, n, case):
    return np.array([post[tri_offset(n, i) + j] for i, j in (case.closing, case.enclosed)])


def planted_kept(cases, posts):
    """the cases in which the oracle puts more than 0.5 on a stem (the closing or the enclosed pair)"""
    return [k for k, (c, p) in enumerate(zip(cases, posts)) if stem_posteriors(p, len(c.seq), c).max() > 0.5]


# ---- two-molecule ensemble
COFOLD_SIZES = ((30, 35), (70, 75))


def cofold_pairs():
    rng = np.random.RandomState(1835)
    return [(rnd(rng, a, False), rnd(rng, b, False)) for a, b in COFOLD_SIZES]


# ---- pf_duplex: the smallest group-edge lengths of test_gpu_duplex_edges.py (62 - 1, 62, 62 + 1) and its planted loops (_duplex_cases.py)
def duplex_pairs():
    edge = [("edge shape %d x %d" % (len(a), len(b)), a, b) for a, b in dc.edge_pairs("vienna")[:3]]
    assert [(len(a), len(b)) for _, a, b in edge] == [(61, 9), (62, 62), (63, 64)]
    return edge + dc.planted_pairs("vienna")


# ---- span family
SPAN_SHAPES = ((90, 33, 1), (130, 64, 1), (90, 33, 33), (130, 64, 15), (70, 70, 64))    # (n, L, max_w)
SPAN_BATCH = ((13, 65, 130), 31, 8)                                                   # ragged lengths, L, max_w
SPAN_PLANTED_L = 40


def span_seq(n):
    return rnd(np.random.RandomState(1800 + n), n)


# ---- the oracle on all of it
FAMILIES = ("fold", "planted", "cofold", "duplex", "span", "span planted")


def oracle_results(params, families=FAMILIES, planted_only=None):
    """family -> list of (what, {quantity: array}) of the oracle on a table file; the quantities are what the GPU tests compare.
    planted_only: indices of planted_cases() to run (None: all)"""
    vo = ViennaOracle(params)
    out = {}
    with ThreadPoolExecutor(max_workers=ORACLE_WORKERS) as pool:
        if "fold" in families:
            jobs = [(s, W, pool.submit(vo._mccaskill, s, W, False)) for pr in fold_pairs() for s in pr for W in FOLD_WIDTHS]
            out["fold"] = [("fold n=%d max_w=%d" % (len(s), W), dict(logZ=f.result()["logZ"], bp=f.result()["post"], up=f.result()["up"]))
                           for s, W, f in jobs]
        if "planted" in families:
            cases = planted_cases()
            idx = range(len(cases)) if planted_only is None else planted_only
            jobs = [(k, pool.submit(vo._mccaskill, cases[k].seq, 1, False)) for k in idx]
            out["planted"] = [(cases[k].what, dict(logZ=f.result()["logZ"], stems=stem_posteriors(f.result()["post"], len(cases[k].seq), cases[k]),
                                                   post=f.result()["post"])) for k, f in jobs]
        if "cofold" in families:
            jobs = [(s1, s2, pool.submit(vo._cofold, s1, s2)) for s1, s2 in cofold_pairs()]
            out["cofold"] = [("cofold %d+%d" % (len(s1), len(s2)), dict(logZ=f.result()["logZ"], hp=f.result()["hp"])) for s1, s2, f in jobs]
        if "duplex" in families:
            jobs = [(what, pool.submit(vo.pf_duplex, s1, s2)) for what, s1, s2 in duplex_pairs()]
            out["duplex"] = [(what, dict(logZ=f.result()["logZ"], hp=f.result()["pr"])) for what, f in jobs]
    if "span" in families:      # under the band mask, which is one global of the oracle: on this thread
        out["span"] = []
        shapes = list(SPAN_SHAPES) + [(n, SPAN_BATCH[1], SPAN_BATCH[2]) for n in SPAN_BATCH[0]]
        for n, L, W in shapes:
            r = ac.masked_acc(span_seq(n), L, W, params=params)
            out["span"].append(("span n=%d L=%d max_w=%d" % (n, L, W), dict(logZ=r["logZ"], band=r["band"], up=r["up"])))
    if "span planted" in families:      # the planted loops as items of one span_fold_batch
        out["span planted"] = []
        for c in planted_cases():
            r = ac.masked_acc(c.seq, SPAN_PLANTED_L, 1, params=params)
            out["span planted"].append(("L=%d %s" % (SPAN_PLANTED_L, c.what), dict(logZ=r["logZ"], band=r["band"], up=r["up"])))
    return out


def movement(a, b):
    """largest shift between two oracle results of one input, in units of the GPU tolerance of each quantity: log Z against
    1e-9 * max(1, |log Z|); a probability of at least 1e-6 in either result against 1e-6 of the larger of the two"""
    worst = 0.0
    for key in a:
        if key == "post":
            continue
        x, y = np.asarray(a[key], dtype=np.float64), np.asarray(b[key], dtype=np.float64)
        if key == "logZ":
            worst = max(worst, float(abs(x - y) / (LOGZ * max(1.0, abs(x)))))
            continue
        big = np.maximum(x, y) >= 1e-6
        if big.any():
            worst = max(worst, float((np.abs(x - y)[big] / (REL * np.maximum(x, y)[big])).max()))
    return worst
