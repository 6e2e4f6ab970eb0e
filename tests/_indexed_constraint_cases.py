"""The indexed batch under structure constraints that tests/test_gpu_indexed_constraints.py runs and whose share pairs
tests/test_indexed_constraints_cpu.py hands to tools/joint_compose_check.cpp.  No GPU, no oracle: strings only.

Nine distinct sequences: 65 / 64 / 63 are the mask kernel's 64-row tile edges, 33 and 31 give row pitches that are no multiple
of 16, 2 and 1 are the degenerate ends, and the second 16 is used by no pair.  Sequence k has a fold constraint, a share as s1
(co_first) and a share as s2 (co_second); a share leaves 0..3 brackets open and pairs are formed between equal open counts."""
import numpy as np

from test_gpu_batch_constraints import FOLD_CONS

LENS = (65, 64, 63, 33, 31, 16, 2, 1, 16)
CONS = (FOLD_CONS[0], FOLD_CONS[1], FOLD_CONS[3], None, FOLD_CONS[8], ".((...)).x.<..>.", FOLD_CONS[4], FOLD_CONS[2], "(....)")


def _line(n, marks):
    c = ["."] * n
    for pos, ch in marks.items():
        c[pos] = ch
    return "".join(c)


CO_FIRST = (
    # 65, three open; the pair 46-50 matched inside the share lies between the open 44 and 52 with free letters (one '|') inside:
    # those letters are enclosed by a bracket of their own share, the letters 45 and 51 by an open one
    _line(65, {42: "(", 43: "x", 44: "(", 46: "(", 48: "|", 50: ")", 52: "(", 54: "<"}),
    _line(37, {30: "(", 33: "x", 36: "("}),                      # 64, two open; shorter than the sequence
    _line(63, {5: "(", 9: "<", 10: "|", 12: "(", 14: "x"}),      # 63, two open
    _line(33, {3: "(", 6: "x"}),                                 # 33, one open
    _line(31, {12: "(", 17: "x"}),                               # 31, one open
    "........x.(..)..",                                          # 16, none open, a pair of its own
    None,                                                        # 2
    "x..",                                                       # 1, longer than the sequence
    ")",                                                         # 16, in no pair: a ')' no first share may leave open, never put to one
)
CO_SECOND = (
    _line(65, {56: ")", 58: "x", 60: ")", 62: ">"}),             # 65, two open
    # 64, three open; 42-46 matched inside the share between the open 40 and 48: letter 44 is enclosed by its own share's bracket,
    # 41 and 47 by the first share's open bracket that pairs with 48, 49..51 by the one that pairs with 52
    _line(64, {40: ")", 42: "(", 46: ")", 48: ")", 50: "x", 52: ")"}),
    _line(63, {40: "x", 45: ")", 47: ">"}),                      # 63, one open
    _line(33, {20: ")", 22: "(", 26: ")", 28: ")", 30: "x"}),    # 33, two open around a pair of its own
    _line(31, {27: ")", 29: "x"}),                               # 31, one open
    "x..|",                                                      # 16, none open; shorter than the sequence
    ".x",                                                        # 2
    ".",                                                         # 1
    "(",                                                         # 16, in no pair
)
# (first, second): 4 is s1 and s2 of one pair and is in both roles elsewhere, 3 is in four pairs, 8 in none
INDEX = ((0, 1), (1, 0), (1, 3), (2, 0), (2, 3), (3, 2), (3, 4), (4, 4), (4, 2), (5, 6), (6, 5), (5, 7), (7, 5), (7, 7))
OPEN_PAIRS = tuple(p for p in range(len(INDEX)) if INDEX[p][0] <= 4)   # pairs whose joint constraint forces pairs across the cut


def pad(share, n):
    line = (share or "")[:n]
    return line + "." * (n - len(line))


def open_brackets(share, n, first):
    """0-based positions of the brackets the share leaves open in its role"""
    stack, out = [], []
    for k, ch in enumerate(pad(share, n)):
        if ch == "(":
            stack.append(k)
        elif ch == ")":
            if stack:
                stack.pop()
            else:
                out.append(k)
    return stack if first else out


def batch():
    """(seqs, cons, co_first, co_second, index).  Letters: random, then G-C on every bracket pair of a fold constraint and of a
    share, G on the open '(' of a first share and C on the open ')' of a second one -- each letter planted at most once."""
    rng = np.random.RandomState(1129)
    seqs = []
    for k, n in enumerate(LENS):
        s = list(rng.choice(list("ACGU"), n))
        planted = {}

        def plant(pos, ch):
            assert planted.setdefault(pos, ch) == ch and pos < n, (k, pos)
            s[pos] = ch
        for line in (CONS[k], pad(CO_FIRST[k], n), pad(CO_SECOND[k], n)):
            for i, j in inner_pairs(line):
                plant(i, "G"), plant(j, "C")
        for i in open_brackets(CO_FIRST[k], n, True):
            plant(i, "G")
        for j in open_brackets(CO_SECOND[k], n, False):
            plant(j, "C")
        seqs.append("".join(s))
    for a, b in INDEX:
        assert len(open_brackets(CO_FIRST[a], LENS[a], True)) == len(open_brackets(CO_SECOND[b], LENS[b], False)), (a, b)
    return seqs, list(CONS), list(CO_FIRST), list(CO_SECOND), [tuple(p) for p in INDEX]


def inner_pairs(line):
    """(i, j) of the bracket pairs matched inside one string, 0-based; open brackets are skipped"""
    stack, out = [], []
    for k, ch in enumerate(line or ""):
        if ch == "(":
            stack.append(k)
        elif ch == ")" and stack:
            out.append((stack.pop(), k))
    return out


def joint_string(p, seqs, co_first, co_second, index):
    a, b = index[p]
    return pad(co_first[a], len(seqs[a])) + pad(co_second[b], len(seqs[b]))


def expanded(seqs, cons, co_first, co_second, index):
    """The same batch for Context.batch_upload: pairs, per-pair fold constraints, materialised joint strings"""
    pairs = [(seqs[a], seqs[b]) for a, b in index]
    return pairs, [(cons[a], cons[b]) for a, b in index], [joint_string(p, seqs, co_first, co_second, index) for p in range(len(index))]
