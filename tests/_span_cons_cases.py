"""Shared by the tests of span folds under structure constraints (rh_span_fold_constrained, rh_span_fold_batch_constrained): the
cases, and the reference -- the Vienna-BL oracle under band_mask(n, L) & constraint_mask(cons, n), computed once per key and left
unchanged.  oracle/vienna_oracle.c applies the mask to every pair test of its DP and of its brute-force enumeration.

A constraint is laid out by edge_constraint(n, L) from features at fixed letters (1-based), each present where the sequence is long
enough and the span limit admits it:
  x run 62..67            across entries 64 / 65, the block edge of the exterior passes
  < run 100..103, > run 120..123
  helix 253..258 with 266..271   six nested brackets whose letters straddle column 256, the workgroup edge of the sweeps (enc
                          differs between neighbours); at n = 257 the helix 243..246 with 254..257 instead, which also ends on
                          the last letter
  bracket (150, 150+L-1)  a pair spanning exactly L - 1 (at L = 2: the adjacent "()"); where the sequence ends before it, the pair
                          (1, L) if L <= n
  bracket (200, 202)      fewer than three letters inside: the pair itself cannot form, what conflicts with it is still removed
  short sequences         x at 5..6, bracket (8, 12), helix 20..22 with 30..32, < at 40..41, > at 50..51
Trailing '.' are cut off, so the string is shorter than n wherever the last letters are free.  plant() then makes the letters of
every bracket pair complementary, as the pre-pass demands."""
import numpy as np

import _span_cases as sc
from _oracle import constraint_mask

_refs = {}
COMP = {"G": "C", "C": "G", "A": "U", "U": "A", "N": "C"}


def edge_constraint(n, L):
    c = ["."] * (n + 1)          # 1-based

    def run(ch, a, b):
        for k in range(a, min(b, n) + 1):
            if c[k] == ".":
                c[k] = ch

    def pair(a, b):
        if 1 <= a < b <= n and b - a < L and c[a] == "." and c[b] == ".":
            c[a], c[b] = "(", ")"

    def helix(a, b, k):          # a..a+k-1 with b-k+1..b
        if b <= n and b - a < L:
            for m in range(k):
                pair(a + m, b - m)

    if n >= 150 + L - 1:
        pair(150, 150 + L - 1)
    elif L <= n:
        pair(1, L)
    run("x", 62, 67)
    run("<", 100, 103)
    run(">", 120, 123)
    if n == 257:
        helix(243, 257, 4)
    helix(253, 271, 6)
    pair(200, 202)
    if n < 150:
        run("x", 5, 6)
        pair(8, 12)
        helix(20, 32, 3)
        run("<", 40, 41)
        run(">", 50, 51)
        if L == 2:
            pair(8, 9)
    return "".join(c[1:]).rstrip(".")


def plant(seq, cons, L=None):
    """seq with the 3' letter of every matched bracket pair replaced by the complement of its 5' letter; L: every pair lies within it"""
    s, stack = list(seq), []
    for j, ch in enumerate(cons[:len(seq)]):
        if ch == "(":
            stack.append(j)
        elif ch == ")":
            i = stack.pop()
            assert L is None or j - i < L
            if s[i] not in "GCAU":
                s[i] = "G"
            s[j] = COMP[s[i]]
    assert not stack
    return "".join(s)


def case(n, L, seed=0):
    """(sequence, constraint) of length n for the span limit L"""
    cons = edge_constraint(n, L)
    return plant(sc.random_seq(n, seed=seed), cons, L), cons


# the single calls of the GPU suite: (n, L); L = 2 admits no pair at all (a hairpin needs three letters inside), with or without a constraint
SINGLE = [(300, 2), (300, 20), (300, 60), (257, 20), (257, 60), (70, 70), (70, 100)]
MAX_W = (1, 15)

# the short cases, within reach of the enumeration: (sequence, constraint, L).  The first is a G/C sequence with every kind of character.
SHORT = [(plant(s, t), t, L) for s, t, L in (
    ("GCGGCGCCGCGCCGCGGC", "..(..xx.....)<..>.", 18), ("GCGGCGCCGCGCCGCGGC", "..(..xx.....)<..>.", 12), ("GCGGCGCCGCGCCGCGGC", ".(.)..((....))<>", 8),
    ("GGGGCGCCGCCCCGCGGC", "(<<..>>..x.)", 12), ("GCGCGGCGCCGCGCUA", "()..x|..<...>", 2))]


def combined_mask(n, L, cons):
    m = constraint_mask(cons, n)
    return np.ascontiguousarray(m & sc.band_mask(n, L)) if L is not None else m


def masked_cons(seq, L, cons, max_w=1, bruteforce=False):
    """dict(logZ, band (n, min(L, n)), up (n, max_w)) of the oracle under band_mask(n, L) & constraint_mask(cons, n); cons = None: the
    band mask alone"""
    key = (seq, L, cons, max_w, bruteforce)
    if key not in _refs:
        vo, n = sc.oracle(), len(seq)
        mask = combined_mask(n, L, cons) if cons is not None else sc.band_mask(n, L)
        vo.L.vo_set_allow_mask(mask.ctypes.data)
        try:
            r = vo._fold_bruteforce(seq, max_w) if bruteforce else vo._mccaskill(seq, max_w, False)
        finally:
            vo.L.vo_set_allow_mask(None)
        band, up = sc.tri_to_band(r["post"], n, min(L, n)), r["up"]
        band.setflags(write=False)
        up.setflags(write=False)
        _refs[key] = dict(logZ=r["logZ"], band=band, up=up)
    return _refs[key]
