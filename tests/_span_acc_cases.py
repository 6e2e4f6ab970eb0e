"""Shared by the tests of region accessibility on span folds (rh_span_fold_acc): the Vienna-BL oracle under the band mask of
tests/_span_cases.py with widths above one, computed once per (sequence, L, max_w) and left unchanged, and the reference runs of
the long factorising sequence.

up[i, w] = P(letters i .. i + w unpaired), 0-based, and 0 where the run passes the last letter."""
import numpy as np

import _span_cases as sc

_refs = {}


def masked_acc(seq, L, max_w, bruteforce=False, params=None):
    """dict(logZ, band (n, min(L, n)), up (n, max_w)) of the oracle under the band mask; L = None: no mask; params: the table file"""
    key = (seq, L, max_w, bruteforce, sc.file_key(params))
    if key not in _refs:
        vo, n = sc.oracle(params), len(seq)
        mask = sc.band_mask(n, L) if L is not None else None
        vo.L.vo_set_allow_mask(mask.ctypes.data if mask is not None else None)
        try:
            r = vo._fold_bruteforce(seq, max_w) if bruteforce else vo._mccaskill(seq, max_w, False)
        finally:
            vo.L.vo_set_allow_mask(None)
        ld = min(L, n) if L is not None else n
        up = r["up"]
        up.setflags(write=False)
        _refs[key] = dict(logZ=r["logZ"], band=sc.tri_to_band(r["post"], n, ld), up=up)
    return _refs[key]


def insert_acc_reference(s, max_w):
    """up (len, max_w) on an insert of the factorising sequence: the unmasked oracle on "A" + s + "A", cut back to the insert.  A run
    that leaves the insert runs on into the spacer, whose letters are unpaired with probability 1: it equals the run cut at the
    insert's last letter, which is what the columns past it are filled with."""
    m = len(s)
    up = masked_acc("A" + s + "A", None, max_w)["up"][1:1 + m].copy()
    for i in range(m):
        last = m - 1 - i                      # the widest run from i that stays on the insert
        if last + 1 < max_w:
            up[i, last + 1:] = up[i, last]
    return up
