"""The yardstick of region accessibility on span folds under the CONTRAfold model: two runs of the masked restatement
(tests/_cf_span_ref.py: inference(seq, allow)), so it shares nothing with the five-term decomposition of the kernels:

    up_ref[i, w] = exp(logZ(band and neither letter in i+1 .. i+1+w) - logZ(band))          (letters 1-based, i 0-based)

Results are cached per (sequence, L, weight file, entry).  Measured on one core, per region: n = 41, L = 20: 0.009 s;
n = 66, L = 33: 0.024 s; n = 130, L = 64: 0.10 s -- so every region only up to about 41 letters, lists or samples beyond."""
import math

import numpy as np

import _cf_span_ref as ref

_UP = {}


def region_allow(L, i, w):
    """the band, and no letter of the 0-based region i .. i + w"""
    lo, hi = i + 1, i + 1 + w
    return lambda a, b: (b - a < L) & ~((a >= lo) & (a <= hi)) & ~((b >= lo) & (b <= hi))


def up_ref(seq, L, entries, params=None):
    """the yardstick at the entries (i, w), an array in their order"""
    key = (seq, L, ref.file_digest(params))
    have = _UP.setdefault(key, {})
    base = ref.span_ref(seq, L, params)["logZ"]
    for i, w in entries:
        if (i, w) not in have:
            have[(i, w)] = math.exp(ref.inference(seq, region_allow(L, i, w), params)["logZ"] - base)
    return np.array([have[e] for e in entries])


def every(n, max_w):
    return [(i, w) for i in range(n) for w in range(max_w) if i + w < n]


def sampled(n, max_w, count, seed):
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < count:
        w = int(rng.integers(0, max_w))
        if w < n:
            out.add((int(rng.integers(0, n - w)), w))
    return sorted(out)


def past_the_end(n, max_w):
    return [(i, w) for i in range(n) for w in range(max_w) if i + w >= n]


def comp(s):
    return "".join({"G": "C", "C": "G", "A": "U", "U": "A"}[c] for c in reversed(s))


def planted_multiloop(branches):
    """tests/test_gpu_cf_accessibility.py::planted_multiloop: an 8-pair helix closing `branches` hairpins of 8 pairs, one G between
    them and six trailing letters before the closing pair; the sequence and the 0-based trailing run"""
    lefts = ["GCGCGGCG", "GGCCGCGG", "GCCGGCCG", "GGGCGCCG", "GCGGCCGG"]
    seq = lefts[-1]
    for b in lefts[:branches]:
        seq += "G" + b + "GGGG" + comp(b)
    t0 = len(seq)
    seq += "GGGGGG" + comp(lefts[-1])
    return seq, list(range(t0, t0 + 6))


def multiloop_entries(seq, trail):
    """the entries of that file's multiloop test"""
    entries = [(i, w) for i in trail for w in range(6) if i + w <= trail[-1]]
    entries += [(i, w) for i in range(trail[0] - 3, trail[-1] + 2) for w in (0, 1, 6, 10) if i + w < len(seq)]
    return sorted(set(entries))


def planted_side(side):
    """that file's interior loop with one side of `side` unpaired letters; sequence, entries, (outer 5' letter, outer 3' letter) 1-based"""
    inner = "GCGGC" + "GGGG" + "GCCGC"
    seq = "GCGGCGC" + "G" * side + inner + "GCGCCGC"
    i0 = 7
    entries = [(i, w) for i in range(i0 - 1, i0 + side) for w in (1, 7, 14, 27, 28, 29, 30, 31) if i + w < len(seq)]
    return seq, entries, (7, len(seq) - 6)


def hairpin_of_forty():
    stem = "GCGGCGGC"
    return stem + "G" * 40 + comp(stem)
