"""Shared by the span-fold tests: the band mask that turns the Vienna-BL oracle into the span-limited checker, references computed
once per (sequence, L), and the long factorising sequence.

oracle/vienna_oracle.c applies vo_set_allow_mask to every pair test of its DP and of its brute-force enumeration, so the mask
allow[a][b] = 1 iff b - a < L (1-based a < b) makes both the ensemble of rh_span_fold."""
import hashlib

import numpy as np

from _oracle import ViennaOracle, tri_offset

_vo = {}
_refs = {}


def file_key(params):
    """what the caches name a table file by: its path and a digest of what it holds now, so that a file written again under the same
    name is another file (None: the bundled BL* file)"""
    if params is None:
        return None
    with open(params, "rb") as f:
        return params, hashlib.sha1(f.read()).hexdigest()


def oracle(params=None):
    """the oracle on a table file (None: the bundled BL* file), one per file and content"""
    key = file_key(params)
    if key not in _vo:
        _vo[key] = ViennaOracle(params)
    return _vo[key]


def band_mask(n, L):
    a, b = np.arange(n + 1)[:, None], np.arange(n + 1)[None, :]
    m = ((a >= 1) & (b > a) & (b - a < L)).astype(np.uint8)
    return np.ascontiguousarray(m)


def tri_to_band(tri, n, ld):
    """band[i, d] = P(i, i + d), 0-based i, of a triangular table; pairs further apart than the band is wide must be 0 there"""
    band = np.zeros((n, ld))
    for i in range(n):
        at = tri_offset(n, i + 1) + i + 2
        row = np.asarray(tri[at:at + n - 1 - i])
        m = min(ld - 1, n - 1 - i)
        band[i, 1:1 + m] = row[:m]
        assert not row[m:].any(), "the reference has a pair beyond the band"
    return band


def masked(seq, L, bruteforce=False, params=None):
    """dict(logZ, band (n, min(L, n)), up (n, 1), post) of the oracle under the band mask; L = None: no mask; params: the table file"""
    key = (seq, L, bruteforce, file_key(params))
    if key not in _refs:
        vo, n = oracle(params), len(seq)
        mask = band_mask(n, L) if L is not None else None
        vo.L.vo_set_allow_mask(mask.ctypes.data if mask is not None else None)
        try:
            r = vo._fold_bruteforce(seq, 1) if bruteforce else vo._mccaskill(seq, 1, False)
        finally:
            vo.L.vo_set_allow_mask(None)
        ld = min(L, n) if L is not None else n
        _refs[key] = dict(logZ=r["logZ"], post=r["post"], band=tri_to_band(r["post"], n, ld), up=r["up"])
    return _refs[key]


def random_seq(n, seed=0, alphabet="ACGU", plant_n=True):
    s = list(np.random.RandomState(20261021 + 7 * n + seed).choice(list(alphabet), n))
    if plant_n and n >= 8:
        s[n // 3] = "N"
    return "".join(s)


# ---- the long sequence: inserts of G/C letters between spacers of A.  A pairs with neither G, C nor A and a spacer of L - 1
# letters keeps the letters of two inserts at least L apart, so the ensemble factorises: band and up on an insert are those of the
# unmasked oracle on "A" + insert + "A", and log Z is the sum over the inserts.
def inserts(count, length, distinct=6, seed=5):
    rs = np.random.RandomState(20261021 + seed)
    kinds = ["".join(rs.choice(list("GC"), length)) for _ in range(distinct)]
    return [kinds[k % distinct] for k in range(count)]


def long_sequence(n, L, ins, lead=1, gaps=None):
    """(sequence, 0-based starts of the inserts): `lead` A's, then every insert followed by L - 1 A's (gaps[k] A's where given),
    then A's up to n letters"""
    parts, starts, at = ["A" * lead], [], lead
    for k, s in enumerate(ins):
        g = (gaps or {}).get(k, L - 1)
        starts.append(at)
        parts.append(s + "A" * g)
        at += len(s) + g
    assert at <= n
    parts.append("A" * (n - at))
    return "".join(parts), starts


def insert_reference(s):
    """the unmasked oracle on "A" + s + "A", cut back to the insert: (log Z, band (len, len), up (len,))"""
    r = masked("A" + s + "A", None)
    m = len(s)
    return r["logZ"], r["band"][1:1 + m, :m], r["up"][1:1 + m, 0]
