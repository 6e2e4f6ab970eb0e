"""The checker of span folds under the CONTRAfold model: a numpy restatement of cfo_inference (oracle/cf_oracle.c: inside, outside,
posterior) with one addition -- a predicate allow(a, b) on the letters a < b (1-based) that is and-ed into `pairable`, the only
place where those recurrences admit a pair.  oracle/cf_oracle.c has no pair mask, so the band b - a < L needs this.

Written from the recurrences: plain linear doubles (n stays <= 300, where log Z is about 30 nats), tables diagonal-major
T[d, i] = T(i, j = i + d) in the oracle's gap indexing, one numpy step per diagonal with the single-branch shapes gathered as a
(shape, cell) matrix.  The outside is the oracle's push form turned into pulls, term for term; the posterior of a pair is
FCo x FCi / Z, which is the sum the oracle's three posterior loops accumulate.  The weight file ("name value" rows) is read here:
the tying of symmetric spellings and the prefix sums of the *_at_least_k rows as cfo_load_params does them.

tests/test_cf_span_ref_cpu.py pins it three ways: without a mask against the oracle, under region masks against the clone oracle,
under band masks where the unmasked oracle knows the answer.

Measured on one CPU core: a reference at (n, L) = (300, 60) takes 0.18 s, (130, 65) 0.05 s, n = 80 without a mask 0.04 s.
"""
import hashlib

import numpy as np

from _oracle import PARAMS, tri_offset, tri_size
from _span_cases import tri_to_band

ALPHA = "ACGU"
MINHAIRPIN = 3
_models, _refs = {}, {}


def _code(ch):
    return ALPHA.index(ch.upper()) if ch.upper() in ALPHA else 4


class Model:
    """the scoring tables of one weight file; index 4 (an unknown letter, the sentinels) scores 0 everywhere"""

    def __init__(self, path):
        rows = {}
        with open(path) as f:
            for line in f:
                parts = line.split()
                if len(parts) == 2:
                    rows[parts[0]] = float(parts[1])
        get = rows.__getitem__
        tied = lambda a, b: get(min(a, b))
        A = range(4)
        self.base_pair = np.zeros((5, 5))
        self.helix_closing = np.zeros((5, 5))
        self.internal_1x1 = np.zeros((5, 5))
        self.terminal_mismatch = np.zeros((5, 5, 5, 5))
        self.helix_stacking = np.zeros((5, 5, 5, 5))
        self.dangle_left = np.zeros((5, 5, 5))
        self.dangle_right = np.zeros((5, 5, 5))
        self.bulge_0x1 = np.zeros(5)
        for i in A:
            x = ALPHA[i]
            self.bulge_0x1[i] = get("bulge_0x1_nucleotides_" + x)
            for j in A:
                y = ALPHA[j]
                self.base_pair[i, j] = tied("base_pair_" + x + y, "base_pair_" + y + x)
                self.helix_closing[i, j] = get("helix_closing_" + x + y)
                self.internal_1x1[i, j] = tied("internal_1x1_nucleotides_" + x + y, "internal_1x1_nucleotides_" + y + x)
                for k in A:
                    z = ALPHA[k]
                    self.dangle_left[i, j, k] = get("dangle_left_" + x + y + z)
                    self.dangle_right[i, j, k] = get("dangle_right_" + x + y + z)
                    for l in A:
                        w = ALPHA[l]
                        self.terminal_mismatch[i, j, k, l] = get("terminal_mismatch_" + x + y + z + w)
                        self.helix_stacking[i, j, k, l] = tied("helix_stacking_" + x + y + z + w, "helix_stacking_" + w + z + y + x)
        self.bulge_1x0 = self.bulge_0x1   # one row feeds both tables

        def prefix(name, lo, hi):
            out = np.zeros(hi + 1)
            for k in range(lo, hi + 1):
                out[k] = (out[k - 1] if k > 0 else 0.0) + get("%s_%d" % (name, k))
            return out
        self.hairpin_len = prefix("hairpin_length_at_least", 0, 30)
        bulge = prefix("bulge_length_at_least", 1, 30)
        inter = prefix("internal_length_at_least", 2, 30)
        sym = prefix("internal_symmetric_length_at_least", 1, 15)
        asym = prefix("internal_asymmetry_at_least", 1, 28)
        self.single_len = np.zeros((31, 31))
        for l1 in range(31):
            for l2 in range(31 - l1):
                if l1 == 0 and l2 == 0:
                    continue
                if l1 == 0 or l2 == 0:
                    v = bulge[min(l1 + l2, 30)]
                else:
                    v = inter[min(l1 + l2, 30)] + asym[min(abs(l1 - l2), 28)]
                    if l1 <= 4 and l2 <= 4:
                        v += get("internal_explicit_%d_%d" % (min(l1, l2), max(l1, l2)))
                    if l1 == l2:
                        v += sym[min(l1, 15)]
                self.single_len[l1, l2] = v
        self.multi_base, self.multi_unpaired, self.multi_paired = get("multi_base"), get("multi_unpaired"), get("multi_paired")
        self.external_unpaired, self.external_paired = get("external_unpaired"), get("external_paired")
        # the generic shapes: everything but stacking, 0x1, 1x0, 1x1
        sh = [(l1, t - l1) for t in range(2, 31) for l1 in range(t + 1) if not (t == 2 and l1 == 1)]
        self.sh_l1 = np.array([a for a, _ in sh])
        self.sh_l2 = np.array([b for _, b in sh])
        self.sh_w = np.exp(self.single_len[self.sh_l1, self.sh_l2])


def file_digest(params):
    with open(params or PARAMS, "rb") as f:
        return hashlib.sha1(f.read()).hexdigest()


def model(params=None):
    key = file_digest(params)
    if key not in _models:
        _models[key] = Model(params or PARAMS)
    return _models[key]


def inference(seq, allow=None, params=None):
    """dict(logZ, post) as Oracle.inference returns them (post triangular, 1-based letters) of the ensemble in which letters
    a < b pair only if they are complementary and allow(a, b) holds (allow: a function of two integer arrays, or None)."""
    M = model(params)
    n = len(seq)
    s = np.array([4] + [_code(c) for c in seq] + [4, 4])           # s[0] = s[n+1] = 4 (and one more for the reads at j + 2 = n + 2)
    comp = np.zeros((5, 5), dtype=bool)
    for a, b in ("AU", "UA", "GU", "UG", "CG", "GC"):
        comp[ALPHA.index(a), ALPHA.index(b)] = True
    W = n + 3
    shape = (n + 2, W)
    d_, i_ = np.meshgrid(np.arange(n + 2), np.arange(W), indexing="ij")
    j_ = i_ + d_
    cell = (i_ >= 1) & (j_ <= n - 1)                               # 0 < i, j < L: the cells of FC
    ic, jc = np.where(cell, i_, 1), np.where(cell, j_, 1)
    si, sip, sim, sj, sjp, sjpp = s[ic], s[ic + 1], s[ic - 1], s[jc], s[jc + 1], s[jc + 2]
    ok = cell & comp[si, sjp]
    if allow is not None:
        ok &= np.asarray(allow(ic, jc + 1), dtype=bool)
    mp, mb, mu = M.multi_paired, M.multi_base, M.multi_unpaired
    eu, ep = M.external_unpaired, M.external_paired
    # the pair (i, j+1) as the enclosing pair of a loop ...
    jb_enc = np.exp(M.helix_closing[si, sjp] + M.terminal_mismatch[si, sjp, sip, sj])
    ja_enc = np.exp(M.helix_closing[si, sjp] + M.dangle_left[si, sjp, sip] + np.where(jc > 0, M.dangle_right[si, sjp, sj], 0.0))
    stack = np.exp(M.helix_stacking[si, sjp, sip, sj])
    n01, n10, n11 = np.exp(M.bulge_0x1[sj]), np.exp(M.bulge_1x0[sip]), np.exp(M.internal_1x1[sip, sj])
    # ... and as the enclosed one: base_pair(i, j+1) with junction_b(j+1, i-1) resp. junction_a(j+1, i-1)
    bp = np.exp(M.base_pair[si, sjp])
    dec_b = bp * np.exp(M.helix_closing[sjp, si] + M.terminal_mismatch[sjp, si, sjpp, sim])
    dec_a = bp * np.exp(M.helix_closing[sjp, si] + np.where(jc + 1 < n, M.dangle_left[sjp, si, sjpp], 0.0) +
                        np.where(ic - 1 > 0, M.dangle_right[sjp, si, sim], 0.0))
    w01, w10, w11 = np.exp(M.single_len[0, 1]), np.exp(M.single_len[1, 0]), np.exp(M.single_len[1, 1])
    e_mu, e_mp, e_close = np.exp(mu), np.exp(mp), np.exp(mp + mb)

    dmax = int(d_[ok].max()) if ok.any() else -1                   # nothing above it feeds a pair
    FC, FCB, FCA, FCS = (np.zeros(shape) for _ in range(4))      # FC; times dec_b; times dec_a; times bp (the stacking shape)
    FM1, FM = np.zeros(shape), np.zeros(shape)
    for d in range(dmax + 1):
        i = np.arange(1, n - d)                                    # j = i + d <= n - 1
        if i.size == 0:
            break
        fm2 = np.zeros(i.size)
        if d >= 3:
            m = np.arange(1, d)[:, None]
            fm2 = (FM1[m, i[None, :]] * FM[d - m, i[None, :] + m]).sum(0)
        acc = np.zeros(i.size)
        if d >= MINHAIRPIN:
            acc += np.exp(M.hairpin_len[min(d, 30)])
        use = M.sh_l1 + M.sh_l2 <= d - 2
        if use.any():
            l1, l2 = M.sh_l1[use][:, None], M.sh_l2[use][:, None]
            acc += (M.sh_w[use][:, None] * FCB[d - 2 - l1 - l2, i[None, :] + 1 + l1]).sum(0)
        if d >= 3:
            acc += w01 * n01[d, i] * FCB[d - 3, i + 1] + w10 * n10[d, i] * FCB[d - 3, i + 2]
        if d >= 4:
            acc += w11 * n11[d, i] * FCB[d - 4, i + 2]
        fc = jb_enc[d, i] * acc
        if d >= 2:
            fc += FCS[d - 2, i + 1] * stack[d, i]
        fc += fm2 * ja_enc[d, i] * e_close
        fc = np.where(ok[d, i], fc, 0.0)
        FC[d, i], FCB[d, i], FCA[d, i], FCS[d, i] = fc, fc * dec_b[d, i], fc * dec_a[d, i], fc * bp[d, i]
        if d >= 2:
            FM1[d, i] = FCA[d - 2, i + 1] * e_mp + FM1[d - 1, i + 1] * e_mu
            FM[d, i] = fm2 + FM[d - 1, i] * e_mu + FM1[d, i]
    F5i, F5o = np.zeros(n + 1), np.zeros(n + 1)
    F5i[0] = F5o[n] = 1.0
    e_eu, e_ep = np.exp(eu), np.exp(ep)
    for j in range(1, n + 1):
        k = np.arange(max(0, j - 2 - dmax), j - 1)
        F5i[j] = F5i[j - 1] * e_eu + (F5i[k] * FCA[j - k - 2, k + 1]).sum() * e_ep
    for k in range(n - 1, -1, -1):
        j = np.arange(k + 2, min(n, k + 2 + dmax) + 1)
        F5o[k] = F5o[k + 1] * e_eu + (F5o[j] * FCA[j - k - 2, k + 1]).sum() * e_ep
    Z = F5i[n]

    FCo, FCoB = np.zeros(shape), np.zeros(shape)                   # FCo; times jb_enc (what an enclosed pair reads)
    FMo, FM1o, FM2o = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for d in range(dmax, -1, -1):
        i = np.arange(1, n - d)
        if i.size == 0:
            continue
        j = i + d
        if d >= 2:
            fmo = FMo[d + 1, i] * e_mu
            fm1o = FM1o[d + 1, i - 1] * e_mu
            emax = dmax - d
            if emax >= 1:
                e = np.arange(1, emax + 1)[:, None]
                src = i[None, :] - e
                fmo = fmo + np.where(src >= 1, FM2o[d + e, np.maximum(src, 0)] * FM1[e, np.maximum(src, 0)], 0.0).sum(0)
                dst = np.minimum(j[None, :], n)
                fm1o = fm1o + (FM2o[d + e, i[None, :]] * FM[e, dst]).sum(0)
            fm1o = fm1o + fmo
            FMo[d, i], FM1o[d, i] = fmo, fm1o
        out = F5i[i - 1] * F5o[j + 1] * e_ep * dec_a[d, i]
        if d + 2 <= dmax:
            out = out + FM1o[d + 2, i - 1] * e_mp * dec_a[d, i]
        acc = np.zeros(i.size)
        use = M.sh_l1 + M.sh_l2 <= dmax - d - 2
        if use.any():
            l1, l2 = M.sh_l1[use][:, None], M.sh_l2[use][:, None]
            io = i[None, :] - 1 - l1
            acc += (M.sh_w[use][:, None] * np.where(io >= 1, FCoB[d + 2 + l1 + l2, np.maximum(io, 0)], 0.0)).sum(0)
        # the enclosing pair of a 0x1 / 1x0 / 1x1 loop reads ITS letters: (io + 1, jo) = (i, j + 2), (i - 1, j + 1), (i - 1, j + 2)
        if d + 3 <= dmax:
            acc += w01 * np.exp(M.bulge_0x1[s[j + 2]]) * FCoB[d + 3, i - 1]
            acc += w10 * np.exp(M.bulge_1x0[s[i - 1]]) * np.where(i >= 2, FCoB[d + 3, np.maximum(i - 2, 0)], 0.0)
        if d + 4 <= dmax:
            acc += w11 * np.exp(M.internal_1x1[s[i - 1], s[j + 2]]) * np.where(i >= 2, FCoB[d + 4, np.maximum(i - 2, 0)], 0.0)
        out = out + acc * dec_b[d, i]
        if d + 2 <= dmax:   # stacked on (i - 1, j + 2): base_pair of this pair, helix_stacking of the enclosing one
            out = out + FCo[d + 2, i - 1] * bp[d, i] * stack[d + 2, i - 1]
        out = np.where(ok[d, i], out, 0.0)
        FCo[d, i], FCoB[d, i] = out, out * jb_enc[d, i]
        FM2o[d, i] = FMo[d, i] + out * ja_enc[d, i] * e_close
    post = np.zeros(tri_size(n))
    for a in range(1, n):
        dd = np.arange(0, min(dmax, n - 1 - a) + 1)
        post[tri_offset(n, a) + a + 1 + dd] = np.clip(FCo[dd, a] * FC[dd, a] / Z, 0.0, 1.0)
    return dict(logZ=float(np.log(Z)), post=post, f5i=F5i, fca=FCA * e_ep, eu=eu)


def band_allow(L):
    return lambda a, b: b - a < L


def span_ref(seq, L, params=None):
    """dict(logZ, post, band (n, min(L, n)), up (n, 1)) of the span-limited ensemble; cached per (sequence, L, file digest)"""
    key = (seq, L, file_digest(params))
    if key not in _refs:
        n = len(seq)
        r = inference(seq, band_allow(L), params)
        band = tri_to_band(r["post"], n, min(L, n))
        paired = band.sum(1)                                       # P(i, i + d) over d ...
        for d in range(1, band.shape[1]):
            paired[d:] += band[:n - d, d]                          # ... and P(i - d, i)
        _refs[key] = dict(r, band=band, up=np.maximum(0.0, 1.0 - paired)[:, None])
    return _refs[key]
