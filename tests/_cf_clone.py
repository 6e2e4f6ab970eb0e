"""Oracle for the CONTRAfold model's region accessibility, from the pinned oracle alone (oracle/cf_oracle.c is not touched).

up[i][w] = Z(letters i..i+w forbidden to pair) / Z, with Z the sum over the derivations the inside recurrences count.  The
numerator comes from a CLONE parameter file: a letter X' that scores like X in every unpaired context and pairs with nothing
that occurs in the sequence.  Recoding the letters of a region X -> X' then forbids exactly those letters from pairing and
changes nothing else, so

    up[i][w] = exp(logZ_clone(s recoded on i..i+w) - logZ(s)).

A clone file is derived from the bundled one: every parameter whose name ends in letters takes the value of the name with the
clone letters rewritten to their originals (or of its symmetric spelling, where the file keeps only one of the two), and the
base_pair scores under which a clone letter could pair are set to -1e4.  The files are test temporaries."""
import math
import os
import re

import numpy as np

from _oracle import PARAMS, Oracle, tri_offset

_SUFFIX = re.compile(r"^(.*_)([ACGU]+)$")


class Family:
    """alphabet: letters of the sequences; clone: clone letter -> the letter it scores like (also the recoding of a region, read
    backwards); disabled: the base_pair names that let a clone letter pair."""

    def __init__(self, name, alphabet, clone, disabled):
        self.name, self.alphabet, self.clone, self.disabled = name, alphabet, clone, disabled
        self.recode = {orig: c for c, orig in clone.items()}


FAMILIES = {
    "AU": Family("AU", "AU", {"C": "A", "G": "U"}, ("base_pair_CG", "base_pair_GU")),
    "CG": Family("CG", "CG", {"A": "G", "U": "C"}, ("base_pair_AU", "base_pair_GU")),
    "AUG": Family("AUG", "AUG", {"C": "A"}, ("base_pair_CG",)),   # regions inside runs of A only
}


def read_params(path=PARAMS):
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip()]
    return [(name, float(v)) for name, v in rows]


def clone_params(family, rows=None):
    """The (name, value) rows of the clone file of `family`."""
    rows = rows or read_params()
    table = dict(rows)
    out = []
    for name, v in rows:
        m = _SUFFIX.match(name)
        if m:
            stem, letters = m.group(1), "".join(family.clone.get(c, c) for c in m.group(2))
            half = len(letters) // 2
            for spelling in (letters, letters[::-1], letters[half:] + letters[:half]):
                if stem + spelling in table:
                    v = table[stem + spelling]
                    break
            else:
                raise KeyError("no parameter under any spelling of " + stem + letters)
        out.append((name, v))
    return [(name, -1e4 if name in family.disabled else v) for name, v in out]


def write_clone(path, family):
    with open(path, "w") as f:
        for name, v in clone_params(family):
            f.write("%s %r\n" % (name, v))
    return path


class CloneOracle:
    """The pinned oracle with the bundled parameters and the clone file of one family (written into `tmpdir`)."""

    def __init__(self, family, tmpdir):
        self.family = FAMILIES[family] if isinstance(family, str) else family
        self.o = Oracle()
        path = write_clone(os.path.join(str(tmpdir), "clone_%s.params" % self.family.name), self.family)
        self.clone = self.o.L.cfo_load_params(path.encode())
        assert self.clone, "the oracle does not take the clone file " + path
        self._logz = {}

    def _z(self, model, seq, post=None):
        return self.o.L.cfo_inference(model, seq.encode(), len(seq), post.ctypes.data if post is not None else None, None, None)

    def logz(self, seq):
        """log Z under the bundled parameters (memoised)."""
        if seq not in self._logz:
            self._logz[seq] = self._z(self.o.m, seq)
        return self._logz[seq]

    def logz_clone(self, seq):
        return self._z(self.clone, seq)

    def recoded(self, seq, i, w):
        region = seq[i:i + w + 1]
        assert len(region) == w + 1 and all(c in self.family.recode for c in region), "region leaves the sequence or the recodable letters"
        return seq[:i] + "".join(self.family.recode[c] for c in region) + seq[i + w + 1:]

    def unpaired1(self, seq):
        """1 - sum_j post(i, j) per letter, from the oracle's own posterior."""
        n = len(seq)
        post = np.zeros((n + 1) * (n + 2) // 2)
        self._z(self.o.m, seq, post)
        P = np.zeros((n + 1, n + 1))
        for i in range(1, n + 1):
            P[i, i + 1:] = post[tri_offset(n, i) + i + 1:tri_offset(n, i) + n + 1]
        return 1.0 - (P + P.T).sum(axis=1)[1:]

    def pair_rows(self, seq):
        """P(letter i is paired), 0-based, from the oracle's posterior."""
        return 1.0 - self.unpaired1(seq)


def region_up(oracle, seq, i, w):
    """up[i][w] = P(letters i..i+w unpaired), 0-based i, w = width - 1."""
    return math.exp(oracle.logz_clone(oracle.recoded(seq, i, w)) - oracle.logz(seq))


def random_seq(rng, n, alphabet):
    return "".join(alphabet[k] for k in rng.integers(0, len(alphabet), n))
