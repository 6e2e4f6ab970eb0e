"""CONTRAfold weight files other than the bundled one, for tests/test_contrafold_weights_cpu.py and tests/test_gpu_contrafold_weights.py.

A file is a list of (name, value) rows in the "name value" format of ractip_amd/data/contrafold_complementary.params: the 708 spellings
that file lists and no others (of two tied spellings only the lexicographically smaller one exists).  Binding is by name in the oracle
and in the product, so write() shuffles the rows.

scrambled(seed): every row of the bundled file moved by a uniform offset drawn in file order from RandomState(seed): +-AMP_LETTERS on
the letter-indexed rows and the five scalars, +-AMP_NUMBERED on the numbered rows (`*_at_least_k`, `internal_explicit_a_b`), which the
loaders prefix-sum over up to 30 entries.  The rows that are 0 in the bundled file move like the others.

The committed pair is SEED = 19 at 0.2 / 0.03.  It is chosen against two assertions of tests/test_contrafold_weights_cpu.py, on the
oracle alone: every in-budget shape of _contrafold_cases.shape_set() (496 inputs) keeps both middle stem letters paired with probability
>= 0.9 (measured minimum 0.9825; seed 18 at the same amplitudes gives 0.63, seed 20 at 0.1 / 0.02 gives 0.9954), and one letter past the
loop budget the outer stem loses its probability as it does under the bundled file.

unread_rows(): the letter-indexed names that no derivation of the model reads, because the letters in their PAIR slots are not
complementary (AU, CG, GU either way): the first two letters of terminal_mismatch / dangle_left / dangle_right / helix_closing /
base_pair, either pair (letters 1-2, letters 3-4) of helix_stacking.  Derived from the names; that these are exactly the zero
letter-indexed rows of the bundled file is a test.

mutants(rows): name -> rows, each a rewrite of NAMES (a permutation of values among the 708 rows), so that the oracle and the product
both load it: what a kernel or a host-built table computes if it mixes up two indices of one table or two tables."""
import re

import numpy as np

from _oracle import PARAMS

SEED, AMP_LETTERS, AMP_NUMBERED = 19, 0.2, 0.03
NROWS = 708
_NUMBERED = re.compile(r"^(.*?)_(\d+)(?:_(\d+))?$")
_LETTERS = re.compile(r"^(.*)_([ACGU]+)$")
PAIRED_TABLES = ("terminal_mismatch", "dangle_left", "dangle_right", "helix_closing", "base_pair")     # letters 1-2 are a pair
UNREAD_COUNTS = {"terminal_mismatch": 160, "dangle_left": 40, "dangle_right": 40, "helix_stacking": 115, "helix_closing": 10, "base_pair": 7}


def read(path=PARAMS):
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip()]
    return [(name, float(v)) for name, v in rows]


def write(path, rows, seed=0):
    """The rows in a shuffled order (binding is by name); values with repr, so that they read back bit for bit.  Returns the path."""
    order = np.random.RandomState(seed).permutation(len(rows))
    with open(str(path), "w") as f:
        for k in order:
            f.write("%s %r\n" % (rows[k][0], float(rows[k][1])))
    return str(path)


def is_numbered(name):
    return _NUMBERED.match(name) is not None


def scrambled(seed=SEED, amp_letters=AMP_LETTERS, amp_numbered=AMP_NUMBERED):
    rng = np.random.RandomState(seed)
    out = []
    for name, v in read():
        u = rng.uniform(-1.0, 1.0)
        out.append((name, v + u * (amp_numbered if is_numbered(name) else amp_letters)))
    return out


def complementary(a, b):
    return a + b in ("AU", "UA", "CG", "GC", "GU", "UG")


def split_letters(name):
    """(table, letters) of a letter-indexed name, else (name, None)"""
    m = _LETTERS.match(name)
    return (m.group(1), m.group(2)) if m else (name, None)


def is_unread(name):
    table, x = split_letters(name)
    if x is None:
        return False
    if table in PAIRED_TABLES:
        return not complementary(x[0], x[1])
    if table == "helix_stacking":       # [s_i][s_j][s_i+1][s_j-1]: (i, j) and (i + 1, j - 1) are both pairs
        return not (complementary(x[0], x[1]) and complementary(x[2], x[3]))
    return False


def unread_rows(rows=None):
    return [name for name, _ in (rows or read()) if is_unread(name)]


def with_unread_moved(rows, delta):
    return [(name, v + delta if is_unread(name) else v) for name, v in rows]


# ---- the mutants: value of row `name` taken from row rename(name)
def _renamed(rows, rename):
    table = dict(rows)
    out = []
    for name, v in rows:
        src = rename(name)
        out.append((name, table[src] if src is not None and src in table else v))
    assert len(out) == len(rows)
    return out


def _letters_map(table, perm, tied=None):
    """rename of `table`: letters x -> perm(x); tied(spelling) -> the spelling the file keeps"""
    def rename(name):
        t, x = split_letters(name)
        if t != table or x is None:
            return None
        y = perm(x)
        return t + "_" + (tied(y) if tied else y)
    return rename


def _swap_tables(a, b):
    def rename(name):
        if name == a or name.startswith(a + "_"):
            return b + name[len(a):]
        if name == b or name.startswith(b + "_"):
            return a + name[len(b):]
        return None
    return rename


def _shift_numbered(rows, prefix):
    """row k takes the value of row k + 1, the last one that of the first"""
    ks = sorted(int(m.group(2)) for m in (_NUMBERED.match(n) for n, _ in rows) if m and m.group(1) == prefix and m.group(3) is None)

    def rename(name):
        m = _NUMBERED.match(name)
        if m and m.group(1) == prefix and m.group(3) is None:
            return "%s_%d" % (prefix, ks[(ks.index(int(m.group(2))) + 1) % len(ks)])
        return None
    return rename


ROT = {"A": "C", "C": "G", "G": "U", "U": "A"}
_min_rev = lambda y: min(y, y[::-1])


def mutants(rows):
    def swap_exact(a, b):
        return lambda name: b if name == a else (a if name == b else None)
    return {
        "terminal_mismatch letters 3 <-> 4": _renamed(rows, _letters_map("terminal_mismatch", lambda x: x[0] + x[1] + x[3] + x[2])),
        "terminal_mismatch pair letters swapped": _renamed(rows, _letters_map("terminal_mismatch", lambda x: x[1] + x[0] + x[2] + x[3])),
        "dangle_left <-> dangle_right": _renamed(rows, _swap_tables("dangle_left", "dangle_right")),
        "dangle_left pair letters swapped": _renamed(rows, _letters_map("dangle_left", lambda x: x[1] + x[0] + x[2])),
        "helix_closing letters swapped": _renamed(rows, _letters_map("helix_closing", lambda x: x[1] + x[0])),
        "multi_paired <-> external_paired": _renamed(rows, swap_exact("multi_paired", "external_paired")),
        "multi_unpaired <-> external_unpaired": _renamed(rows, swap_exact("multi_unpaired", "external_unpaired")),
        # WXYZ is tied with ZYXW; outer <-> inner pair is YZWX (tied with XWZY), which is another weight unless YZWX is WXYZ or ZYXW
        "helix_stacking outer <-> inner pair": _renamed(rows, _letters_map("helix_stacking", lambda x: x[2] + x[3] + x[0] + x[1], _min_rev)),
        "bulge_0x1_nucleotides letter rotation": _renamed(rows, _letters_map("bulge_0x1_nucleotides", lambda x: ROT[x[0]])),
        "internal_1x1_nucleotides letter rotation": _renamed(rows, _letters_map("internal_1x1_nucleotides", lambda x: ROT[x[0]] + ROT[x[1]], _min_rev)),     # (both: XY is tied with YX)
        "hairpin_length_at_least_k shifted by one": _renamed(rows, _shift_numbered(rows, "hairpin_length_at_least")),
        "bulge_length <-> internal_length": _renamed(rows, _swap_tables("bulge_length_at_least", "internal_length_at_least")),
        "internal_symmetric_length shifted by one": _renamed(rows, _shift_numbered(rows, "internal_symmetric_length_at_least")),
        "internal_asymmetry shifted by one": _renamed(rows, _shift_numbered(rows, "internal_asymmetry_at_least")),
        "internal_explicit_1_4 <-> internal_explicit_2_3": _renamed(rows, swap_exact("internal_explicit_1_4", "internal_explicit_2_3")),
        "multi_base <-> multi_paired": _renamed(rows, swap_exact("multi_base", "multi_paired")),
    }


# the families of tests/_contrafold_weight_cases.py whose compared quantities READ the table a mutant rewrites
MUTANT_FAMILIES = {
    "terminal_mismatch letters 3 <-> 4": ("fold", "letters", "hairpin", "duplex"),
    "terminal_mismatch pair letters swapped": ("fold", "letters", "hairpin", "duplex"),
    "dangle_left <-> dangle_right": ("fold", "exterior", "multiloop", "duplex"),
    "dangle_left pair letters swapped": ("fold", "exterior", "multiloop", "duplex"),
    "helix_closing letters swapped": ("fold", "letters", "hairpin", "duplex"),
    "multi_paired <-> external_paired": ("fold", "multiloop"),
    "multi_unpaired <-> external_unpaired": ("fold", "multiloop", "duplex"),
    "helix_stacking outer <-> inner pair": ("fold", "letters", "duplex"),
    "bulge_0x1_nucleotides letter rotation": ("fold", "letters", "duplex"),
    "internal_1x1_nucleotides letter rotation": ("fold", "letters", "duplex"),
    "hairpin_length_at_least_k shifted by one": ("fold", "shapes", "hairpin"),
    "bulge_length <-> internal_length": ("fold", "shapes", "letters"),
    "internal_symmetric_length shifted by one": ("fold", "shapes", "letters"),
    "internal_asymmetry shifted by one": ("fold", "shapes", "letters"),
    "internal_explicit_1_4 <-> internal_explicit_2_3": ("fold", "shapes", "letters"),
    "multi_base <-> multi_paired": ("fold", "multiloop"),
}
