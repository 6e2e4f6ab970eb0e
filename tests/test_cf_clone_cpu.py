"""CPU suite: the clone-parameter oracle of the CONTRAfold model's region accessibility (tests/_cf_clone.py) against the pinned
oracle's own posterior.  No GPU: this checks the yardstick the GPU suite (test_gpu_cf_accessibility.py) compares with."""
import math
import re

import numpy as np
import pytest

from _cf_clone import FAMILIES, CloneOracle, clone_params, random_seq, read_params, region_up

LENGTHS = (12, 33, 70)


@pytest.fixture(scope="module")
def clones(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cf_clone")
    return {name: CloneOracle(name, tmp) for name in FAMILIES}


def sequence(fam, n):
    """{A,U} and {C,G}: random; {A,U,G}: random with a run of A (the recodable letters) planted in the middle"""
    rng = np.random.default_rng(40 + n + len(fam))
    s = random_seq(rng, n, FAMILIES[fam].alphabet)
    if fam == "AUG":
        run = min(16, n // 2)
        s = s[:n // 4] + "A" * run + s[n // 4 + run:]
    return s


def recodable(co, seq):
    return [i for i, c in enumerate(seq) if c in co.family.recode]


def test_clone_files_keep_every_name_and_change_only_letter_suffixed_values():
    rows = read_params()
    assert len(rows) == 708
    for fam in FAMILIES.values():
        clone = clone_params(fam, rows)
        assert [n for n, _ in clone] == [n for n, _ in rows]
        for (name, v), (_, c) in zip(rows, clone):
            if not re.search(r"_[ACGU]+$", name):
                assert v == c, name
        assert all(dict(clone)[d] == -1e4 for d in fam.disabled)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("n", LENGTHS)
def test_logz_of_in_alphabet_sequences_is_the_same_under_both_files(clones, fam, n):
    co = clones[fam]
    seq = sequence(fam, n)
    assert co.logz_clone(seq) == co.logz(seq)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("n", LENGTHS)
def test_width_one_is_one_minus_the_posterior_row_sums(clones, fam, n):
    co = clones[fam]
    seq = sequence(fam, n)
    want = co.unpaired1(seq)
    for i in recodable(co, seq):
        assert abs(region_up(co, seq, i, 0) - want[i]) <= 1e-9, (fam, n, i)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("n", LENGTHS)
def test_wider_regions_are_not_more_accessible(clones, fam, n):
    co = clones[fam]
    seq = sequence(fam, n)
    ok = set(recodable(co, seq))
    for i in sorted(ok)[::3]:
        prev = math.inf
        for w in range(15):
            if i + w >= n or i + w not in ok:
                break
            cur = region_up(co, seq, i, w)
            assert cur <= prev * (1 + 1e-12), (fam, n, i, w)
            prev = cur
