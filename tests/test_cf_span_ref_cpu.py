"""Pins tests/_cf_span_ref.py, the numpy checker of span folds under the CONTRAfold model, to the pinned oracle (oracle/cf_oracle.c)
in three independent ways, without a GPU:

1. no mask: log Z and the posterior of the oracle itself, under the bundled weights and under the scrambled file (no zero rows, no
   accidental symmetries: a mixed-up index or tying rule shows);
2. region masks: "no letter of i..i+w pairs" against the clone oracle (tests/_cf_clone.py), which forbids a region by recoding its
   letters -- this pins the mask mechanism itself;
3. band masks where the unmasked oracle knows the answer: at L = n - 1 only the pair (1, n) is excluded, at L = n - 2 three mutually
   exclusive pairs are, so log Z moves by log(1 - their probability); L >= n is no mask at all.
"""
import math

import numpy as np
import pytest

import _cf_span_ref as ref
import _contrafold_weights as cw
from _cf_clone import CloneOracle
from _oracle import Oracle, tri_offset
from _span_cases import random_seq

END_PAIR = "GGGCGCGG" + random_seq(54, seed=3, plant_n=False) + "CCGCGCCC"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return {"bundled": None, "scrambled": cw.write(tmp_path_factory.mktemp("cfref") / "scrambled.params", cw.scrambled())}


@pytest.mark.parametrize("which", ["bundled", "scrambled"])
def test_no_mask_is_the_oracle(files, which):
    o = Oracle(files[which])
    for n in range(1, 81):
        seq = random_seq(n, seed=11)
        want, got = o.inference(seq), ref.inference(seq, None, files[which])
        assert abs(got["logZ"] - want["logZ"]) <= 1e-9, (which, n)
        big = want["post"] > 1e-12
        if big.any():
            rel = np.abs(got["post"][big] - want["post"][big]) / want["post"][big]
            assert rel.max() <= 1e-9, (which, n, rel.max())
        assert np.abs(got["post"][~big] - want["post"][~big]).max() <= 1e-12, (which, n)


@pytest.mark.parametrize("family", ["AU", "CG"])
def test_region_masks_against_the_clone_oracle(tmp_path, family):
    co = CloneOracle(family, tmp_path)
    rs = np.random.RandomState(5)
    for n, regions in ((30, ((0, 0), (4, 2), (11, 7), (29, 0))), (47, ((20, 5), (0, 9), (40, 6)))):
        seq = "".join(rs.choice(list(co.family.alphabet), n))
        for i, w in regions:
            lo, hi = i + 1, i + 1 + w   # the region in 1-based letters
            free = lambda a, b: ~(((a >= lo) & (a <= hi)) | ((b >= lo) & (b <= hi)))
            got = ref.inference(seq, free)["logZ"]
            assert abs(got - co.logz_clone(co.recoded(seq, i, w))) <= 1e-9, (family, n, i, w)
        assert abs(ref.inference(seq)["logZ"] - co.logz(seq)) <= 1e-9


def test_band_masks_where_the_unmasked_oracle_knows_the_answer():
    n = len(END_PAIR)
    r = Oracle().inference(END_PAIR)
    P = lambda a, b: r["post"][tri_offset(n, a) + b]
    assert abs(r["logZ"] - 12.7128) < 1e-3 and P(1, n) > 0.9, "the end pair dominates: the cut moves log Z by more than two nats"
    one = ref.span_ref(END_PAIR, n - 1)
    assert abs(one["logZ"] - (r["logZ"] + math.log1p(-P(1, n)))) <= 1e-9
    three = ref.span_ref(END_PAIR, n - 2)
    assert abs(three["logZ"] - (r["logZ"] + math.log1p(-(P(1, n) + P(1, n - 1) + P(2, n))))) <= 1e-9
    assert r["logZ"] - one["logZ"] > 2.0
    free = ref.inference(END_PAIR)
    for L in (n, n + 1, 500):
        got = ref.span_ref(END_PAIR, L)
        assert got["logZ"] == free["logZ"] and np.array_equal(got["post"], free["post"]), L
    assert one["band"].shape == (n, n - 1) and one["up"].shape == (n, 1)
    # up is 1 - the row sums of the posterior
    full = ref.span_ref(END_PAIR, n)
    M = np.zeros((n + 1, n + 1))
    for a in range(1, n):
        M[a, a + 1:] = full["post"][tri_offset(n, a) + a + 1:tri_offset(n, a) + n + 1]
    np.testing.assert_allclose(full["up"][:, 0], np.maximum(0.0, 1.0 - (M + M.T).sum(1)[1:]), rtol=0, atol=1e-14)


def test_no_pair_within_the_band_leaves_the_unpaired_chain():
    seq = random_seq(40)
    for L in (2, 4):
        r = ref.span_ref(seq, L)
        assert not r["band"].any() and (r["up"] == 1.0).all()
        assert abs(r["logZ"] - 40 * r["eu"]) <= 1e-12
