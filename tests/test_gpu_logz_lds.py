"""dxl_logz_part (duplex_lin.hip) reads the letters of the pair and the weights E_dl / E_dr / E_hc from LDS; only the table value of an
item comes from global memory.  The item list, the per-thread order of the sums and the reductions are what they were, so log Z and
hp keep their oracle parity and stay bit-equal between a pair alone and in a batch, and between two computes on one context."""
import numpy as np
import pytest

from _oracle import NEG, assert_log_close, assert_prob_close

pytestmark = pytest.mark.gpu

REL = 1e-6   # tests/test_gpu_parity.py


def rnd(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), n))


def cases():
    rng = np.random.RandomState(733)
    with_n = list(rnd(rng, 90))
    for k in (0, 17, 44, 89):
        with_n[k] = "N"              # letter code 4
    return [
        (rnd(rng, 5), rnd(rng, 300)),
        (rnd(rng, 260), rnd(rng, 300)),          # rows longer than 256 cells: two items per row and thread
        (rnd(rng, 33), rnd(rng, 17)),            # 49 anti-diagonals: the last chunk holds one row
        (rnd(rng, 21, "AC"), rnd(rng, 30, "AC")),   # no complementary letters at all
        ("".join(with_n), "N" + rnd(rng, 70) + "N"),
    ]


@pytest.fixture(scope="module")
def computed(hotlib):
    import ractip_amd
    pairs = cases()
    c = ractip_amd.Context(device=0)
    c.batch_upload(pairs)
    c.batch_compute()
    assert c.last_path() == 1   # the scaled linear kernels
    res = [c.batch_results(p) for p in range(len(pairs))]
    yield c, pairs, res
    c.close()


def test_logz_and_hp_against_the_oracle(computed, oracle):
    _, pairs, res = computed
    for (s1, s2), r in zip(pairs, res):
        od = oracle.duplex(s1, s2)
        what = "pair (%d,%d)" % (len(s1), len(s2))
        assert_log_close([r["logZ"][2]], [od["logZ2"][0]], tol=1e-9, what=what)
        assert_prob_close(r["hp"], od["post"], rel=REL, what="hp " + what)
    z, hp = res[3]["logZ"][2], res[3]["hp"]
    assert z < NEG / 2 and hp.max() == 0.0   # the reference's sentinel: no complementary pair


def test_alone_equals_batch_and_recompute_bit_for_bit(computed):
    c, pairs, res = computed
    import ractip_amd
    c.batch_compute()   # a second compute on the same context
    for p, r0 in enumerate(res):
        r = c.batch_results(p)
        assert np.array_equal(r["hp"], r0["hp"]) and r["logZ"][2] == r0["logZ"][2], p
    a = ractip_amd.Context(device=0)
    try:
        for (s1, s2), r0 in zip(pairs, res):
            hp, z = a.duplex(s1, s2)
            assert np.array_equal(hp, r0["hp"]) and z == r0["logZ"][2], (len(s1), len(s2))
    finally:
        a.close()
