"""GPU suite: span-limited folding at length.  n = 20000, L = 70: 90 inserts of 60 random G/C letters (six distinct, cycling), each
followed by 69 A's, at the front of a poly-A sequence.  A pairs with neither G, C nor A and the spacers are L - 1 long, so the
ensemble factorises (pinned on the oracle by tests/test_span_fold_cpu.py::test_the_insert_identity): band and up on an insert are
those of the UNMASKED oracle on "A" + insert + "A", log Z is the sum over the inserts -- more than 3 x 745 nats, all of it in the
first 60 % of the letters, which no single scale exponent keeps inside the double range.  The tolerance on log Z is 1e-9 x the
number of inserts (the reference is a sum of that many oracle values), everything between the inserts is exactly 0.  With only 30
A's between the first two inserts they must NOT factorise: that stretch is compared with the masked oracle on it."""
import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot
import _span_cases as sc
from _oracle import assert_prob_close

pytestmark = pytest.mark.gpu

N, L, COUNT, M = 20000, 70, 90, 60


@pytest.fixture(scope="module")
def v1(hotlib):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    yield c
    c.close()


def test_twenty_thousand_letters_factorise(v1):
    ins = sc.inserts(COUNT, M)
    seq, starts = sc.long_sequence(N, L, ins)
    refs = {s: sc.insert_reference(s) for s in set(ins)}
    total = sum(refs[s][0] for s in ins)
    assert len(set(ins)) == 6 and total > 3 * 745.0
    band, up, logz = v1.span_fold(seq, L)
    assert band.shape == (N, L) and up.shape == (N, 1)
    assert abs(logz - total) <= 1e-9 * COUNT, (logz, total)
    covered = np.zeros(N, dtype=bool)
    for s, at in zip(ins, starts):
        _, rb, ru = refs[s]
        assert_prob_close(band[at:at + M, :M], rb, what="band on the insert at %d" % at)
        assert_prob_close(up[at:at + M, 0], ru, what="up on the insert at %d" % at)
        assert not band[at:at + M, M:].any()
        covered[at:at + M] = True
    assert not band[~covered].any() and (up[~covered] == 1.0).all()


def test_near_inserts_do_not_factorise(v1):
    ins = sc.inserts(COUNT, M)
    seq, starts = sc.long_sequence(N, L, ins, gaps={0: 30})
    assert starts[1] - starts[0] == M + 30
    stretch = seq[:starts[1] + M + 1]                      # "A" + insert + 30 A + insert + "A": 1 + 60 + 30 + 60 + 1 letters
    ref = sc.masked(stretch, L)
    apart = sc.insert_reference(ins[0])[0] + sc.insert_reference(ins[1])[0]
    assert abs(ref["logZ"] - apart) > 1e-6                 # the neighbours see each other
    band, up, logz = v1.span_fold(seq, L)
    k = len(stretch) - 1                                   # the last A of the stretch is followed by A's as in the oracle's end
    assert_prob_close(band[:k], ref["band"][:k], what="band on the stretch")
    assert_prob_close(up[:k, 0], ref["up"][:k, 0], what="up on the stretch")
    rest = sum(sc.insert_reference(s)[0] for s in ins[2:])
    assert abs(logz - (ref["logZ"] + rest)) <= 1e-9 * COUNT
    first = sc.insert_reference(ins[0])[1]
    assert np.abs(band[1:1 + M, :M] - first).max() > 1e-6  # and the band on the first insert is not the lone insert's
