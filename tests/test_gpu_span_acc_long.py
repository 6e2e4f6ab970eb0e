"""GPU suite: region accessibility on a span fold at length.  n = 20000, L = 70, max_w = 15 on the factorising sequence of
tests/test_gpu_span_fold_long.py: 90 inserts of 60 random G/C letters (six distinct, cycling), each followed by 69 A's, at the front
of a poly-A sequence (pinned on the oracle for widths 1..15 by tests/test_span_acc_cpu.py::test_the_insert_identity_for_widths_1_to_15).
  * A run inside an insert equals the UNMASKED oracle on "A" + insert + "A" (rel 1e-6 above 1e-12).
  * A run that starts in an insert and ends in the spacer behind it equals the reference run cut at the insert's last letter.
  * A run inside a spacer or the poly-A tail equals 1 within 1e-9: such an entry is the exponential of the sum of three exterior
    logarithms at log Z ~ 4298, each of which the span fold's own length test holds to the same bound.
  * A run that passes the last letter holds 0."""
import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot
import _span_acc_cases as ac
import _span_cases as sc
from _oracle import assert_prob_close

pytestmark = pytest.mark.gpu

N, L, COUNT, M, W = 20000, 70, 90, 60, 15


def test_twenty_thousand_letters_at_fifteen_widths(hotlib):
    ins = sc.inserts(COUNT, M)
    seq, starts = sc.long_sequence(N, L, ins)
    refs = {s: ac.insert_acc_reference(s, W) for s in set(ins)}
    total = sum(sc.insert_reference(s)[0] for s in ins)
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    try:
        band, up, logz = c.span_fold(seq, L, W)
        ms = c.span_acc_times()
    finally:
        c.close()
    assert band.shape == (N, L) and up.shape == (N, W) and all(x > 0.0 for x in ms)
    assert abs(logz - total) <= 1e-9 * COUNT, (logz, total)
    insert = np.zeros(N + W, dtype=bool)
    for s, at in zip(ins, starts):
        assert_prob_close(up[at:at + M], refs[s], what="up on the insert at %d, runs into the spacer included" % at)
        insert[at:at + M] = True
    reach = np.lib.stride_tricks.sliding_window_view(insert, W)[:N]          # reach[i, w]: letter i + w lies on an insert
    free = ~np.logical_or.accumulate(reach, axis=1)                           # the run i .. i + w touches none
    i, w = np.arange(N)[:, None], np.arange(W)[None, :]
    fits = i + w < N
    assert (free & fits).sum() > N * W // 2
    assert np.abs(up[free & fits] - 1.0).max() <= 1e-9
    assert not up[~fits].any()
    # what is left: runs that start in a spacer and reach the next insert -- exterior in front, then the insert's own letters
    for k in (1, 7, COUNT - 1):
        at, ref = starts[k], refs[ins[k]]
        for back in (1, 5, W - 1):                                            # the run starts `back` letters in front of the insert
            got = up[at - back, back:]
            assert_prob_close(got, ref[0, :W - back], what="a run from the spacer into the insert at %d" % at)
