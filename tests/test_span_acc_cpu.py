"""CPU suite of region accessibility on span folds (rh_span_fold_acc):
  * the checker of the GPU tests without a GPU: up[i][w], widths 1..8, of the Vienna-BL oracle under the band mask against the
    brute-force enumeration under the same mask; what the entries past the end hold and that a row never grows with the width; the
    insert identity the length test rests on, for widths 1..15;
  * the sizes of the accessibility stage (span_acc_check in ractip_amd/csrc/span_fold.cpp) through the stand-alone program
    tools/span_fold_check.cpp built with the host sanitizers: n = 10^6 at L = 1000 and max_w = 64 as size_t, and every max_w
    rejection with its text."""
import os
import subprocess

import numpy as np
import pytest

import _span_acc_cases as ac
import _span_cases as sc
from _oracle import assert_prob_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")
RH_ERR_ARG = -1


# ---- the checker itself
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("L", [4, 5, 7, 9, 13])
def test_masked_dp_against_masked_enumeration_widths_1_to_8(seed, L):
    seq = sc.random_seq(13, seed=seed, plant_n=False)
    dp, bf = ac.masked_acc(seq, L, 8), ac.masked_acc(seq, L, 8, bruteforce=True)
    assert dp["up"].shape == (13, 8)
    assert np.abs(dp["up"] - bf["up"]).max() <= 1e-13
    assert np.abs(dp["band"] - bf["band"]).max() <= 1e-13
    assert (dp["up"][:, 0] == sc.masked(seq, L)["up"][:, 0]).all()   # the width-1 column does not depend on how many are asked for


@pytest.mark.parametrize("L", [6, 14])
def test_runs_past_the_end_hold_zero_and_rows_do_not_grow(L):
    seq = "GGCGCCGAAGGCGC"
    up = ac.masked_acc(seq, L, 14)["up"]
    i, w = np.arange(14)[:, None], np.arange(14)[None, :]
    assert not up[i + w >= 14].any() and (up[i + w < 14] > 0.0).all()
    assert (np.diff(up, axis=1) <= 1e-15).all()
    assert np.abs(up - ac.masked_acc(seq, L, 14, bruteforce=True)["up"]).max() <= 1e-13


def test_the_insert_identity_for_widths_1_to_15():
    """n = 206, L = 45: on the inserts up[., 0..14] is that of the unmasked oracle on "A" + insert + "A", a run that leaves the insert
    equals the run cut at its last letter, and a run inside a spacer holds 1"""
    L, m, ins = 45, 40, sc.inserts(2, 40, distinct=2)
    seq, starts = sc.long_sequence(206, L, ins, lead=19)
    up = ac.masked_acc(seq, L, 15)["up"]
    spacer = np.ones(206, dtype=bool)
    for s, at in zip(ins, starts):
        assert_prob_close(up[at:at + m], ac.insert_acc_reference(s, 15), rel=1e-9, what="up on an insert")
        spacer[at:at + m] = False
    free = np.array([[i + w < 206 and spacer[i:i + w + 1].all() for w in range(15)] for i in range(206)])
    assert free.sum() > 500 and np.abs(up[free] - 1.0).max() <= 1e-12


# ---- the sizes of the stage
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "span_fold_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "span_fold_check.cpp"), os.path.join(CSRC, "span_fold.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


@pytest.mark.parametrize("max_w", [0, -1, 65, 1000, -2 ** 31, 2 ** 31 - 1])
def test_every_max_w_rejection_with_its_text(exe, max_w):
    assert run(exe, "acc", 40, 5, max_w) == "err %d span fold: max_w %d (must be 1..64)\n" % (RH_ERR_ARG, max_w)


def test_the_checks_of_the_fold_come_first(exe):
    assert run(exe, "acc", 40, 1, 0) == "err %d span fold: max_span 1 (must be >= 2)\n" % RH_ERR_ARG
    assert run(exe, "acc", 0, 5, 5) == "err %d span fold: the sequence has length 0 (must be >= 1)\n" % RH_ERR_ARG


@pytest.mark.parametrize("n,L,max_w", [(40, 5, 1), (40, 5, 2), (47, 20, 15), (1, 2, 5), (257, 20, 64), (20000, 70, 15)])
def test_the_sizes(exe, n, L, max_w):
    got = [int(x) for x in run(exe, "acc", n, L, max_w).split()[1:]]
    ldn = -(-(n + 1) // 16) * 16
    assert got == [n, L, max_w, n * max_w, 64 * ldn if max_w > 1 else 0]


def test_the_sizes_of_a_million_letters_are_size_t(exe):
    got = [int(x) for x in run(exe, "acc", 10 ** 6, 1000, 64).split()[1:]]
    assert got == [10 ** 6, 1000, 64, 64 * 10 ** 6, 64 * 1000016]
    big = [int(x) for x in run(exe, "acc", 2 ** 31 - 64, 2, 64).split()[1:]]
    assert big[3] == 64 * (2 ** 31 - 64) > 2 ** 32   # the doubles of up alone do not fit 32 bits


def test_the_plan_output_is_what_it_was(exe):
    assert run(exe, "plan", 20000, 70) == "ok 20000 70 70 20016 1401120 18214560 1400000 40002\n"
