"""CPU suite: the window arithmetic of local folding (ractip_amd/csrc/local_windows.{h,cpp}) through the stand-alone program
tools/local_windows_check.cpp built with the host sanitizers: the starts and the window count against the definition restated
here, every rejection with its code and exact text, the windows that contain a run against a brute-force loop over the starts,
the band sizes of a sequence of a million letters as size_t, and the chunks of the tile walk when there is no second molecule."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")
RH_ERR_ARG = -1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "local_windows_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "local_windows_check.cpp"), os.path.join(CSRC, "local_windows.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def starts_restated(n, W, S):
    """the definition of the issue: one window if n <= W, else the grid 0, S, .. below n - W and a last window at n - W"""
    if n <= W:
        return [0]
    m = -(-(n - W) // S)
    return [k * S for k in range(m)] + [n - W]


def plan(exe, n, W, S):
    words = run(exe, "plan", n, W, S).split()
    assert words[0] == "ok" and words[4] == ":", words
    return dict(We=int(words[1]), nw=int(words[2]), ld=int(words[3]), starts=[int(x) for x in words[5:]])


# n < W, n = W, n = W + 1, (n - W) a multiple of S, not a multiple, S = W, S = 1, and the shapes of tests/test_gpu_local_fold.py
PLANS = [(9, 16, 1), (16, 16, 1), (17, 16, 1), (17, 16, 16), (46, 16, 5), (43, 16, 5), (48, 16, 16), (50, 16, 16), (41, 16, 1), (70, 65, 1),
         (40, 33, 2), (230, 200, 7), (52, 16, 9), (2, 2, 1), (3, 2, 2), (1, 2, 1), (60, 2, 1), (60, 59, 59)]


@pytest.mark.parametrize("n,W,S", PLANS)
def test_starts_and_window_count(exe, n, W, S):
    p = plan(exe, n, W, S)
    want = starts_restated(n, W, S)
    assert p["starts"] == want and p["nw"] == len(want)
    assert p["We"] == min(W, n) and p["ld"] == p["We"]
    assert want[0] == 0 and want[-1] + p["We"] == n                      # the first window starts, the last one ends the sequence
    assert all(a < b for a, b in zip(want, want[1:]))                    # distinct and increasing
    assert all(b - a <= S for a, b in zip(want, want[1:]))               # no letter between two windows


def test_the_named_cases():
    assert starts_restated(43, 16, 5) == [0, 5, 10, 15, 20, 25, 27]      # the final start is off the grid
    assert starts_restated(46, 16, 5) == [0, 5, 10, 15, 20, 25, 30]      # (n - W) a multiple of S: the last start is on it
    assert starts_restated(48, 16, 16) == [0, 16, 32] and starts_restated(50, 16, 16) == [0, 16, 32, 34]
    assert starts_restated(17, 16, 1) == [0, 1] and starts_restated(16, 16, 1) == [0] and starts_restated(9, 16, 1) == [0]


@pytest.mark.parametrize("args,text", [
    ((10, 1, 1), "local fold: window 1 (must be >= 2)"),
    ((10, 0, 1), "local fold: window 0 (must be >= 2)"),
    ((10, 4, 0), "local fold: step 0 (must be >= 1)"),
    ((10, 4, -3), "local fold: step -3 (must be >= 1)"),
    ((10, 4, 5), "local fold: step 5 exceeds the window 4"),
    ((0, 4, 1), "local fold: the sequence has length 0 (must be >= 1)"),
    ((-2, 4, 1), "local fold: the sequence has length -2 (must be >= 1)"),
    ((10, 4, 1, "null"), "local fold: the sequence is NULL"),
])
def test_every_rejection_with_its_text(exe, args, text):
    assert run(exe, "plan", *args) == "err %d %s\n" % (RH_ERR_ARG, text)


RANGES = [(n, W, S) for n in (1, 2, 7, 16, 17, 33, 60) for W in (2, 5, 16, 60, 64) for S in (1, 2, 3, 5, 16) if S <= W]


def test_containing_windows_against_brute_force(exe):
    """for every run (i, len), runs past the end included: the windows lo..hi are exactly the windows whose letters hold the run"""
    seen = 0
    for n, W, S in RANGES:
        starts, We = starts_restated(n, W, S), min(W, n)
        lines = run(exe, "ranges", n, W, S).splitlines()
        assert len(lines) == sum(n - i + 1 for i in range(n))
        for line in lines:
            i, ln, lo, hi = (int(x) for x in line.split())
            brute = [k for k, s in enumerate(starts) if s <= i and i + ln - 1 <= s + We - 1 and i + ln <= n]
            got = list(range(lo, hi + 1))
            assert got == brute, (n, W, S, i, ln, lo, hi, brute)
            seen += 1
    assert seen > 20000


def test_uncovered_runs_exist_only_with_a_step_above_one(exe):
    """S > 1: a run longer than We - S + 1 letters may lie in no window; S = 1: every run of at most We letters lies in one"""
    for n, W, S in [(50, 16, 16), (52, 16, 9), (41, 16, 1)]:
        We = min(W, n)
        uncovered = []
        for line in run(exe, "ranges", n, W, S).splitlines():
            i, ln, lo, hi = (int(x) for x in line.split())
            if ln <= We and i + ln <= n and lo > hi:
                uncovered.append(ln)
        if S == 1:
            assert not uncovered
        else:
            assert uncovered and min(uncovered) > We - S + 1


@pytest.mark.parametrize("n,W,S,chunk", [(41, 16, 1, 8), (41, 16, 1, 7), (43, 16, 5, 3), (43, 16, 5, 1), (43, 16, 5, 7), (43, 16, 5, 100), (9, 16, 1, 4)])
def test_the_chunks_of_a_walk_without_a_second_molecule(exe, n, W, S, chunk):
    """local_tile_at with P2.nw = 0: the chunks of rh_local_fold, first and last, with a ragged last one, one chunk, one window"""
    nw = len(starts_restated(n, W, S))
    chunk = min(chunk, nw)
    want = [(k0, min(nw, k0 + chunk), 0, 0) for k0 in range(0, nw, chunk)]
    got = [tuple(int(x) for x in line.split()) for line in run(exe, "chunks", n, W, S, chunk).splitlines()]
    assert got == want and got[0][0] == 0 and got[-1][1] == nw


def test_band_sizes_of_a_million_letters_are_size_t(exe):
    assert run(exe, "sizes", 10 ** 6, 1000, 1, 15) == "band %d up %d\n" % (10 ** 9, 15 * 10 ** 6)
    assert 8 * 10 ** 9 > 2 ** 32                                          # bytes of that band: past 32 bits
    p = plan(exe, 10 ** 6, 1000, 250)
    assert p["nw"] == (10 ** 6 - 1000) // 250 + 1 and p["starts"][-1] == 10 ** 6 - 1000
