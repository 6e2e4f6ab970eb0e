"""CPU suite: the layout of the packed float image (packed_layout, ractip_amd/csrc/batch.h) through the stand-alone program
tools/packed_layout_check.cpp built with the host sanitizers: its own checks over ragged batches, 512 and 2048 pairs of 2000 + 2000 (no
overlap, offsets multiples of 4, tight block sizes, exact totals beyond 2^32, at most half the bytes of the padded double tables), and
the offsets of a few batches against the formulas restated here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "packed_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "packed_layout_check.cpp"), "-o", path])
    return path


def test_the_layout_holds_its_properties(exe):
    r = subprocess.run([exe, "self"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1:] == ["failures 0"], (r.stdout[-4000:], r.stderr[-4000:])


def pad4(x):
    return (x + 3) // 4 * 4


def restated(lens, pairs, max_w):
    """bp_off, up_off, hp_off, totals: every block at the next multiple of 4 elements behind the one before it"""
    bp, up, hp = [0], [0], [0]
    for n in lens:
        bp.append(bp[-1] + pad4((n + 1) * (n + 2) // 2))
        up.append(up[-1] + pad4(n * max_w))
    for a, b in pairs:
        hp.append(hp[-1] + pad4((lens[a] + 1) * (lens[b] + 1)))
    return bp, up, hp, [bp[-1], up[-1], hp[-1]]


CASES = [
    # the ragged batch of tests/test_gpu_packed_f32.py: T(1) = 3, T(2) = 6, T(5) = 21 are no multiples of 4
    ([1, 1, 2, 3, 5, 4, 7, 64, 65, 31, 113, 53, 130, 1], [(2 * p, 2 * p + 1) for p in range(7)], 1),
    ([1, 17, 40, 64, 9, 30], [(0, 1), (2, 3), (4, 5)], 64),
    ([12, 9, 12, 40], [(0, 1), (1, 0), (2, 2), (0, 2), (1, 1)], 15),   # indexed: sequence 3 in no pair, 1 in both roles
    ([2000] * 1024, [(2 * p, 2 * p + 1) for p in range(512)], 15),
]


@pytest.mark.parametrize("lens,pairs,max_w", CASES, ids=["ragged", "wide", "indexed", "512x2000"])
def test_offsets_equal_the_restated_formulas(exe, lens, pairs, max_w):
    args = [str(max_w), str(len(lens))] + [str(n) for n in lens] + [str(len(pairs))] + [str(x) for p in pairs for x in p]
    r = subprocess.run([exe, "offsets"] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    got = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert got == [list(v) for v in restated(lens, pairs, max_w)]
    if len(pairs) == 512:
        assert got[3][2] == 512 * pad4(2001 * 2001) == 2050050048 and 4 * got[3][2] > 2 ** 32   # (past 32-bit byte offsets)
