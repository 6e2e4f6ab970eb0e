"""CPU suite: the index maps of the exterior-sum passes (ractip_amd/csrc/f5_stage.h, used by lin_f5i_pass / lin_f5o_pass) through the
stand-alone program tools/f5_stage_check.cpp: both passes run on the CPU thread by thread in the kernels' order, over a synthetic FCA
table of distinct values, and every F5i / F5o entry has the bits of the serial recurrences under the same 256-way partition; every
term is delivered exactly once to the thread that owns it, no staged address leaves the sequence's own cells, no LDS slot is written
twice within a chunk, and the dynamic LDS stays within 64 KB at every ld that launched the pass kernels before they staged."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ractip_amd", "csrc", "f5_stage.h")
# every n in 32..600, 1025 and 2000 at their own ld; every fifth of them (2000 itself apart) at ld = 2002; 40 / 300 / 600 at ld = 4088
OWN = list(range(32, 601)) + [1025, 2000]
LENGTHS = len(OWN) + len([n for n in OWN[::5] if n < 2000]) + 3
# F5i entries 32..n and F5o entries 1..n-1 of every run
ENTRIES = sum((n - 31) + (n - 1) for n in OWN + [n for n in OWN[::5] if n < 2000] + [40, 300, 600])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "f5_stage_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ractip_amd", "csrc"), os.path.join(ROOT, "tools", "f5_stage_check.cpp"),
                           "-o", path])
    return path


def test_staged_passes_have_the_bits_of_the_serial_recurrences(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    words = r.stdout.split()
    d = {words[k]: int(words[k + 1]) for k in range(0, len(words), 2)}
    assert d["lengths"] == LENGTHS and d["entries"] == ENTRIES and d["terms"] > 0, d
    assert d["differ"] == 0 and d["misdelivered"] == 0 and d["stray"] == 0 and d["rewritten"] == 0 and d["lds"] == 0, d


def test_the_gpu_test_knows_the_chunk_rows():
    """tests/test_gpu_f5_staged.py places lengths around the chunk-row count; its constant is the header's"""
    from test_gpu_f5_staged import STAGE_ROWS
    with open(HEADER) as f:
        m = re.search(r"constexpr int kF5StageRows = (\d+);", f.read())
    assert m and int(m.group(1)) == STAGE_ROWS
