"""CPU suite: the index maps of the packed operand tiles (ractip_amd/csrc/pk_layout.h, used by lin_pack_tiles and the block products
of mccaskill_far.hip) through the stand-alone program tools/pk_layout_check.cpp, built with the address and undefined-behaviour
sanitizers: both element -> index maps are bijections on 0..255, load half h of lane l addresses bytes 1024 h + 16 l .. + 15 of the
tile, register s of lane l is the element the MFMA operand needs in both layouts, LB of a tile is LA of its transpose, the pack
kernel's stores write every index once, a product formed from the fragments is the product of the tiles, and the pack kernel's fetch
map covers exactly the cells of a run of 0..8 tiles at the first and last run of every block diagonal at five row pitches."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 2 x 256 elements (bijections) + 256 pack threads + 128 loads + 256 product cells
CHECKS = 2 * 256 + 256 + 128 + 256


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "pk_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ractip_amd", "csrc"),
                           os.path.join(ROOT, "tools", "pk_layout_check.cpp"), "-o", path])
    return path


def test_fragment_order_of_the_packed_tiles(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    words = r.stdout.split()
    d = {words[k]: int(words[k + 1]) for k in range(0, len(words), 2)}
    assert d.pop("checks") == CHECKS and d.pop("runs") > 2000 and d.pop("run_cells") > 10 ** 6, r.stdout
    assert all(v == 0 for v in d.values()), d
