"""CPU suite: the fused, pair-indexed weight tables of dxl_strip8 (DxLinModel::F, ractip_amd/csrc/lin_model.h, built on the host by
build_dx_lin_model) through the stand-alone program tools/dx_fused_check.cpp: every fused entry, looked up the way the kernel looks
it up, has the bits of the product evaluated from the plain tables in the order dx_cell_weights writes it -- for the shipped
CONTRAfold parameters and for synthetic tables whose entries are all distinct, at the scale exponents the library uses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "ractip_amd", "data", "contrafold_complementary.params")
# 6 pair types x 5^4 neighbour letters x 2 directions x 7 weights
COMPARED = 6 * 625 * 2 * 7


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "dx_fused_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ractip_amd", "csrc"),
                           os.path.join(ROOT, "tools", "dx_fused_check.cpp"), os.path.join(ROOT, "ractip_amd", "csrc", "param_loader.cpp"),
                           "-o", path])
    return path


def summary(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    words = r.stdout.split()
    return {words[k]: int(words[k + 1]) for k in (0, 2, 4, 6, 8)}


@pytest.mark.parametrize("source", [PARAMS, "synthetic"], ids=["shipped", "synthetic"])
@pytest.mark.parametrize("s", ["0.65", "1.6", "0"])
def test_every_fused_entry_has_the_bits_of_the_plain_product(exe, source, s):
    """all 150 entries of both directions are reached as own entry and as decorating entry; no weight differs in a bit"""
    d = summary(exe, source, s)
    assert d["types"] == 6 and d["compared"] == COMPARED and d["differ"] == 0 and d["unreached"] == 0, d


def test_synthetic_tables_do_not_hide_a_transposed_index(exe):
    """Under the synthetic scores few fused doubles are equal, and those by construction: e_b01 / e_b10 depend on one letter (5 values
    each), e_11 on two (25), and the decorating weight of one direction is the own weight of the other (2 x 150); e_ends and e_st
    are distinct per entry and direction (4 x 150): at most 935 distinct doubles of 2100, against some 540 for the shipped parameters,
    many of which are exp(0).  At least 850 says that the synthetic run compares distinct numbers in every one of these classes."""
    d = summary(exe, "synthetic")
    assert 850 <= d["distinct"] <= 935, d


def test_the_scale_exponents_are_the_librarys():
    def text(name):
        with open(os.path.join(ROOT, "ractip_amd", "csrc", name)) as f:
            return f.read()
    assert "build_dx_lin_model(host_model, 0.65, &c->h_dxlin)" in text("rh_api.hip")
