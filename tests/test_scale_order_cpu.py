"""CPU suite: the order in which the scale-exponent ladders try their exponents (ractip_amd/csrc/scale_order.h: the start model,
then the larger exponents ascending, then the smaller ones descending), through the stand-alone program
tools/exponent_order_check.cpp.  Model -1 is the default exponent, k is rung k."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the exponents as the library sets them: rh_create (0.12, 0.28), kRungS (fallbacks.hip), kVRungS (launch_vienna.hip)
CONTRAFOLD = ("0.12", "0.45", "1.5", "0")
VIENNA_BL = ("0.28", "0.7", "1.8", "0")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "exponent_order_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ractip_amd", "csrc"),
                           os.path.join(ROOT, "tools", "exponent_order_check.cpp"), "-o", path])
    return path


def orders(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        start, models = line.split(":")
        out[int(start)] = [int(m) for m in models.split()]
    return out


def test_contrafold_ladder_after_a_pass_on_each_model(exe):
    """retry_mc_lin_rungs: 0.45 and 1.5 for what overflowed, 0 for what vanished; from a remembered rung the default is one of them"""
    assert orders(exe, "retry", *CONTRAFOLD) == {-1: [0, 1, 2], 0: [1, -1, 2], 1: [0, -1, 2], 2: [-1, 0, 1]}


def test_vienna_bl_attempts_start_with_the_start_model(exe):
    """compute: the whole batch on the start model, then on the others in the same order"""
    assert orders(exe, "attempts", *VIENNA_BL) == {-1: [-1, 0, 1, 2], 0: [0, 1, -1, 2], 1: [1, 0, -1, 2], 2: [2, -1, 0, 1]}


def test_the_constants_are_the_librarys():
    """the tables above against the source: a changed rung has to change the expectation"""
    def text(name):
        with open(os.path.join(ROOT, "ractip_amd", "csrc", name)) as f:
            return f.read()
    assert "kRungS[rh_ctx::kRungs] = {0.45, 1.5, 0.0}" in text("fallbacks.hip")
    assert "kVRungS[Ctx::kVRungs] = {0.7, 1.8, 0.0}" in text("launch_vienna.hip")
    assert "build_lin_model(host_model, 0.12, &c->lin0.h)" in text("rh_api.hip")
    assert "build_vlin_model(*host_vienna, 0.28, v0.h)" in text("rh_api.hip")
