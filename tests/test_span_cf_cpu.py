"""CPU suite of what span folds under the CONTRAfold model add outside the kernels: the two ABI functions (header and the built
library's exports), the plans sized by the model's table count (thirteen band tables per item under Vienna-BL, eleven under
CONTRAfold: a batch is chunked by the bytes really used, and the Vienna-BL plans are what they were), and the exterior passes
(span_ext_pass_host, the kernel's host twin) on a table that carries the unpaired step's weight: with
FCA' = FC x stem weight x exp(external_paired - external_unpaired (d + 2)) from the restatement tests/_cf_span_ref.py they give the
restatement's log Z - n external_unpaired in both directions.  The host code runs in the stand-alone program tools/span_cf_check.cpp,
built with the host sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import _cf_span_ref as ref
import _contrafold_weights as cw
from _span_cases import random_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "span_cf_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "span_cf_check.cpp"), os.path.join(CSRC, "span_fold.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def plan(exe, model, L, max_w, budget, lens):
    out = dict(items=[], chunks=[])
    for line in run(exe, "plan", model, L, max_w, budget, *lens).splitlines():
        kind, rest = line.split()[0], [int(x) for x in line.split()[1:]]
        if kind == "ok":
            out["head"] = rest
        else:
            out[kind + "s"].append(rest)
    return out


def test_the_header_declares_and_the_library_exports_the_switch(hotlib):
    text = open(os.path.join(ROOT, "include", "ractip_hot.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+rh_set_span_contrafold\s*\(\s*rh_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", text)
    assert re.search(r"\bint\s+rh_get_span_contrafold\s*\(\s*const\s+rh_ctx\s*\*\s*ctx\s*\)\s*;", text)
    assert hasattr(hotlib, "rh_set_span_contrafold") and hasattr(hotlib, "rh_get_span_contrafold")
    import ractip_amd.hot as hot
    assert hasattr(hot.Context, "set_span_contrafold") and hasattr(hot.Context, "get_span_contrafold")


LENS = [257, 1, 300, 3, 13, 129, 64, 65]


@pytest.mark.parametrize("L,max_w", [(33, 1), (70, 15), (500, 1)])
def test_the_plans_are_sized_by_the_model(exe, L, max_w):
    plans = {m: plan(exe, m, L, max_w, 0, LENS) for m in ("default", "vienna", "contrafold")}
    assert plans["default"] == plans["vienna"], "the Vienna-BL plans are the call without a table count"
    for model, count in (("vienna", 13), ("contrafold", 11)):
        p = plans[model]
        assert p["head"] == [len(LENS), 1] and p["chunks"] == [[0, len(LENS), sum(it[5] for it in p["items"])]]
        for k, (n, it) in enumerate(zip(LENS, p["items"])):
            Le, ldn = min(n, L), -(-(n + 1) // 16) * 16
            gaps = 64 * ldn if max_w > 1 else 0
            assert it == [k, n, Le, ldn, Le * ldn, count * Le * ldn, n * Le, 2 * (n + 1), (count * Le * ldn + gaps) * 8]


def greedy(sizes, budget):
    chunks, used = [], 0
    for b in sizes:
        if chunks and used + b <= budget:
            chunks[-1] += 1
            used += b
        else:
            chunks.append(1)
            used = b
    return chunks


def test_chunking_under_a_budget_follows_the_bytes_of_the_model(exe):
    L = 33
    sizes = {m: [c * min(n, L) * (-(-(n + 1) // 16) * 16) * 8 for n in LENS] for m, c in (("vienna", 13), ("contrafold", 11))}
    budget = max(sizes["vienna"])          # the longest item under Vienna-BL: under CONTRAfold more items fit a chunk
    want = {m: greedy(sizes[m], budget) for m in sizes}
    assert want["vienna"] != want["contrafold"]
    for m in sizes:
        p = plan(exe, m, L, 1, budget, LENS)
        assert [c[1] for c in p["chunks"]] == want[m] and [c[0] for c in p["chunks"]] == [sum(want[m][:k]) for k in range(len(want[m]))]
        assert all(c[2] * 8 <= budget for c in p["chunks"])
        assert [len(plan(exe, m, L, 1, 1, LENS)["chunks"])] == [len(LENS)]


@pytest.mark.parametrize("which", ["bundled", "scrambled"])
@pytest.mark.parametrize("n,L", [(40, 4), (66, 70), (129, 40), (130, 65)])
def test_the_exterior_passes_on_the_folded_in_unpaired_weight(exe, tmp_path, which, n, L):
    params = None if which == "bundled" else cw.write(tmp_path / "scrambled.params", cw.scrambled())
    seq = random_seq(n)
    r = ref.span_ref(seq, L, params)
    Le, s, eu = min(L, n), 0.12, r["eu"]
    d = np.arange(Le)[:, None]
    # FCA~ of cell (i, d): the restatement's FC x stem weight x exp(external_paired), times exp(-eu (d + 2)), times lam^d
    table = np.ascontiguousarray(r["fca"][:Le, :n + 2] * np.exp(-eu * (d + 2)) * np.exp(-s * d))
    path = tmp_path / "fca.bin"
    table.tofile(str(path))
    gi_n, go_0 = (float(x) for x in run(exe, "ext", n, Le, s, path).split())
    assert abs(gi_n - (r["logZ"] - n * eu)) <= 1e-9 and abs(go_0 - (r["logZ"] - n * eu)) <= 1e-9
