"""CPU suite of region accessibility on span folds under the CONTRAfold model: the yardstick of tests/test_gpu_span_cf_acc.py
(tests/_cf_span_acc_ref.py: two runs of the masked restatement) against what is already pinned, the floor of every GPU case's
references, and the plans sized with the stage's band tables (tools/span_cf_acc_check.cpp, built with the host sanitizers).

  - at L >= n the yardstick is the clone oracle's exp(logZ_clone - logZ) (tests/_cf_clone.py) on its families, to 1e-9;
  - at width 1 and L < n it is 1 - the row sums of span_ref's posterior, to 1e-9;
  both under the bundled and the scrambled weight file;
  - every reference of a GPU case lies above 1e-9 (assert_prob_close's absolute floor is 1e-12 against rel 1e-6: no entry is judged by
    the floor), and the planted multiloop's six trailing letters have the figures the GPU test names;
  - a CONTRAfold item at max_w > 1 takes (11 + extra) Le ldn + 64 ldn doubles, at max_w = 1 eleven tables, and a budget chunks a batch
    by those bytes."""
import math
import os
import subprocess

import numpy as np
import pytest

import _cf_clone as clone
import _cf_span_acc_ref as acc
import _cf_span_ref as ref
import _contrafold_weights as cw
from _cf_span_acc_cases import ALL_CASES, SCRAMBLED_CASES, case_entries, case_seq
from _oracle import Oracle
from _span_cases import random_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """weight file (None: the bundled one) and its rows, per name"""
    tmp = tmp_path_factory.mktemp("cfspanacc")
    rows = cw.scrambled()
    return tmp, {"bundled": (None, cw.read()), "scrambled": (cw.write(tmp / "scrambled.params", rows), rows)}


# ---- the yardstick against what is pinned
@pytest.mark.parametrize("which", ["bundled", "scrambled"])
@pytest.mark.parametrize("fam,n,extra", [("AU", 33, 0), ("CG", 33, 5), ("CG", 20, 0)])
def test_the_yardstick_at_full_span_is_the_clone_oracle(files, which, fam, n, extra):
    tmp, by_name = files
    params, rows = by_name[which]
    family = clone.FAMILIES[fam]
    o = Oracle(params)
    path = os.path.join(str(tmp), "clone_%s_%s.params" % (fam, which))
    with open(path, "w") as f:
        for name, v in clone.clone_params(family, rows):
            f.write("%s %r\n" % (name, v))
    cm = o.L.cfo_load_params(path.encode())
    assert cm
    z = lambda m, s: o.L.cfo_inference(m, s.encode(), len(s), None, None, None)
    seq = clone.random_seq(np.random.default_rng(1000 + n + 7 * len(fam)), n, family.alphabet)
    entries = acc.sampled(n, 15, 50, seed=n)
    got = acc.up_ref(seq, n + extra, entries, params)
    base = z(o.m, seq)
    for (i, w), g in zip(entries, got):
        recoded = seq[:i] + "".join(family.recode[c] for c in seq[i:i + w + 1]) + seq[i + w + 1:]
        want = math.exp(z(cm, recoded) - base)
        assert abs(g - want) <= 1e-9 * want, (i, w, g, want)


@pytest.mark.parametrize("which", ["bundled", "scrambled"])
@pytest.mark.parametrize("n,L", [(41, 20), (33, 12)])
def test_the_yardstick_at_width_one_is_one_minus_the_row_sums(files, which, n, L):
    params = files[1][which][0]
    seq = random_seq(n)
    want = ref.span_ref(seq, L, params)["up"][:, 0]
    got = acc.up_ref(seq, L, [(i, 0) for i in range(n)], params)
    assert np.abs(got - want).max() <= 1e-9


# ---- the GPU cases
@pytest.mark.parametrize("case", ALL_CASES, ids=str)
def test_the_references_of_a_gpu_case_lie_above_the_floor(case):
    want = acc.up_ref(case_seq(case), case[2], case_entries(case))
    print(case, len(want), "references, smallest %.3g" % want.min())
    assert want.min() > 1e-9 and want.max() <= 1.0 + 1e-12


@pytest.mark.parametrize("case", SCRAMBLED_CASES, ids=str)
def test_the_same_under_the_scrambled_weights(files, case):
    want = acc.up_ref(case_seq(case), case[2], case_entries(case), files[1]["scrambled"][0])
    print(case, len(want), "references, smallest %.3g" % want.min())
    assert want.min() > 1e-9


def test_the_trailing_run_of_the_planted_multiloop_across_the_band_edge():
    seq, trail = acc.planted_multiloop(3)
    run = {L: acc.up_ref(seq, L, [(trail[0], 5)])[0] for L in (86, 85, 84, 83, 40)}
    for L, want in ((86, 0.6976), (85, 0.6976), (84, 0.2934), (83, 0.2934), (40, 0.1472)):
        assert abs(run[L] - want) < 5e-5, (L, run[L])


# ---- the plans
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "span_cf_acc_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "span_cf_acc_check.cpp"), os.path.join(CSRC, "span_fold.cpp"), "-o", path])
    return path


def plan(exe, L, max_w, budget, lens):
    r = subprocess.run([exe, "plan"] + [str(a) for a in (L, max_w, budget) + tuple(lens)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = dict(items=[], chunks=[])
    for line in r.stdout.splitlines():
        kind, rest = line.split()[0], [int(x) for x in line.split()[1:]]
        if kind == "ok":
            out["head"] = rest
        else:
            out[kind + "s"].append(rest)
    return out


LENS = [257, 1, 300, 3, 13, 129, 64, 65]


def item_doubles(n, L, max_w, extra):
    Le, ldn = min(n, L), -(-(n + 1) // 16) * 16
    return ((11 + extra) * Le * ldn, 64 * ldn) if max_w > 1 else (11 * Le * ldn, 0)


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


@pytest.mark.parametrize("L,max_w", [(33, 1), (33, 2), (70, 15), (500, 64)])
def test_an_item_is_sized_with_the_tables_of_the_stage(exe, L, max_w):
    sweeps, extra = (int(x) for x in subprocess.run([exe, "tables"], capture_output=True, text=True, check=True).stdout.split())
    assert sweeps == 11 and extra >= 4, "hairpin sums, S and two A at the least"
    p = plan(exe, L, max_w, 0, LENS)
    assert p["head"] == [len(LENS), 1]
    for k, (n, it) in enumerate(zip(LENS, p["items"])):
        tables, gaps = item_doubles(n, L, max_w, extra)
        assert it == [k, n, min(n, L), -(-(n + 1) // 16) * 16, tables, gaps, (tables + gaps) * 8]


def test_chunking_under_a_budget_follows_those_bytes(exe):
    extra = int(subprocess.run([exe, "tables"], capture_output=True, text=True, check=True).stdout.split()[1])
    L = 33
    sizes = {w: [sum(item_doubles(n, L, w, extra)) * 8 for n in LENS] for w in (1, 15)}
    budget = max(sizes[15])
    want = {w: greedy(sizes[w], budget) for w in sizes}
    assert want[1] != want[15], "the same budget holds more items of a max_w = 1 batch"
    for w in sizes:
        p = plan(exe, L, w, budget, LENS)
        assert [c[1] for c in p["chunks"]] == want[w]
        assert all((c[2] + c[3]) * 8 <= budget for c in p["chunks"])
        assert len(plan(exe, L, w, 1, LENS)["chunks"]) == len(LENS)
