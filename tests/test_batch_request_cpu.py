"""CPU suite: what an upload is checked and sized by, through the stand-alone program tools/batch_request_check.cpp built with the
host sanitizers: the layout functions of ractip_amd/csrc/batch.h against a restatement of the formulas written here, the shape
check_batch (ractip_amd/csrc/batch_request.cpp) derives from a request, every rejection with its code and exact text -- the texts
the GPU tests pin, from their own strings -- and hairpin_length_weights bit for bit."""
import os
import subprocess

import pytest

import _indexed_constraint_cases as cases
from test_gpu_batch_constraints import ragged_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")
RH_ERR_ARG, RH_ERR_UNSUPPORTED = -1, -5
EDGES = (1, 2, 13, 14, 15, 16, 17, 29, 30, 31, 57, 58, 59, 64, 109, 110)
NONCOMP = "a forced pair of non-complementary letters (pair type 7) is not supported"
VIENNA_ONLY = "structure constraints apply to the Vienna-BL model only (RactIP::contrafold takes none)"


# ---- the layouts, restated
def tri_size(n):
    return (n + 1) * (n + 2) // 2


def seq_lds(nmax):
    return (nmax + 18) & ~15


def mc_restated(nmax, tables):
    ld = (nmax + 3) & ~1
    nb = (nmax - 1) // 16 + 1
    return dict(ld=ld, lds=seq_lds(nmax), tab_stride=ld * ld, seq_stride=ld * ld * tables, tri_stride=(tri_size(nmax) + 1) & ~1, nb=nb,
                pk_stride=nb * (nb + 1) // 2 * 256)


def dx_restated(n1max, n2max, tables):
    ldd = (n2max + 3) & ~1
    return dict(ldd=ldd, tab_stride=(n1max + 2) * ldd, pair_stride=(n1max + 2) * ldd * tables)


def dxl_restated(n1max, n2max, tables):
    lda = (n1max + 2 + 64 + 1) & ~1
    tab = (n1max + n2max + 3) * lda + 128
    return dict(lda=lda, tab_stride=tab, pair_stride=tab * tables, lz_chunks=(n1max + n2max - 1 + 15) // 16)


def batch_layout_restated(lens1, lens2, max_w, nmax=None):
    """(tri_stride, up_ld, hp_stride, hp_ld) as rh_batch_layout reports them for pairs of these lengths"""
    nmax = max(lens1 + lens2) if nmax is None else nmax
    m, d = mc_restated(nmax, 1), dx_restated(max(lens1), max(lens2), 1)
    return m["tri_stride"], m["ld"] * max_w, d["tab_stride"], d["ldd"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "batch_request_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "batch_request_check.cpp"), os.path.join(CSRC, "batch_request.cpp"),
                           os.path.join(CSRC, "constraint_prepass.cpp"), "-o", path])
    return path


def test_layout_functions_equal_the_restated_formulas(exe):
    r = subprocess.run([exe, "layouts"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    words = lines[0].split()
    assert words[0] == "counts"
    count = {words[k]: int(words[k + 1]) for k in range(1, len(words), 2)}
    assert count["T"] < count["VM"] and count["VD"] < count["VD20"]
    seen = {"mc": set(), "dx": set(), "dxl": set()}
    for line in lines[1:-1]:
        key, vals = line.split(" : ")
        kind, *args = key.split()
        args, v = [int(x) for x in args], [int(x) for x in vals.split()]
        if kind == "mc":
            nmax, tables = args
            m = mc_restated(nmax, tables)
            assert tables in (count["T"], count["VM"])
            assert v == [7, nmax, m["ld"], m["lds"], m["tab_stride"], m["seq_stride"], m["tri_stride"], m["nb"], m["pk_stride"]], line
        elif kind == "dx":
            n1, n2 = args
            d = dx_restated(n1, n2, count["V"])
            assert v == [5, n1, n2, d["ldd"], seq_lds(max(n1, n2)), d["tab_stride"], d["pair_stride"]], line
        else:
            n1, n2 = args
            x = dxl_restated(n1, n2, count["VD20"])
            assert v == [5, n1, n2, x["lda"], seq_lds(max(n1, n2)), dx_restated(n1, n2, 1)["ldd"], x["tab_stride"], x["pair_stride"], x["lz_chunks"]], line
        seen[kind].add(tuple(args))
    assert seen["mc"] == {(n, t) for n in range(1, 201) for t in (count["T"], count["VM"])}
    assert seen["dx"] == seen["dxl"] == {(a, b) for a in EDGES for b in EDGES}
    assert lines[-1] == "unset 0"
    # the range crosses the steps of lds, ld and nb
    assert seq_lds(13) != seq_lds(14) and mc_restated(14, 1)["ld"] != mc_restated(15, 1)["ld"] and mc_restated(16, 1)["nb"] != mc_restated(17, 1)["nb"]


def test_hairpin_length_weights_have_the_bits_of_the_expression(exe):
    r = subprocess.run([exe, "hairpin"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["entries", "45", "differ", "0"], (r.stdout, r.stderr[-4000:])


# ---- requests
def request(model, seqs, folds=True, pairs=True, index=None, lens=None, **arrays):
    """arrays: fold / joint / first / second = a list of strings or None per entry"""
    out = ["model " + model] + (["folds"] if folds else []) + (["pairs"] if pairs else [])
    for k, s in enumerate(seqs):
        out.append("seq %d %s" % (len(s) if lens is None or lens[k] is None else lens[k], "NULL" if s is None else s))
    if index is not None:
        out += ["indexed"] + ["index %d %d" % tuple(p) for p in index]
    for name, entries in arrays.items():
        if entries is None:
            continue
        out.append(name)
        out += ["%s %d %s" % (name, k, e or '""') for k, e in enumerate(entries) if e is not None]
    return "\n".join(out + ["end"]) + "\n"


def answers(exe, requests):
    r = subprocess.run([exe, "check"], input="".join(requests), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests)
    return lines


def shape_of(line):
    words = line.split()
    assert words[0] == "ok", line
    at = words.index("pair_seq")
    d = {words[k]: int(words[k + 1]) for k in range(1, at, 2)}
    d["pair_seq"] = [int(x) for x in words[at + 1:words.index("codes")]]
    d["codes"] = words[words.index("codes") + 1]
    return d


def rnd(n, seed):
    import numpy as np
    return "".join(np.random.RandomState(seed).choice(list("ACGU"), n))


def test_shapes_of_a_plain_an_indexed_and_a_fold_only_request(exe):
    plain = [rnd(n, 10 + n) for n in (61, 45, 13, 29, 40, 17)]
    distinct = [rnd(n, 30 + n) for n in (33, 7, 58, 20)]
    index = [(0, 1), (2, 2), (1, 0), (3, 2), (1, 3)]            # (2, 2) a self pair; 0, 1, 2 and 3 in both roles
    got = [shape_of(a) for a in answers(exe, [request("contrafold", plain), request("vienna", distinct, index=index),
                                              request("vienna", [plain[0]], pairs=False)])]
    base = dict(fold=0, joint=0, shares=0)
    assert {k: got[0][k] for k in got[0] if k != "codes"} == dict(base, indexed=0, np=3, nmax=61, n1max=61, n2max=45, cut_min=13, cut_max=61,
                                                                  lds=seq_lds(61), co_lds=seq_lds(61 + 45), pair_seq=[0, 1, 2, 3, 4, 5])
    assert {k: got[1][k] for k in got[1] if k != "codes"} == dict(base, indexed=1, np=5, nmax=58, n1max=58, n2max=58, cut_min=7, cut_max=58,
                                                                  lds=seq_lds(58), co_lds=seq_lds(116), pair_seq=[0, 1, 2, 2, 1, 0, 3, 2, 1, 3])
    assert {k: got[2][k] for k in got[2] if k != "codes"} == dict(base, indexed=0, np=0, nmax=61, n1max=0, n2max=0, cut_min=0, cut_max=0,
                                                                  lds=seq_lds(61), co_lds=seq_lds(0), pair_seq=[])
    # the codes: [ns][lds], the model's sentinel around each sequence and behind it
    cf, vi = "ACGU".index, " ACGU".index
    assert got[0]["codes"] == "".join("4" + "".join(str(cf(x)) for x in s) + "4" * (seq_lds(61) - 1 - len(s)) for s in plain)
    assert got[2]["codes"] == "0" + "".join(str(vi(x)) for x in plain[0]) + "0" * (seq_lds(61) - 62)


def test_every_rejection_has_its_code_and_text(exe):
    pairs, cons, joint = ragged_batch()
    flat = [s for pr in pairs for s in pr]
    fold = [x for c in cons for x in c]

    def changed(seq, k, value):
        out = list(seq)
        out[k] = value
        return out
    seqs, icons, first, second, index = cases.batch()
    gg = ["GAAG", "GGGAAACCC", "GGGAAACCC", "GAAG"]
    g, a = seqs[4].index("G", 13), seqs[5].index("C", 8)
    two = ["ACGU", "ACG"]
    unbal = " in the structure constraint"
    want = [
        # lengths, NULLs, counts, indices
        (request("contrafold", two, lens=[None, 0]), RH_ERR_ARG, "sequence 1 has length 0 (must be >= 1)"),
        (request("vienna", [two[0], None], lens=[None, 3]), RH_ERR_ARG, "sequence 1 is NULL"),
        (request("contrafold", two + ["A"]), RH_ERR_ARG, "duplex batch needs an even number of sequences"),
        (request("contrafold", two, index=[]), RH_ERR_ARG, "indexed batch of 0 pairs (must be >= 1)"),
        (request("vienna", seqs, index=[(0, 1), (1, 9)], fold=icons), RH_ERR_ARG, "pair 1 = (1, 9): index outside [0, 9)"),
        (request("vienna", seqs, index=[(0, 1), (-1, 2)]), RH_ERR_ARG, "pair 1 = (-1, 2): index outside [0, 9)"),
        # fold constraints, plain and indexed
        (request("vienna", flat, fold=changed(fold, 5, "..((.."), joint=joint), RH_ERR_ARG, "sequence 5: unbalanced '('" + unbal),
        (request("vienna", flat, fold=changed(fold, 5, "..)"), joint=joint), RH_ERR_ARG, "sequence 5: unbalanced ')'" + unbal),
        (request("vienna", seqs, index=index, fold=changed(icons, 5, "..((.."), first=cases.CO_FIRST, second=cases.CO_SECOND), RH_ERR_ARG,
         "sequence 5: unbalanced '('" + unbal),
        (request("vienna", seqs, index=index, fold=changed(icons, 6, ".)")), RH_ERR_ARG, "sequence 6: unbalanced ')'" + unbal),
        (request("vienna", gg, fold=[None, "(((...)))", "(((...)))", "(..)"]), RH_ERR_ARG, "sequence 3: " + NONCOMP),
        (request("vienna", ["N" + "A" * 30 + "A", "G" + "A" * 30 + "C"], fold=["(" + "." * 30 + ")"] * 2), RH_ERR_ARG, "sequence 0: " + NONCOMP),
        # per-pair strings of a plain batch
        (request("vienna", gg, joint=[None, "(" + "." * 11 + ")"]), RH_ERR_ARG, "pair 1: " + NONCOMP),
        (request("vienna", gg, joint=["(...", None]), RH_ERR_ARG, "pair 0: unbalanced '('" + unbal),
        # shares
        (request("vienna", seqs, index=index, first=cases.CO_FIRST, second=changed(cases.CO_SECOND, 3, cases.CO_SECOND[4])), RH_ERR_ARG,
         "pair 2: unbalanced '('" + unbal + " (2 open in the first share, 1 in the second)"),
        (request("vienna", seqs, index=index, first=changed(cases.CO_FIRST, 2, "...)" + cases.CO_FIRST[2][4:]), second=cases.CO_SECOND), RH_ERR_ARG,
         "pair 3: unbalanced ')'" + unbal + " (left open in the first share)"),
        (request("vienna", seqs, index=index, first=cases.CO_FIRST, second=changed(cases.CO_SECOND, 4, cases.CO_SECOND[4][:28] + "(" + cases.CO_SECOND[4][29:])),
         RH_ERR_ARG, "pair 6: unbalanced '('" + unbal + " (left open in the second share)"),
        (request("vienna", seqs, index=index, first=cases.CO_FIRST, second=changed(cases.CO_SECOND, 4, "." * g + ")")), RH_ERR_ARG, "pair 6: " + NONCOMP),
        (request("vienna", seqs, index=index, first=changed(cases.CO_FIRST, 5, "." * a + "(" + "." * (14 - a) + ")"), second=cases.CO_SECOND), RH_ERR_ARG,
         "pair 9: " + NONCOMP),
        # another model than Vienna-BL takes no constraint, plain or indexed, whichever array carries it
        (request("contrafold", flat, fold=fold), RH_ERR_UNSUPPORTED, VIENNA_ONLY),
        (request("contrafold", flat, joint=joint), RH_ERR_UNSUPPORTED, VIENNA_ONLY),
        (request("contrafold", seqs, index=index, fold=icons), RH_ERR_UNSUPPORTED, VIENNA_ONLY),
        (request("contrafold", seqs, index=index, first=cases.CO_FIRST), RH_ERR_UNSUPPORTED, VIENNA_ONLY),
        (request("contrafold", seqs, index=index, second=cases.CO_SECOND), RH_ERR_UNSUPPORTED, VIENNA_ONLY),
        (request("contrafold", [flat[0]], pairs=False, fold=["."]), RH_ERR_UNSUPPORTED, VIENNA_ONLY),
        # which of two errors wins: the model, then lengths, then indices, then the fold constraints, then the joint ones
        (request("contrafold", two, lens=[0, None], fold=["(", None]), RH_ERR_UNSUPPORTED, VIENNA_ONLY),
        (request("vienna", two, lens=[None, 0], fold=["(", None]), RH_ERR_ARG, "sequence 1 has length 0 (must be >= 1)"),
        (request("vienna", two, lens=[0, None], index=[(0, 5)]), RH_ERR_ARG, "sequence 0 has length 0 (must be >= 1)"),
        (request("vienna", two, index=[(0, 5)], fold=["(", None]), RH_ERR_ARG, "pair 0 = (0, 5): index outside [0, 2)"),
        (request("vienna", gg, fold=[None, None, None, ")"], joint=["(...", None]), RH_ERR_ARG, "sequence 3: unbalanced ')'" + unbal),
    ]
    got = answers(exe, [w[0] for w in want])
    for line, (_, code, text) in zip(got, want):
        assert line == "err %d %s" % (code, text)


def test_accepted_requests_say_which_constraints_apply(exe):
    pairs, cons, joint = ragged_batch()
    flat = [s for pr in pairs for s in pr]
    fold = [x for c in cons for x in c]
    seqs, icons, first, second, index = cases.batch()
    none_s, none_p = [None] * len(seqs), [None] * len(pairs)
    reqs = [
        request("vienna", flat, fold=fold, joint=joint),
        request("vienna", seqs, index=index, fold=icons, first=first, second=second),
        request("vienna", seqs[5:], index=[(0, 1), (2, 0)], second=second[5:]),      # shares in one role only (none of them leaves a bracket open)
        # arrays whose entries are all NULL: no constraint, under either model
        request("contrafold", flat, fold=[None] * len(flat), joint=none_p),
        request("vienna", flat, fold=[None] * len(flat), joint=none_p),
        request("contrafold", seqs, index=index, fold=none_s, first=none_s, second=none_s),
        request("vienna", seqs, index=index, fold=none_s, first=None, second=none_s),
        # a constraint where it does not apply is not looked at: fold constraints without folds
        request("vienna", flat[:2], folds=False, fold=["((((", None]),
    ]
    got = [shape_of(a) for a in answers(exe, reqs)]
    flags = [(s["fold"], s["joint"], s["shares"]) for s in got]
    assert flags[:3] == [(1, 1, 0), (1, 0, 1), (0, 0, 1)] and flags[3:] == [(0, 0, 0)] * 5, flags
    assert got[0]["pair_seq"] == list(range(len(flat))) and got[1]["pair_seq"] == [x for p in index for x in p]
