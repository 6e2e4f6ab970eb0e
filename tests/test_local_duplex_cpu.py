"""CPU suite: arguments, shapes and chunk sizes of local hybridization (rh_local_duplex; ractip_amd/csrc/local_windows.{h,cpp})
through the stand-alone program tools/local_duplex_check.cpp built with the host sanitizers: every rejection with its code and
exact text, the shape (query, windows, longest s1 / s2 of a chunk's pairs), the automatic chunk sizes against the layout functions
of batch.h restated here for both hybrid sources, and the sizes of a 200 x 10^6 matrix as size_t."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")
RH_ERR_ARG = -1
CHUNK_BYTES, CHUNK_MAX = 4 << 30, 32768   # kLocalChunkBytes, kLocalChunkMax


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "local_duplex_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "local_duplex_check.cpp"), os.path.join(CSRC, "local_windows.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def starts_restated(n, W, S):
    if n <= W:
        return [0]
    m = -(-(n - W) // S)
    return [k * S for k in range(m)] + [n - W]


# ---- rejections
@pytest.mark.parametrize("args,text", [
    ((7, 40, 2, 16, 1, "null1"), "local duplex: sequence 1 is NULL"),
    ((7, 40, 2, 16, 1, "null2"), "local duplex: sequence 2 is NULL"),
    ((0, 40, 2, 16, 1), "local duplex: sequence 1 has length 0 (must be >= 1)"),
    ((7, -1, 2, 16, 1), "local duplex: sequence 2 has length -1 (must be >= 1)"),
    ((7, 40, 0, 16, 1), "local duplex: windowed 0 (must be 1 or 2)"),
    ((7, 40, 3, 16, 1), "local duplex: windowed 3 (must be 1 or 2)"),
    ((7, 40, 2, 1, 1), "local duplex: window 1 (must be >= 2)"),
    ((7, 40, 1, 0, 1), "local duplex: window 0 (must be >= 2)"),
    ((7, 40, 2, 16, 0), "local duplex: step 0 (must be >= 1)"),
    ((7, 40, 2, 16, -2), "local duplex: step -2 (must be >= 1)"),
    ((7, 40, 2, 16, 17), "local duplex: step 17 exceeds the window 16"),
    ((7, 40, 1, 16, 17), "local duplex: step 17 exceeds the window 16"),
])
def test_every_rejection_with_its_text(exe, args, text):
    assert run(exe, "plan", *args) == "err %d %s\n" % (RH_ERR_ARG, text)


# ---- the shape: the shapes of tests/test_gpu_local_duplex.py in both roles, W >= n, a tie
SHAPES = [(7, 41, 16, 1), (23, 43, 16, 5), (60, 70, 65, 1), (23, 50, 33, 33), (60, 9, 16, 1), (7, 16, 16, 3), (23, 23, 16, 2), (100, 5000, 200, 20)]


@pytest.mark.parametrize("nq,n,W,S", SHAPES)
@pytest.mark.parametrize("windowed", [1, 2])
def test_the_shape(exe, nq, n, W, S, windowed):
    n1, n2 = (nq, n) if windowed == 2 else (n, nq)
    words = run(exe, "plan", n1, n2, windowed, W, S).split()
    assert words[0] == "ok" and words[9] == ":", words
    got = [int(x) for x in words[1:9]]
    starts, We = starts_restated(n, W, S), min(W, n)
    assert got == [n1, n2, windowed, nq, We, len(starts), nq if windowed == 2 else We, We if windowed == 2 else nq]
    assert [int(x) for x in words[10:]] == starts
    assert run(exe, "sizes", n1, n2, windowed, W, S) == "hp %d logz %d\n" % ((n1 + 1) * (n2 + 1), len(starts))


def test_sizes_of_a_query_on_a_million_letters_are_size_t(exe):
    for windowed, (n1, n2) in ((2, (200, 10 ** 6)), (1, (10 ** 6, 200))):
        assert run(exe, "sizes", n1, n2, windowed, 1000, 250) == "hp %d logz %d\n" % (201 * (10 ** 6 + 1), (10 ** 6 - 1000) // 250 + 1)
    # a longer query: the count of doubles itself passes 31 bits, the bytes 34
    assert run(exe, "sizes", 2200, 10 ** 6, 2, 1000, 250).split()[1] == str(2201 * (10 ** 6 + 1))
    assert 2201 * (10 ** 6 + 1) > 2 ** 31


# ---- chunk sizes: the layout functions of batch.h, restated
T_COUNT, VM_COUNT, D_COUNT, V_COUNT, DL_COUNT, VD_COUNT, VD_COUNT20, PK_COPIES, DX_PAD = 14, 16, 4, 6, 4, 6, 10, 6, 32
MODELS = {"contrafold": (T_COUNT, DL_COUNT, False), "vienna-duplex": (VM_COUNT, VD_COUNT, False), "vienna-cofold": (VM_COUNT, VD_COUNT, True),
          "vienna20-duplex": (VM_COUNT, VD_COUNT20, False)}


def mc_doubles(nmax, tables):
    """mc_layout: square tables, kPkCopies copies of the operand tiles, the posterior"""
    ld = (nmax + 3) & ~1
    nb = (nmax - 1) // 16 + 1
    tri = ((nmax + 1) * (nmax + 2) // 2 + 1) & ~1
    return tables * ld * ld + PK_COPIES * (nb * (nb + 1) // 2 * 256) + tri


def pair_doubles(n1max, n2max, dxl_tables, cofold):
    """dx_layout and dxl_layout share one buffer; the hp block; under cofold the tables of the concatenation"""
    ldd = (n2max + 3) & ~1
    tab = (n1max + 2) * ldd
    lda = (n1max + 2 + 2 * DX_PAD + 1) & ~1
    lin = (n1max + n2max + 3) * lda + 128
    return max(max(D_COUNT, V_COUNT) * tab, dxl_tables * lin) + tab + (mc_doubles(n1max + n2max, VM_COUNT) if cofold else 0)


def chunk_restated(budget, per_window, most):
    c = min(most, max(1, budget // per_window))
    return c & ~7 if c > 8 else c


CHUNKS = [(100, 20000, 200, 1), (100, 5000, 200, 20), (23, 43, 16, 5), (60, 70, 65, 1), (500, 100000, 1000, 100), (2000, 50000, 3000, 500),
          (30, 10 ** 6, 2, 1)]


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("nq,n,W,S", CHUNKS)
def test_automatic_chunks_come_from_the_layout_functions(exe, model, nq, n, W, S):
    fold_tables, dxl_tables, cofold = MODELS[model]
    We = min(W, n)
    for windowed in (1, 2):
        n1, n2 = (nq, n) if windowed == 2 else (n, nq)
        n1max, n2max = (nq, We) if windowed == 2 else (We, nq)
        words = run(exe, "chunk", n1, n2, windowed, W, S, model).split()
        got = dict(zip(words[0::2], (int(x) for x in words[1::2])))
        fold = 8 * mc_doubles(max(nq, We), fold_tables)
        pair = 8 * pair_doubles(n1max, n2max, dxl_tables, cofold)
        assert got["fold"] == fold and got["pair"] == pair
        assert got["chunk"] == chunk_restated(max(0, CHUNK_BYTES - fold), fold + pair, CHUNK_MAX - 1)   # the query counts once
        assert got["fold_only"] == chunk_restated(CHUNK_BYTES, 8 * mc_doubles(We, fold_tables), CHUNK_MAX)
        assert 1 <= got["chunk"] <= CHUNK_MAX - 1 and (got["chunk"] <= 8 or got["chunk"] % 8 == 0)
        assert got["chunk"] <= got["fold_only"]                      # a window with its pair is never cheaper than the window alone
        if got["chunk"] > 8:
            assert fold + got["chunk"] * (fold + pair) <= CHUNK_BYTES


def test_cofold_counts_the_joint_tables(exe):
    """the two hybrid sources differ by mc_layout(1, nq + We, VM_COUNT) with its tile copies, and the chunk shrinks accordingly"""
    a = dict(zip(*[iter(run(exe, "chunk", 100, 20000, 2, 200, 1, "vienna-duplex").split())] * 2))
    b = dict(zip(*[iter(run(exe, "chunk", 100, 20000, 2, 200, 1, "vienna-cofold").split())] * 2))
    assert int(b["pair"]) - int(a["pair"]) == 8 * mc_doubles(300, VM_COUNT)
    assert int(b["chunk"]) < int(a["chunk"]) and a["fold"] == b["fold"]
    assert int(run(exe, "chunk", 2, 10 ** 6, 2, 2, 1, "contrafold").split()[1]) == (CHUNK_MAX - 1) & ~7   # tiny windows: the cap, a multiple of 8


# ---- the pipeline's argument checks (no GPU: both answer before a context exists)
def test_local_hp_needs_a_window(tmp_path):
    from ractip_amd import pipeline
    with pytest.raises(ValueError, match="local_hp needs a window"):
        pipeline.predict("ACGU", "ACGU", local_hp=True)
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGUACGU\n")
    with pytest.raises(SystemExit, match="--local-hp requires --window"):
        pipeline.main(["--local-hp", str(fa), str(fa)])
