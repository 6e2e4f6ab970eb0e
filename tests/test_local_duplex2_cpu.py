"""CPU suite: arguments, shapes, tile sizes and tile walk of local hybridization of two windowed molecules (rh_local_duplex2;
ractip_amd/csrc/local_windows.{h,cpp}) through the stand-alone program tools/local_duplex2_check.cpp built with the host sanitizers:
every rejection with its code and exact text, the shapes of the GPU cases, the sizes of a 10^5 x 10^5 matrix as size_t, the automatic
tile against the rule restated here from the layout functions of batch.h, and the walk -- every window pair once, row blocks in
increasing k, column tiles in increasing l -- with a numpy simulation of the row-buffer accumulation over it, which must give the
bits of the definition under every tiling."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")
RH_ERR_ARG = -1
CHUNK_BYTES, CHUNK_MAX = 4 << 30, 32768   # kLocalChunkBytes, kLocalChunkMax


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "local_duplex2_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "local_duplex2_check.cpp"), os.path.join(CSRC, "local_windows.cpp"), "-o", path])
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


# ---- rejections: (n1, n2, W1, S1, W2, S2[, nullK])
@pytest.mark.parametrize("args,text", [
    ((23, 41, 16, 5, 16, 5, "null1"), "local duplex2: sequence 1 is NULL"),
    ((23, 41, 16, 5, 16, 5, "null2"), "local duplex2: sequence 2 is NULL"),
    ((0, 41, 16, 5, 16, 5), "local duplex2: sequence 1 has length 0 (must be >= 1)"),
    ((23, -1, 16, 5, 16, 5), "local duplex2: sequence 2 has length -1 (must be >= 1)"),
    ((23, 41, 1, 1, 16, 5), "local duplex2: window1 1 (must be >= 2)"),
    ((23, 41, 16, 5, 0, 1), "local duplex2: window2 0 (must be >= 2)"),
    ((23, 41, 16, 0, 16, 5), "local duplex2: step1 0 (must be >= 1)"),
    ((23, 41, 16, 5, 16, -2), "local duplex2: step2 -2 (must be >= 1)"),
    ((23, 41, 16, 17, 16, 5), "local duplex2: step1 17 exceeds window1 16"),
    ((23, 41, 16, 5, 33, 34), "local duplex2: step2 34 exceeds window2 33"),
    ((10 ** 6, 10 ** 6, 2, 1, 2, 1), "local duplex2: 999999 x 999999 window pairs (at most 2147483647)"),
])
def test_every_rejection_with_its_text(exe, args, text):
    assert run(exe, "plan", *args) == "err %d %s\n" % (RH_ERR_ARG, text)


def test_the_pair_count_is_taken_in_64_bits(exe):
    """999999^2 wraps to a small positive int in 32 bits: the rejection above needs the 64-bit product; 46341 x 46341 is the first
    square above 2^31 - 1, 46340 x 46341 the largest accepted product of this kind"""
    assert 46341 * 46341 > 2 ** 31 - 1 >= 46340 * 46341
    assert run(exe, "plan", 46342, 46342, 2, 1, 2, 1).startswith("err %d local duplex2: 46341 x 46341 window pairs" % RH_ERR_ARG)
    assert run(exe, "sizes", 46341, 46342, 2, 1, 2, 1).split()[3] == str(46340 * 46341)


# ---- shapes: the cases of tests/test_gpu_local_duplex2.py and one of production size
SHAPES = {"A": (23, 16, 5, 41, 16, 5), "B": (41, 16, 1, 23, 16, 5), "C": (50, 33, 33, 43, 33, 5), "D": (70, 65, 1, 70, 65, 5),
          "E": (9, 16, 1, 41, 16, 1), "F": (16, 16, 1, 16, 16, 1), "long": (2000, 200, 50, 5000, 200, 50)}
WINDOWS = {"A": (3, 6), "B": (26, 3), "C": (2, 3), "D": (6, 2), "E": (1, 26), "F": (1, 1), "long": (37, 97)}


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_the_shape(exe, case):
    n1, W1, S1, n2, W2, S2 = SHAPES[case]
    head, rest = run(exe, "plan", n1, n2, W1, S1, W2, S2).split(":")
    a, b = starts_restated(n1, W1, S1), starts_restated(n2, W2, S2)
    assert (len(a), len(b)) == WINDOWS[case]
    assert head.split() == ["ok"] + [str(x) for x in (n1, n2, min(W1, n1), len(a), min(W2, n2), len(b))]
    got1, got2 = rest.split("|")
    assert [int(x) for x in got1.split()] == a and [int(x) for x in got2.split()] == b
    assert run(exe, "sizes", n1, n2, W1, S1, W2, S2) == "hp %d logz %d rowbuf %d\n" % (
        (n1 + 1) * (n2 + 1), len(a) * len(b), (min(W1, n1) + 1) * (n2 + 1))


def test_sizes_are_size_t(exe):
    words = run(exe, "sizes", 10 ** 5, 10 ** 5, 1000, 250, 1000, 250).split()
    nw = (10 ** 5 - 1000) // 250 + 1
    assert words == ["hp", str((10 ** 5 + 1) ** 2), "logz", str(nw * nw), "rowbuf", str(1001 * (10 ** 5 + 1))]
    assert (10 ** 5 + 1) ** 2 > 2 ** 33


# ---- the automatic tile: the layout functions of batch.h, restated
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


def tile_restated(fold, pair, rowbuf, nw1, nw2):
    """the rule of the interface: the largest t with 2t fold + t^2 pair + t rowbuf under the budget; clip; grow the unclipped side"""
    def fits(r, c):
        return r + c <= CHUNK_MAX and r * c <= CHUNK_MAX - 1 and (r + c) * fold + r * c * pair + r * rowbuf <= CHUNK_BYTES
    t = max([x for x in range(1, 200) if fits(x, x)], default=1)
    assert not fits(200, 200)                                   # (the pair cap alone ends the search below 182)
    rows, cols = min(t, nw1), min(t, nw2)
    if rows < t:
        while cols < nw2 and fits(rows, cols + 1):
            cols += 1
    elif cols < t:
        while rows < nw1 and fits(rows + 1, cols):
            rows += 1
    return rows, cols


# (n1, W1, S1, n2, W2, S2): neither side clipped; s1 one window, cols grow to a byte limit; s2 clipped, rows grow; tiny windows at the
# pair cap; tiny windows, two / one rows, cols grow to the pair / sequence cap; a row buffer of 2.25 GB (t = 1); one above the budget
TILES = [(2000, 200, 50, 5000, 200, 50), (100, 200, 50, 50000, 200, 50), (50000, 200, 50, 300, 200, 50), (1000, 2, 1, 1000, 2, 1),
         (3, 2, 1, 10 ** 5, 2, 1), (2, 2, 1, 10 ** 5, 2, 1), (5000, 200, 50, 1400000, 200, 50),(5000, 1000, 250, 10 ** 6, 200, 50),
         (23, 16, 5, 41, 16, 5), (70, 65, 1, 70, 65, 5)]


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("n1,W1,S1,n2,W2,S2", TILES)
def test_automatic_tiles_come_from_the_layout_functions(exe, model, n1, W1, S1, n2, W2, S2):
    fold_tables, dxl_tables, cofold = MODELS[model]
    We1, We2 = min(W1, n1), min(W2, n2)
    nw1, nw2 = len(starts_restated(n1, W1, S1)), len(starts_restated(n2, W2, S2))
    words = run(exe, "tile", n1, n2, W1, S1, W2, S2, model).split()
    got = dict(zip(words[0::2], (int(x) for x in words[1::2])))
    fold = 8 * mc_doubles(max(We1, We2), fold_tables)
    pair = 8 * pair_doubles(We1, We2, dxl_tables, cofold)
    rowbuf = 8 * (We1 + 1) * (n2 + 1)
    assert (got["fold"], got["pair"], got["rowbuf"]) == (fold, pair, rowbuf)
    assert (got["rows"], got["cols"]) == tile_restated(fold, pair, rowbuf, nw1, nw2)
    assert 1 <= got["rows"] <= nw1 and 1 <= got["cols"] <= nw2
    assert got["rows"] + got["cols"] <= CHUNK_MAX and got["rows"] * got["cols"] <= CHUNK_MAX - 1


def test_the_tile_cases_reach_what_they_name(exe):
    def tile(shape, model="contrafold"):
        n1, W1, S1, n2, W2, S2 = shape
        w = run(exe, "tile", n1, n2, W1, S1, W2, S2, model).split()
        return int(w[1]), int(w[3])
    r, c = tile(TILES[0])
    assert r == c and 1 < r < 37                                # a square tile inside the 37 x 97 grid
    r, c = tile(TILES[1])
    assert r == 1 and r < c < 997                               # one window of s1: the columns grew, up to the bytes
    r, c = tile(TILES[2])
    assert c == 3 and c < r < 997                               # three windows of s2: the rows grew
    assert tile(TILES[3]) == (181, 181)                         # 181^2 <= 32767 < 182^2
    assert tile(TILES[4]) == (2, 16383)                         # 2 x 16383 <= 32767
    assert tile(TILES[5]) == (1, 32767)                         # 1 + 32767 = 32768 sequences
    assert tile(TILES[6]) == (1, 1) and tile(TILES[7]) == (1, 1)
    assert tile(TILES[0], "vienna-cofold")[0] < tile(TILES[0], "vienna-duplex")[0]   # the joint tables count


# ---- the walk
def walk(exe, shape, rows, cols, model="contrafold"):
    n1, W1, S1, n2, W2, S2 = shape
    return [tuple(int(x) for x in line.split()) for line in run(exe, "walk", n1, n2, W1, S1, W2, S2, model, rows, cols).splitlines()]


def definition(shape, h):
    """hp_loc2 by the definition: row sums first, then the sum over k, then one division"""
    n1, W1, S1, n2, W2, S2 = shape
    a, b, We1, We2 = starts_restated(n1, W1, S1), starts_restated(n2, W2, S2), min(W1, n1), min(W2, n2)
    acc, c1, c2 = np.zeros((n1 + 1, n2 + 1)), np.zeros(n1 + 1), np.zeros(n2 + 1)
    for k, sa in enumerate(a):
        row = np.zeros((We1, n2 + 1))
        for l, sb in enumerate(b):
            row[:, sb + 1:sb + We2 + 1] += h[k][l]
        acc[sa + 1:sa + We1 + 1] += row
        c1[sa + 1:sa + We1 + 1] += 1
    for sb in b:
        c2[sb + 1:sb + We2 + 1] += 1
    assert c1[1:].min() >= 1 and c2[1:].min() >= 1
    acc[1:, 1:] /= c1[1:, None] * c2[None, 1:]
    return acc


def simulate(shape, h, tiles):
    """the three kernels over a walk, with buffers that start as NaN: a row buffer entry starts from 0 in the first column tile that
    holds one of its column's windows and continues otherwise; a row of hp starts from 0 in the first row block that holds one of
    its windows; nothing is cleared as a whole"""
    n1, W1, S1, n2, W2, S2 = shape
    a, b, We1, We2 = starts_restated(n1, W1, S1), starts_restated(n2, W2, S2), min(W1, n1), min(W2, n2)
    first1 = np.array([min(k for k, s in enumerate(a) if s < i <= s + We1) for i in range(1, n1 + 1)])   # lo of letter i
    first2 = np.array([min(l for l, s in enumerate(b) if s < j <= s + We2) for j in range(1, n2 + 1)])
    rows = max(kB - kA for kA, kB, _, _ in tiles)
    R = np.full((rows, We1, n2 + 1), np.nan)
    acc = np.full((n1 + 1, n2 + 1), np.nan)
    for kA, kB, lA, lB in tiles:
        for k in range(kA, kB):
            for l in range(lA, lB):                             # local_hp_col_gather: per column its windows of the tile in increasing l
                sl = slice(b[l] + 1, b[l] + We2 + 1)
                lo = first2[b[l]:b[l] + We2]
                starts_here = (lo >= lA) & (np.maximum(lo, lA) == l)
                R[k - kA][:, sl] = np.where(starts_here[None, :], 0.0, R[k - kA][:, sl]) + h[k][l]
        if lB == len(b):                                        # local_hp_row_gather: per row its windows of the block in increasing k
            for k in range(kA, kB):
                sl = slice(a[k] + 1, a[k] + We1 + 1)
                lo = first1[a[k]:a[k] + We1]
                starts_here = (lo >= kA) & (np.maximum(lo, kA) == k)
                acc[sl, 1:] = np.where(starts_here[:, None], 0.0, acc[sl, 1:]) + R[k - kA][:, 1:]
    c1 = np.array([sum(s < i <= s + We1 for s in a) for i in range(1, n1 + 1)], dtype=float)
    c2 = np.array([sum(s < j <= s + We2 for s in b) for j in range(1, n2 + 1)], dtype=float)
    acc[1:, 1:] /= c1[:, None] * c2[None, :]                    # local_hp2_finish
    acc[0, :] = 0.0
    acc[:, 0] = 0.0
    return acc


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "F"])
def test_the_walk_visits_every_pair_once_in_order_and_gives_the_bits_of_the_definition(exe, case):
    shape = SHAPES[case]
    n1, W1, S1, n2, W2, S2 = shape
    nw1, nw2 = WINDOWS[case]
    rng = np.random.RandomState(nw1 * 100 + nw2)
    h = [[rng.rand(min(W1, n1), min(W2, n2)) for _ in range(nw2)] for _ in range(nw1)]
    want = definition(shape, h)
    assert np.isfinite(want).all() and not want[0].any() and not want[:, 0].any()
    for rows, cols in ((1, 1), (2, 3), (3, 2), (nw1, 1), (1, nw2), (0, 0)):
        tiles = walk(exe, shape, rows, cols)
        r, c = (min(rows, nw1), min(cols, nw2)) if rows else (nw1, nw2)   # (these grids fit one automatic tile)
        seen = [(k, l) for kA, kB, lA, lB in tiles for k in range(kA, kB) for l in range(lA, lB)]
        assert sorted(seen) == [(k, l) for k in range(nw1) for l in range(nw2)], (rows, cols)          # every pair exactly once
        assert tiles == [(kA, min(kA + r, nw1), lA, min(lA + c, nw2)) for kA in range(0, nw1, r) for lA in range(0, nw2, c)]
        blocks = [t[0] for t in tiles]
        assert blocks == sorted(blocks)                                                                 # row blocks in increasing k
        for kA in set(blocks):
            inside = [t[2] for t in tiles if t[0] == kA]
            assert inside == sorted(inside) and len(set(inside)) == len(inside)                        # column tiles in increasing l
        assert np.array_equal(simulate(shape, h, tiles), want), (rows, cols)


def test_the_walk_of_a_grid_larger_than_its_automatic_tile(exe):
    shape = SHAPES["long"]
    tiles = walk(exe, shape, 0, 0, "vienna-cofold")
    words = run(exe, "tile", shape[0], shape[3], shape[1], shape[2], shape[4], shape[5], "vienna-cofold").split()
    r, c = int(words[1]), int(words[3])
    assert r < 37 and c < 97
    assert tiles == [(kA, min(kA + r, 37), lA, min(lA + c, 97)) for kA in range(0, 37, r) for lA in range(0, 97, c)]


# ---- the pipeline's argument checks (no GPU: they answer before a context exists)
def test_local_hp_both_needs_a_window_and_excludes_local_hp(tmp_path):
    from ractip_amd import pipeline
    with pytest.raises(ValueError, match="local_hp_both needs a window"):
        pipeline.predict("ACGU", "ACGU", local_hp_both=True)
    with pytest.raises(ValueError, match="local_hp_both and local_hp exclude each other"):
        pipeline.predict("ACGU", "ACGU", window=4, local_hp=True, local_hp_both=True)
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGUACGU\n")
    with pytest.raises(SystemExit, match="--local-hp-both requires --window"):
        pipeline.main(["--local-hp-both", str(fa), str(fa)])
