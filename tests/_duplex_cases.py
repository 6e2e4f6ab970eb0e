"""The inputs of tests/test_gpu_duplex_edges.py (its docstring says what the constants are taken from), in a helper of their own so
that CPU tests and other GPU modules can build them without importing a GPU test module."""
import numpy as np

DUMMY = (300, 300)                         # first pair of every batch: fixes n1max / n2max (and so the table layout and the grids)


# ---- 1. the inputs
def edge_shapes(model):
    """(L1, L2) per model ("contrafold" / "vienna"), chosen from the kernel constants."""
    if model == "contrafold":
        return [
            # dxl_strip8, GS = 58: group g owns columns 58 g .. 58 g + 57 (outside) / is computed on 58 g - 6 .. 58 g + 57 (inside)
            (57, 200),    # L1 = GS - 1: the stationary edge ahi = L1 on the last column of group 0
            (58, 58),     # L1 = GS: on the first column of group 1; square
            (59, 61),     # L1 = GS + 1
            (60, 58),     # L1 = GS + 2; (L1 + L2 - 1) % 8 = 5, the one residue the other shapes leave out
            (115, 9),     # 2 GS - 1, short second strand: few rows, every strip has both ends of the band in it
            (116, 57),    # 2 GS
            (117, 118),   # 2 GS + 1
            (173, 174),   # 3 GS - 1
            (232, 233),   # 4 GS
            # degenerate strands: one cell per row (L2 = 1) or per column (L1 = 1); alo moves over the group edges with sd
            (174, 1),     # 3 GS
            (1, 174),
            (64, 1),      # one wavefront of dxl_sweep<W>
            (7, 300),     # n2max of the dummy: the band [alo - 32, ahi + 32] is wider than the strand
            (300, 7),     # n1max of the dummy
            # the 62-column groups of dxl_sweep4 and the 64-column groups of dxl_sweep<W>
            (63, 66),     # 62 + 1 / 64 - 1
            (62, 65),     # 62 / 64 + 1
            (124, 62),    # 2 * 62
            # dxl_posterior tiles of 32 anti-diagonals x 32 columns; dxl_logz_part items of 256 columns, chunks of kLzRows = 16 rows
            (33, 32),     # 32 + 1 columns, 64 rows
            (32, 33),     # 32 columns, 64 rows
            (26, 39),     # L1 + L2 - 1 = 64 rows = 2 tiles = 4 chunks exactly
            (257, 300),   # rows of 257 cells: the second item (k = 1) of a row holds one cell
        ]
    if model == "vienna":
        return [
            # dxvl_sweep4<S20>: groups advance by 62 columns, lanes 62 / 63 of a group are recomputed by the next
            (61, 9),      # 62 - 1
            (62, 62),     # 62: a0 + 62 > n1max + 1 alone
            (63, 64),     # 62 + 1
            (123, 200),   # 2 * 62 - 1
            (124, 62),    # 2 * 62
            (125, 40),    # 2 * 62 + 1
            (186, 187),   # 3 * 62
            (248, 249),   # 4 * 62
            # degenerate strands
            (1, 130),
            (130, 1),
            (7, 250),
            (250, 7),
            # dxvl_logz_part: chunks of 16 rows (rows sd = 2 .. L1 + L2: L1 + L2 - 1 of them) on both sides of a multiple of 16
            (31, 34),     # 64 rows: four chunks exactly
            (2, 30),      # 31 rows: the second chunk is one row short
            (31, 33),     # 63 rows
            (31, 35),     # 65 rows: the fifth chunk holds the last row alone
        ]
    raise ValueError(model)


def rnd(rng, n):
    return "".join(rng.choice(list("ACGU"), n))


def edge_pairs(model):
    """The sequences of edge_shapes(model): seeded random ACGU."""
    rng = np.random.RandomState(58 if model == "contrafold" else 62)
    return [(rnd(rng, a), rnd(rng, b)) for a, b in edge_shapes(model)]


STEM_A, STEM_B = "GGCGCGCC", "GCCGGCGG"


def rc(s):
    return "".join({"A": "U", "C": "G", "G": "C", "U": "A"}[ch] for ch in reversed(s))


def planted(edge, l1, l2, on="A", tails=(20, 20, 10)):
    """A pair dominated by two 8-bp GC stems joined by one interior loop of l1 unpaired letters on strand 1 and l2 on strand 2.
    on = "A": stem A ends on column `edge` of strand 1; on = "B": the shifted copy, stem B's first column is `edge`.
    tails: the poly-A runs behind stem B on strand 1, before rc(B) and behind rc(A) on strand 2 (none of them pairs)."""
    lead = edge - 8 if on == "A" else edge - 9 - l1
    assert lead >= 0
    s1 = "A" * lead + STEM_A + "A" * l1 + STEM_B + "A" * tails[0]
    s2 = "A" * tails[1] + rc(STEM_B) + "A" * l2 + rc(STEM_A) + "A" * tails[2]
    return s1, s2


def stem_letters(edge, l1, on="A"):
    """1-based letters of strand 1 in the middle of stem A and of stem B"""
    lead = edge - 8 if on == "A" else edge - 9 - l1
    return lead + 4, lead + 8 + l1 + 4


# model -> (edges, loop budget, [(loop at the budget or inside it)], [(loop at the budget, the same loop one letter longer)])
PLANT = {
    "contrafold": dict(edges=(58, 116), budget=28, loops=[(14, 14), (0, 28), (28, 0), (1, 27), (14, 15), (0, 29)],
                       jumps=[((14, 14), (14, 15)), ((0, 28), (0, 29))]),
    "vienna": dict(edges=(62, 124), budget=30, loops=[(15, 15), (0, 30), (30, 0), (1, 29), (3, 27), (15, 16), (0, 31)],
                   jumps=[((15, 15), (15, 16)), ((0, 30), (0, 31))]),
}


def planted_pairs(model):
    """[(what, s1, s2)]: every loop of the model at every edge, stem A's last column on the edge and stem B's first"""
    P = PLANT[model]
    return [("planted edge %d loop %dx%d stem %s" % (e, l1, l2, on),) + planted(e, l1, l2, on)
            for e in P["edges"] for l1, l2 in P["loops"] for on in "AB"]


def stem_row_sums(hp, edge, l1, on="A"):
    return [float(np.asarray(hp)[i].sum()) for i in stem_letters(edge, l1, on)]


def batch_pairs(model):
    """The batch of parts 2 - 4: the dummy, every edge shape, every planted pair; [(what, s1, s2)]"""
    rng = np.random.RandomState(300)
    out = [("dummy",) + (rnd(rng, DUMMY[0]), rnd(rng, DUMMY[1]))]
    out += [("edge shape %d x %d" % (len(a), len(b)), a, b) for a, b in edge_pairs(model)]
    return out + planted_pairs(model)
