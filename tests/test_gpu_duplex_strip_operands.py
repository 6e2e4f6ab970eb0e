"""dxl_strip8 takes the short-loop operands of its first four diagonals from the staged window rows and every cell's weights from the
fused, pair-indexed tables (DxLinModel::F, lin_model.h) in LDS.  Three small batches, each built for one of the places where that can
go wrong, each checked on the CPU alone first (the tests without the gpu mark assert the property the batch is built for, on
oracle/cf_oracle.c and on the sequences themselves):

  1. SHORT_LOOPS: two 8-bp GC stems (planted() of test_gpu_duplex_edges.py) joined by each loop with l1 + l2 <= 2, the stems shifted
     by s = 0..7 letters along strand 1 at constant length.  The pair that closes the loop then sits on every row k = 0..7 of a strip,
     in both directions: for k < 2 (stacked pair), k < 3 (0x1, 1x0) or k < 4 (0x2, 1x1, 2x0) its operand lies on a row of an earlier
     launch (the global load of the raw table, or the staged rows), otherwise on the strip's own rows.
  2. ALL_INDICES: seeded random sequences over A, C, G, U and N whose pairable cells reach every entry of the fused tables, as own entry
     (pair type, xm, yp) and as decorating entry (pair type, xp, ym), with the sentinels of positions 0 and L+1 in every combination
     a strand end allows.
  3. TINY: tables of 1 to 17 rows, alone and behind a (64, 64) first pair: the first strip of either direction has no row before it
     (the staged rows r = 1..4 are absent), the last strip is partial, and at (9, 9) a second strip takes all four from the first.

References: oracle/cf_oracle.c at the project's bars (1e-6 relative on hp above 1e-12, 1e-9 on log Z), and the dxl_sweep4 organisation
(RH_DX_STRIP=0: dx_cell_ops, the plain tables, global loads) of the same batch at 1e-10.  Every GPU test asserts the path
(rh_last_hybrid_path), the absence of fallbacks and the kernel name of what it compares."""
import numpy as np
import pytest

from _oracle import OraclePool, assert_prob_close
from test_gpu_duplex_edges import STEM_A, STEM_B, assert_ran, cf_context, planted, stem_letters

REL = 1e-6
LOOPS = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]
LEADS = range(8)
TAILS = (27, 20, 10)          # behind stem B on strand 1 (minus the lead: the length stays), before rc(B) and behind rc(A) on strand 2
ORGS = [({}, "dxl_strip8"), ({"RH_DX_STRIP": "0"}, "dxl_sweep4")]


# ---- 1. short loops on every strip row
def short_loop_pair(s, l1, l2):
    return planted(s + 8, l1, l2, tails=(TAILS[0] - s, TAILS[1], TAILS[2]))


def short_loop_pairs():
    return [("loop %dx%d lead %d" % (l1, l2, s),) + short_loop_pair(s, l1, l2) for l1, l2 in LOOPS for s in LEADS]


def closing_cells(s, l1, l2):
    """(sd of the cell that takes the loop inside, sd of the cell that takes it outside, L1, L2); a = i, b = L2 + 1 - j, sd = a + b.
    Inside, the first pair of stem B reads the last pair of stem A (rows before it); outside, the last pair of stem A reads the first
    pair of stem B."""
    s1, s2 = short_loop_pair(s, l1, l2)
    L1, L2 = len(s1), len(s2)
    i_a, j_a = s + 8, TAILS[1] + 8 + l2 + 1            # last pair of stem A
    i_b, j_b = s + 8 + l1 + 1, TAILS[1] + 8            # first pair of stem B
    assert s1[i_a - 1] + s2[j_a - 1] == STEM_A[-1] + "G" and s1[i_b - 1] + s2[j_b - 1] == STEM_B[0] + "C"
    assert (i_b - i_a - 1, j_a - j_b - 1) == (l1, l2)
    return i_b + (L2 + 1 - j_b), i_a + (L2 + 1 - j_a), L1, L2


# ---- 2. every index of the fused tables
PAIR_TYPES = ["AU", "CG", "GC", "GU", "UA", "UG"]       # in the order of the bit x*5 + y of the pair mask (dx_pair_type)
SENT = 5                                                # positions 0 and L+1 (the kernels read code 4 there, like N)
ALL_SEED, ALL_PAIRS = 7, 24


def all_index_pairs():
    """Random over ACGUN, 40 - 70 letters; pair k < 6 has the letters of pair type k at both strand ends (first letter of strand 1 with the
    last of strand 2 and the other way round), so that a cell with both neighbours beyond the strands exists for every pair type."""
    rng = np.random.RandomState(ALL_SEED)
    out = []
    for k in range(ALL_PAIRS):
        a = list(rng.choice(list("ACGUN"), rng.randint(40, 71)))
        b = list(rng.choice(list("ACGUN"), rng.randint(40, 71)))
        if k < 6:
            a[0] = a[-1] = PAIR_TYPES[k][0]
            b[0] = b[-1] = PAIR_TYPES[k][1]
        out.append(("random ACGUN %d" % k, "".join(a), "".join(b)))
    return out


def fused_entries(pairs):
    """The entries the pairable cells of `pairs` index: {(type, xm, yp)}, {(type, xp, ym)}, neighbour codes 0..4 and SENT"""
    own, dec = set(), set()
    for _, s1, s2 in pairs:
        c1 = [SENT] + ["ACGUN".index(ch) for ch in s1] + [SENT]
        c2 = [SENT] + ["ACGUN".index(ch) for ch in s2] + [SENT]
        for i in range(1, len(s1) + 1):
            for j in range(1, len(s2) + 1):
                xy = s1[i - 1] + s2[j - 1]
                if xy in PAIR_TYPES:
                    t = PAIR_TYPES.index(xy)
                    own.add((t, c1[i - 1], c2[j + 1]))
                    dec.add((t, c1[i + 1], c2[j - 1]))
    return own, dec


# ---- 3. source rows that do not exist
TINY = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (4, 5), (8, 1), (1, 8), (9, 9)]
FIRST = (64, 64)


def tiny_pairs():
    """Letters over G and C (every second cell pairs: a table of one cell is still a pair); the first pair is random ACGU"""
    rng = np.random.RandomState(88)
    out = [("first %d x %d" % FIRST, "".join(rng.choice(list("ACGU"), FIRST[0])), "".join(rng.choice(list("ACGU"), FIRST[1])))]
    for a, b in TINY:
        s1 = "".join(rng.choice(list("GC"), a))
        s2 = "".join({"G": "C", "C": "G"}[ch] for ch in reversed((s1 * b)[:b]))      # strand 2 pairs with strand 1 letter by letter
        out.append(("tiny %d x %d" % (a, b), s1, s2))
    return out


BATCHES = {"short_loops": short_loop_pairs, "all_indices": all_index_pairs, "tiny": tiny_pairs}


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    for make in BATCHES.values():
        for _, s1, s2 in make():
            p.duplex(s1, s2)
    yield p
    p.close()


def test_short_loops_put_the_closing_pair_on_every_strip_row_and_hold_the_stems(opool):
    """Over the eight leads the closing pair's strip row, (sd - 2) % 8 inside and (L1 + L2 - sd) % 8 outside, takes every value 0..7 for
    every loop; the oracle's row sums of hp over the mid-stem letters of both stems exceed 0.9, so a wrong or missing short-loop operand
    moves hp by tens of percent."""
    pairs = short_loop_pairs()
    assert len(pairs) == 48 and all(40 <= len(s1) <= 50 and 40 <= len(s2) <= 50 for _, s1, s2 in pairs)
    for l1, l2 in LOOPS:
        cells = [closing_cells(s, l1, l2) for s in LEADS]
        assert {(sd_in - 2) % 8 for sd_in, _, _, _ in cells} == set(range(8)), (l1, l2)
        assert {(L1 + L2 - sd_out) % 8 for _, sd_out, L1, L2 in cells} == set(range(8)), (l1, l2)
        for s in LEADS:
            s1, s2 = short_loop_pair(s, l1, l2)
            hp = np.asarray(opool.duplex(s1, s2).result()["post"])
            rows = [float(hp[i].sum()) for i in stem_letters(s + 8, l1)]
            assert min(rows) > 0.9, (l1, l2, s, rows)


def test_random_batch_reaches_every_entry_of_the_fused_tables():
    """(pair type, xm, yp) and (pair type, xp, ym) over the pairable cells: all 6 x 5 x 5 letter combinations each, and the sentinel of a
    strand end with every letter and with the other sentinel (6 x 11 each)"""
    pairs = all_index_pairs()
    assert all(40 <= len(s1) <= 70 and 40 <= len(s2) <= 70 for _, s1, s2 in pairs)
    own, dec = fused_entries(pairs)
    letters = {(t, n1, n2) for t in range(6) for n1 in range(5) for n2 in range(5)}
    ends = {(t, n1, n2) for t in range(6) for n1 in range(6) for n2 in range(6) if SENT in (n1, n2)}
    assert len(letters) == 150 and len(ends) == 66
    for name, got in (("own", own), ("decorating", dec)):
        assert letters <= got, (name, sorted(letters - got))
        assert ends <= got, (name, sorted(ends - got))


def test_tiny_tables_are_partial_full_and_chained_strips_and_every_one_has_a_pair(opool):
    """L1 + L2 - 1 rows: 1, 2, 3, 5 (one partial strip), 8 (one full strip, three shapes), 17 (two full strips and a row); the oracle finds
    a structure in every one (log Z is not the -2e20 of a pair without complementary letters)"""
    assert sorted({a + b - 1 for a, b in TINY}) == [1, 2, 3, 5, 8, 17]
    assert {(1, 8), (8, 1), (4, 5)} <= set(TINY) and all(a <= FIRST[0] and b <= FIRST[1] for a, b in TINY)
    for what, s1, s2 in tiny_pairs()[1:]:
        o = opool.duplex(s1, s2).result()
        assert o["logZ2"][0] > -1e18 and np.asarray(o["post"]).max() > 0, what


# ---- the GPU side
def run(c, pairs, kernel, alone):
    seqs = [(s1, s2) for _, s1, s2 in pairs]
    c.batch_upload(seqs)
    c.batch_compute()
    assert_ran(c, 1, kernel, "batch")
    out = dict(res=[c.batch_results(p) for p in range(len(seqs))], alone=[])
    if alone:
        for what, s1, s2 in pairs[1:]:
            out["alone"].append(c.duplex(s1, s2))
            assert_ran(c, 1, kernel, "alone: " + what)
    return out


@pytest.fixture(scope="module")
def runs(hotlib):
    """{batch: {kernel: results}}: every batch on the default organisation (dxl_strip8) and on dxl_sweep4, computed once"""
    out = {name: {} for name in BATCHES}
    for env, kernel in ORGS:
        c = cf_context(0, env)
        try:
            for name, make in BATCHES.items():
                out[name][kernel] = run(c, make(), kernel, alone=(name == "tiny"))
        finally:
            c.close()
    return out


def against_oracle(opool, what, s1, s2, hp, logz):
    o = opool.duplex(s1, s2).result()
    assert abs(logz - o["logZ2"][0]) < 1e-9, (what, logz, o["logZ2"][0])
    assert_prob_close(hp, o["post"], rel=REL, what="hp " + what)
    big = o["post"] > 1e-12
    return float((np.abs(hp - o["post"])[big] / o["post"][big]).max()) if big.any() else 0.0


def against_sweep4(what, hp, logz, hp4, logz4):
    assert abs(logz - logz4) <= 1e-10, (what, logz, logz4)
    assert_prob_close(hp, hp4, rel=1e-10, what="hp dxl_strip8 vs dxl_sweep4: " + what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_strip_operands_vs_oracle_and_sweep4(opool, runs, name):
    """dxl_strip8 (rh_last_hybrid_path = 1, no fallback) on the batch: hp and log Z == oracle/cf_oracle.c at 1e-6 / 1e-9 and == the
    dxl_sweep4 organisation at 1e-10; for the tiny tables also each pair alone (n1max = L1) on both organisations.  Batch 1
    additionally: the kernel's own row sums over the mid-stem letters exceed 0.9."""
    pairs = BATCHES[name]()
    strip, quad = runs[name]["dxl_strip8"], runs[name]["dxl_sweep4"]
    worst = 0.0
    for (what, s1, s2), r, r4 in zip(pairs, strip["res"], quad["res"]):
        worst = max(worst, against_oracle(opool, what, s1, s2, r["hp"], r["logZ"][2]))
        against_oracle(opool, "dxl_sweep4 " + what, s1, s2, r4["hp"], r4["logZ"][2])
        against_sweep4(what, r["hp"], r["logZ"][2], r4["hp"], r4["logZ"][2])
    print("%s: largest relative error of hp over %d pairs %.3g" % (name, len(pairs), worst))
    if name == "tiny":
        assert len(strip["alone"]) == len(quad["alone"]) == len(TINY)
        for (what, s1, s2), (hp, z), (hp4, z4) in zip(pairs[1:], strip["alone"], quad["alone"]):
            against_oracle(opool, "alone " + what, s1, s2, hp, z)
            against_sweep4("alone " + what, hp, z, hp4, z4)
    if name == "short_loops":
        for (l1, l2), s in ((lp, s) for lp in LOOPS for s in LEADS):
            r = strip["res"][LOOPS.index((l1, l2)) * len(LEADS) + s]
            rows = [float(np.asarray(r["hp"])[i].sum()) for i in stem_letters(s + 8, l1)]
            assert min(rows) > 0.9, (l1, l2, s, rows)
