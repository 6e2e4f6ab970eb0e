"""Tables that are reused without a clear.  The strips of the linear duplex sweep (dxl_strip8) keep each row of the tables correct
only on the band [alo-32, ahi+32] around the row's cells and leave whatever an earlier batch wrote beyond it; the other organisations
(dxl_sweep4, dxl_sweep<W>) rewrite every column and share the buffer.  Every GPU test here computes a sequence of batches on ONE
context and compares each batch, bit for bit over dense bp / up / hp / logZ, with the same batch on a freshly created context (whose
tables are all zero).  The CPU test pins the bound the band rests on: no kept cell reads a row farther than 30 columns from its cells."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ractip_amd.seqgen import random_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")
GS = 58          # columns a group of dxl_strip8 owns: group g has columns 58 g .. 58 g + 57
BAND = 32        # kDxBand


def alo_ahi(sd, L1, L2):
    return max(1, sd - L2), min(L1, sd - 1)


# ---- the batches: a long dummy pair keeps n1max / n2max (and so the table layout) fixed while the others shrink and shift
SHAPES = [(500, 500), (120, 480), (480, 120), (61, 59), (7, 300)]
# a second pair per batch whose stationary edge ahi = L1 is the last / first column of a group (115 = 2*58-1, 116 = 2*58, 173, 58, 57)
EDGE_SHAPES = [(115, 200), (116, 57), (173, 174), (58, 58), (57, 464)]


def shape_batches():
    dummy = random_pairs(1, 500, seed=77)[0]
    out = []
    for k, ((a, b), (c, d)) in enumerate(zip(SHAPES, EDGE_SHAPES)):
        out.append([dummy, random_pairs(1, a, b, seed=1000 + k)[0], random_pairs(1, c, d, seed=2000 + k)[0]])
    return out


def run_sequence(batches, fresh_each):
    """Results of every batch: on one context in turn, or each on a context of its own."""
    import ractip_amd
    out = []
    c = None
    try:
        for pairs in batches:
            if c is None or fresh_each:
                if c is not None:
                    c.close()
                c = ractip_amd.Context(device=0)
            c.batch_upload(pairs)
            c.batch_compute()
            out.append(([c.batch_results(p) for p in range(len(pairs))], [c.batch_fallbacks(w) for w in range(4)]))
    finally:
        if c is not None:
            c.close()
    return out


def assert_same_bits(got, want, what):
    assert len(got) == len(want)
    for b, ((res, fb), (res0, fb0)) in enumerate(zip(got, want)):
        assert fb == fb0, (what, b, fb, fb0)
        for p, (r, r0) in enumerate(zip(res, res0)):
            for k in KEYS:
                assert r[k].shape == r0[k].shape and r[k].tobytes() == r0[k].tobytes(), "%s: batch %d pair %d %s differs from the fresh context" % (what, b, p, k)


def test_shapes_put_live_edges_on_group_boundaries():
    """The sequence of shapes moves alo / ahi of the rows over the first and the last column of a 58-column group, as moving edges
    (ahi = sd-1, alo = sd-L2) and as stationary ones (ahi = L1)."""
    moving = set()
    for L1, L2 in SHAPES + EDGE_SHAPES:
        for sd in range(2, L1 + L2 + 1):
            lo, hi = alo_ahi(sd, L1, L2)
            moving.add(("lo", lo % GS)); moving.add(("hi", hi % GS))
    for edge in ("lo", "hi"):
        assert (edge, 0) in moving and (edge, GS - 1) in moving
    assert {L1 % GS for L1, _ in EDGE_SHAPES} >= {0, GS - 1}


@pytest.mark.gpu
def test_same_shape_other_content(hotlib):
    """Batch A, then batch B of the same lengths and other letters; A holds a G-rich strand against a C / U strand (G pairs with both),
    twice as many complementary cells as the random pair in its place in B: a cell B does not rewrite inside the live region would show."""
    rng = np.random.RandomState(3)
    g_rich = "".join(rng.choice(list("GGGU"), 100))
    cu = "".join(rng.choice(list("CU"), 100))
    A = [random_pairs(1, 300, 280, seed=11)[0], (g_rich, cu), random_pairs(1, 64, 190, seed=12)[0]]
    B = [random_pairs(1, 300, 280, seed=21)[0], random_pairs(1, 100, 100, seed=22)[0], random_pairs(1, 64, 190, seed=23)[0]]
    pairable = lambda s1, s2: sum((x + y) in ("AU", "UA", "CG", "GC", "GU", "UG") for x in s1 for y in s2)
    assert pairable(*A[1]) > 1.8 * pairable(*B[1])
    got = run_sequence([A, B], fresh_each=False)
    assert got[0][1] == [[], [], [], []], "batch A is meant to stay on the first pass"
    assert_same_bits(got[1:], run_sequence([B], fresh_each=True), "B after A")


@pytest.mark.gpu
def test_shrinking_and_shifting_shapes(hotlib):
    batches = shape_batches()
    assert all(max(len(p[0]) for p in b) == 500 and max(len(p[1]) for p in b) == 500 and len(b) == 3 for b in batches)   # one layout
    assert_same_bits(run_sequence(batches, fresh_each=False), run_sequence(batches, fresh_each=True), "shrinking / shifting shapes")


@pytest.mark.gpu
def test_after_an_overflow(hotlib):
    """The 700-nt GC helix of test_mixed_batch_only_the_flagged_problems_fall_back leaves the double range on the first pass (its
    tables hold Inf / NaN afterwards); the ordinary batch behind it equals the one of a fresh context."""
    pairs = random_pairs(6, 300, seed=4242)
    helix = "G" * 348 + "AAAA" + "C" * 348
    mixed = list(pairs)
    mixed[3] = (helix, pairs[3][1])
    got = run_sequence([mixed, pairs], fresh_each=False)
    assert got[0][1][2] == [6], "the helix is meant to be flagged"
    assert_same_bits(got[1:], run_sequence([pairs], fresh_each=True), "ordinary batch after an overflowed one")


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import test_gpu_stale_tables as T
batches = T.shape_batches()
one = T.run_sequence(batches, fresh_each=False)
T.assert_same_bits(one, T.run_sequence(batches, fresh_each=True), "organisation " + sys.argv[3])
np.savez(sys.argv[2], **{"%d/%d/%s" % (b, p, k): r[k] for b, (res, _) in enumerate(one) for p, r in enumerate(res) for k in T.KEYS})
"""
ORGS = {"strip8": {}, "sweep4": {"RH_DX_STRIP": "0"}, "sweep2": {"RH_DX_QUAD": "0", "RH_DX_W": "2"}}


@pytest.mark.gpu
def test_organisations_side_by_side(hotlib, tmp_path):
    """The organisation of the duplex sweep is read once, when the context is created: the shrinking / shifting sequence once per
    organisation, each in a process of its own with its switches set.  Each equals its own fresh contexts bit for bit (asserted in the
    child); strip8 stays within 1e-10 of the other two, the bar of test_sweep_organisations_agree."""
    out = {}
    for name, env in ORGS.items():
        e = dict(os.environ)
        for k in ("RH_DX_STRIP", "RH_DX_QUAD", "RH_DX_W"):
            e.pop(k, None)
        e.update(env)
        path = str(tmp_path / (name + ".npz"))
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, name], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, "%s: exit %d\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        out[name] = dict(np.load(path))
    from _oracle import assert_prob_close
    for name in ("sweep4", "sweep2"):
        assert out[name].keys() == out["strip8"].keys()
        for key, v in out["strip8"].items():
            if key.endswith("logZ"):
                assert np.allclose(v, out[name][key], rtol=0, atol=1e-10), (name, key)
            elif key.endswith("hp") or key.endswith("bp1") or key.endswith("bp2"):
                assert_prob_close(v, out[name][key], rel=1e-10, what="strip8 vs %s %s" % (name, key))


# ---- the band bound, from a model of the reads (duplex_lin.hip): a kept cell (sd, a) of direction dir (-1 inside, +1 outside) reads
# row sd + dir*(2+t), t = 0..28, at columns a + dir*(1..t+1) -- t <= 2 as single operands (dx_cell_loads / finish), t >= 3 as windows
def reads_of_row(sd, L1, L2, direction):
    """(row, lowest column, highest column) over the kept cells of row sd, one entry per source row, as arrays over the cells."""
    lo, hi = alo_ahi(sd, L1, L2)
    a = np.arange(lo, hi + 1)
    out = []
    for t in range(0, 29):
        r = sd + direction * (2 + t)
        if r < 2 or r > L1 + L2:
            continue
        cols = np.stack([a + direction * l for l in range(1, t + 2)])
        out.append((r, cols.min(axis=0), cols.max(axis=0)))
    return out


@pytest.mark.parametrize("L1,L2", [(61, 59), (7, 300), (300, 7), (120, 480), (480, 120), (1, 1), (1, 40), (33, 2), (200, 200)])
def test_every_read_of_a_kept_cell_lies_in_the_band(L1, L2):
    worst = 0
    for direction in (-1, 1):
        for sd in range(2, L1 + L2 + 1):
            for r, cmin, cmax in reads_of_row(sd, L1, L2, direction):
                rlo, rhi = alo_ahi(r, L1, L2)
                assert (cmin >= rlo - 30).all() and (cmax <= rhi + 30).all(), (direction, sd, r)
                worst = max(worst, int((rlo - cmin).max()), int((cmax - rhi).max()))
    assert worst <= 30 <= BAND


def strip8_groups(n1max, n2max, step):
    """dxl_strip8_groups (batch.h)."""
    cnt = min(n1max, n2max, 8 * step + 8, max(1, n1max + n2max - 8 * step - 1))
    return min((n1max + 2 + GS - 1) // GS, (cnt + 7 + 2 * BAND - 1) // GS + 2)


@pytest.mark.parametrize("n1max,n2max", [(500, 500), (61, 59), (7, 300), (300, 7), (480, 120), (1, 1), (130, 700)])
def test_the_strip_grid_covers_every_band(n1max, n2max):
    """The grid of launch `step` is sized from the batch shape alone; the kernel counts its groups from the first one that meets the
    band of the pair's own rows.  Every group that meets a band of any pair no longer than the shape is inside that grid."""
    rng = np.random.RandomState(n1max + n2max)
    shapes = {(n1max, n2max), (1, 1), (1, n2max), (n1max, 1)} | {(rng.randint(1, n1max + 1), rng.randint(1, n2max + 1)) for _ in range(12)}
    all_groups = (n1max + 2 + GS - 1) // GS
    for L1, L2 in shapes:
        smax = L1 + L2
        for step in range((n1max + n2max - 2) // 8 + 1):
            for outside in (False, True):
                sdA = smax - 8 * step if outside else 2 + 8 * step
                rows = [sd for sd in (range(sdA - 7, sdA + 1) if outside else range(sdA, sdA + 8)) if 2 <= sd <= smax]
                if (sdA < 2) if outside else (sdA > smax):
                    continue
                lo = alo_ahi(rows[0], L1, L2)[0]
                first = max(0, lo - BAND) // GS
                need = set()
                for sd in rows:
                    blo, bhi = alo_ahi(sd, L1, L2)
                    need.update((max(0, blo - BAND) // GS, min(n1max + 1, bhi + BAND) // GS))
                assert min(need) >= first and max(need) < min(all_groups, first + strip8_groups(n1max, n2max, step)), (L1, L2, step, outside)
