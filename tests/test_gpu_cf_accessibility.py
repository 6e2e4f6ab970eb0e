"""GPU suite: region accessibility up[i][w] of the CONTRAfold model (rh_set_region_accessibility), against the pinned oracle
through clone parameter files (tests/_cf_clone.py): up[i][w] = exp(logZ_clone(s recoded on i..i+w) - logZ(s)).

The context under test runs on the BUNDLED parameters; only the oracle loads clone files.  Comparison: assert_prob_close at the
project's rel = 1e-6 with the abs_floor = 1e-11 of the Vienna-BL `up` tests -- every term is a sum of positive products, so there
is no cancellation to excuse.  Lengths: 1, 2, 5 (no loop fits), 12, 33 (below kStripMinN = 40), 40 / 41 (first strips), 64 / 65
(one / two 64-column groups and chain tiles), 130, 400 (block products from n = 384); loop budget 30 in the planted cases."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot, ilp, pipeline
from _cf_clone import FAMILIES, CloneOracle, random_seq, region_up
from _oracle import assert_prob_close

pytestmark = pytest.mark.gpu

REL, FLOOR = 1e-6, 1e-11
MAX_W = 15
PATH_OF_MODE = {hot.RH_MODE_AUTO: 1, hot.RH_MODE_LOG: 2, hot.RH_MODE_LINEAR: 1}   # rh_last_path of sequences that stay in range


@pytest.fixture(scope="module")
def clones(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cf_clone")
    return {name: CloneOracle(name, tmp) for name in FAMILIES}


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(max_workers=16) as p:
        yield p


@pytest.fixture(scope="module")
def acc(hotlib):
    c = ractip_amd.Context(device=0)
    c.set_region_accessibility(True)
    yield c
    c.close()


_REF = {}


def reference(pool, co, seq, entries):
    """oracle values of the entries (i, w), computed once per (family, sequence, entry)"""
    co.logz(seq)   # (memoised before the threads ask for it)
    missing = [e for e in entries if (co.family.name, seq, e) not in _REF]
    for e, v in zip(missing, pool.map(lambda e: region_up(co, seq, e[0], e[1]), missing)):
        _REF[(co.family.name, seq, e)] = v
    return np.array([_REF[(co.family.name, seq, e)] for e in entries])


def every(n, max_w):
    return [(i, w) for i in range(n) for w in range(max_w) if i + w < n]


def sampled(n, max_w, count, seed):
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < count:
        w = int(rng.integers(0, max_w))
        out.add((int(rng.integers(0, n - w)), w))
    return sorted(out)


def check(ctx, pool, co, seq, max_w, entries, mode=hot.RH_MODE_AUTO, what=""):
    ctx.set_mode(mode)
    ctx.set_max_w(max_w)
    _, up, _ = ctx.fold(seq)
    assert ctx.last_path() == PATH_OF_MODE[mode], what
    up = np.asarray(up).reshape(len(seq), max_w)
    got = np.array([up[i, w] for i, w in entries])
    want = reference(pool, co, seq, entries)
    assert_prob_close(got, want, rel=REL, abs_floor=FLOOR, what="%s n=%d max_w=%d" % (what, len(seq), max_w))
    past = [(i, w) for i in range(len(seq)) for w in range(max_w) if i + w >= len(seq)]
    assert all(up[i, w] == 0.0 for i, w in past), "entries past the end hold 0, as on the Vienna-BL path"
    return up


def seq_of(fam, n):
    return random_seq(np.random.default_rng(1000 + n + 7 * len(fam)), n, FAMILIES[fam].alphabet)


@pytest.mark.parametrize("fam", ["AU", "CG"])
@pytest.mark.parametrize("n", [1, 2, 5, 12, 33, 40, 41, 64, 65])
def test_every_region_of_short_sequences(acc, clones, pool, fam, n):
    seq = seq_of(fam, n)
    check(acc, pool, clones[fam], seq, MAX_W, every(n, MAX_W), what=fam)


@pytest.mark.parametrize("fam", ["AU", "CG"])
@pytest.mark.parametrize("n,count", [(130, 60), (400, 24)])
def test_sampled_regions_of_long_sequences(acc, clones, pool, fam, n, count):
    """n = 400: two-level block products (from 384), seven chain tiles per axis; logZ of the {C,G} sequence is near 230."""
    seq = seq_of(fam, n)
    check(acc, pool, clones[fam], seq, MAX_W, sampled(n, MAX_W, count, seed=n), what=fam)


@pytest.mark.parametrize("mode", [hot.RH_MODE_LOG, hot.RH_MODE_LINEAR], ids=["log", "linear"])
@pytest.mark.parametrize("fam", ["AU", "CG"])
@pytest.mark.parametrize("n", [33, 65, 130])
def test_the_same_sets_on_the_log_space_and_the_linear_path(acc, clones, pool, fam, n, mode):
    seq = seq_of(fam, n)
    entries = every(n, MAX_W) if n < 130 else sampled(n, MAX_W, 60, seed=n)
    check(acc, pool, clones[fam], seq, MAX_W, entries, mode=mode, what=fam)


def comp(s):
    return "".join({"G": "C", "C": "G", "A": "U", "U": "A"}[c] for c in reversed(s))


def test_planted_hairpin_with_a_loop_of_forty(acc, clones, pool):
    """the length score of a hairpin is constant above 30: the suffix sums must not stop there"""
    stem = "GCGGCGGC"
    seq = stem + "G" * 40 + comp(stem)
    up = check(acc, pool, clones["CG"], seq, MAX_W, every(len(seq), MAX_W), what="hairpin 40")
    assert up[len(stem) + 5, MAX_W - 1] > 0.5, "the loop is the dominant structure"


@pytest.mark.parametrize("side", [29, 30, 31])
def test_planted_interior_loop_sides_at_the_loop_budget(acc, clones, pool, side):
    """one side of `side` unpaired letters (a bulge when the other side is empty): the single-branch term exists up to 30 letters and
    not beyond; widths up to 32 reach past the budget"""
    inner = "GCGGC" + "GGGG" + "GCCGC"
    seq = "GCGGCGC" + "G" * side + inner + "GCGCCGC"
    i0, max_w = 7, 32
    entries = [(i, w) for i in range(i0 - 1, i0 + side) for w in (1, 7, 14, 27, 28, 29, 30, 31) if i + w < len(seq)]
    check(acc, pool, clones["CG"], seq, max_w, entries, what="interior side %d" % side)


def test_max_w_64(acc, clones, pool):
    seq = seq_of("AU", 70)
    entries = [(i, w) for i in (0, 3, 31) for w in range(64) if i + w < 70] + sampled(70, 64, 40, seed=64)
    check(acc, pool, clones["AU"], seq, 64, sorted(set(entries)), what="max_w 64")


def planted_multiloop(branches):
    """an 8-pair helix closing `branches` hairpins of 8 pairs, one G between them and SIX trailing letters before the closing pair;
    returns the sequence, the letters of the helices without their (fraying) end pairs, and the trailing run"""
    lefts = ["GCGCGGCG", "GGCCGCGG", "GCCGGCCG", "GGGCGCCG", "GCGGCCGG"]
    k = 8
    seq, stems = lefts[-1], list(range(1, k - 1))
    for b in lefts[:branches]:
        seq += "G"
        s0 = len(seq)
        seq += b + "GGGG" + comp(b)
        stems += list(range(s0 + 1, s0 + k - 1)) + list(range(s0 + k + 5, s0 + 2 * k + 3))
    t0 = len(seq)
    seq += "GGGGGG"
    s0 = len(seq)
    seq += comp(lefts[-1])
    stems += list(range(s0 + 1, s0 + k - 1))
    return seq, stems, list(range(t0, t0 + 6))


@pytest.mark.parametrize("branches", [3, 4])
def test_planted_multiloop_with_trailing_letters_pins_the_derivation_count(acc, clones, pool, branches):
    """Trailing letters of a multiloop can be shed at every level of FM's right recursion: Z counts C(t + m - 1, m - 1) derivations
    for t trailing letters behind m branches, and so does the oracle's ratio.  A single FMo x mu^len x FM product fails here."""
    seq, stems, trail = planted_multiloop(branches)
    co = clones["CG"]
    rows = co.pair_rows(seq)
    assert min(rows[i] for i in stems) > 0.9, "the planted helices hold: the multiloop dominates the ensemble"
    entries = [(i, w) for i in trail for w in range(6) if i + w <= trail[-1]]
    entries += [(i, w) for i in range(trail[0] - 3, trail[-1] + 2) for w in (0, 1, 6, 10) if i + w < len(seq)]
    up = check(acc, pool, co, seq, MAX_W, sorted(set(entries)), what="multiloop %d" % branches)
    assert up[trail[0], 5] > 0.5, "the whole trailing run is unpaired in most of the ensemble"


def test_planted_a_runs_next_to_gu_pairs(acc, clones, pool):
    """{A,U,G} with runs of sixteen A: the clone has C -> A only, regions lie inside the runs; G.U pairs are in the ensemble"""
    rng = np.random.default_rng(77)
    parts = [random_seq(rng, 14, "UGAUG"), "A" * 16, random_seq(rng, 17, "UGGAU"), "A" * 16, random_seq(rng, 12, "GUUAG")]
    seq = "".join(parts)
    runs = [len(parts[0]), len("".join(parts[:3]))]
    entries = [(r + i, w) for r in runs for i in range(16) for w in range(MAX_W) if i + w < 16]
    check(acc, pool, clones["AUG"], seq, MAX_W, entries, what="A runs")


def test_a_sequence_held_by_another_scale_exponent_agrees_with_the_log_space_path(acc):
    """A perfect GC helix of 700 letters leaves the double range at the default exponent and is recomputed, as a sub-batch of one, on
    the next rung of the ladder: its regions' ratios must not depend on the exponent.  Reference: the same context on the log-space
    kernels (pinned to the oracle above, up to n = 130; one oracle call at n = 700 takes ten seconds), both in double: rel 1e-6."""
    helix = "G" * 348 + "GGGG" + "C" * 348
    pairs = [(helix, seq_of("CG", 33))]
    acc.set_max_w(MAX_W)
    ups = {}
    for mode, path in ((hot.RH_MODE_AUTO, 3), (hot.RH_MODE_LOG, 2)):
        acc.set_mode(mode)
        acc.batch_upload(pairs)
        acc.batch_compute()
        assert acc.last_path() == path
        if mode == hot.RH_MODE_AUTO:
            assert acc.batch_fallbacks(2) == [0] and acc.batch_fallbacks(0) == [], "held by another exponent, not by the log-space kernels"
        r = acc.batch_results(0)
        ups[mode] = (r["up1"], r["up2"])
    acc.set_mode(hot.RH_MODE_AUTO)
    for k in range(2):
        assert ups[hot.RH_MODE_AUTO][k].shape == (len(pairs[0][k]), MAX_W)
        assert_prob_close(ups[hot.RH_MODE_AUTO][k], ups[hot.RH_MODE_LOG][k], rel=REL, abs_floor=FLOOR, what="ladder against log space, sequence %d" % k)
    loop = ups[hot.RH_MODE_AUTO][0][348, 3]
    assert loop > 0.5, "the hairpin loop of the helix is open"


def test_ragged_indexed_batch_fetches_agree_and_the_rest_keeps_its_bits(acc, hotlib):
    """lengths 5 .. 130, sequence 2 in both roles: dense, per-pair and packed fetches agree; candidate lists of up equal a host
    threshold of the dense table; column 0 is the max_w = 1 run's; bp, hp and log Z do not depend on the option"""
    rng = np.random.default_rng(5)
    seqs = [random_seq(rng, n, "ACGU") for n in (5, 130, 41, 64, 12, 33)]
    index = [(0, 2), (2, 1), (3, 2), (4, 5), (2, 2)]
    acc.set_mode(hot.RH_MODE_AUTO)
    acc.set_max_w(MAX_W)
    acc.batch_upload_indexed(seqs, index)
    acc.batch_compute()
    assert acc.last_path() == 1
    assert acc.batch_acc_time() > 0.0
    dense = acc.batch_results_all()
    for k, s in enumerate(seqs):
        assert dense["up"][k].shape == (len(s), MAX_W)
        assert (np.diff(dense["up"][k], axis=1) <= 1e-9).all(), "wider regions are not more accessible"
    for p, (a, b) in enumerate(index):
        one = acc.batch_results(p)
        assert np.array_equal(one["up1"], dense["up"][a]) and np.array_equal(one["up2"], dense["up"][b])
    packed = acc.batch_results_packed_f32()
    for k in range(len(seqs)):
        assert np.array_equal(packed["up"][k].view(np.uint32), dense["up"][k].astype(np.float32).view(np.uint32)), "(float) bits"
    for b in packed["bufs"]:
        acc.pinned_free(b)
    th = 0.25
    for which in (3, 4):
        rec, first = acc.batch_candidates_all(which, th)
        for p, pr in enumerate(index):
            u = dense["up"][pr[which - 3]].astype(np.float32).ravel()
            hit = np.flatnonzero(u > np.float32(th))
            mine = rec[first[p]:first[p + 1]]
            assert np.array_equal(mine["i"] * MAX_W + mine["j"], hit) and np.array_equal(mine["p"], u[hit]), "which=%d pair %d" % (which, p)
    # the option off (max_w = 1) on a fresh default context: column 0, bp, hp and log Z bit for bit
    plain = ractip_amd.Context(device=0)
    try:
        plain.batch_upload_indexed(seqs, index)
        plain.batch_compute()
        base = plain.batch_results_all()
    finally:
        plain.close()
    for k in range(len(seqs)):
        assert np.array_equal(dense["up"][k][:, 0], base["up"][k]), "column 0 of sequence %d" % k
        assert np.array_equal(dense["bp"][k], base["bp"][k])
    for p in range(len(index)):
        assert np.array_equal(dense["hp"][p], base["hp"][p])
    assert np.array_equal(dense["logZ"], base["logZ"])


def test_off_by_default_and_nothing_for_vienna_bl(hotlib):
    c = ractip_amd.Context(device=0)
    try:
        assert not c.region_accessibility
        with pytest.raises(hot.RhError):
            c.set_max_w(5)
        with pytest.raises(hot.RhError):
            c.unpaired("ACGUACGUAC", max_w=5)
        c.set_region_accessibility(True)
        assert c.region_accessibility and c.unpaired("ACGUACGUAC", max_w=5).shape == (10, 5)
        c.set_region_accessibility(False)
        assert c.max_w == 1
        with pytest.raises(hot.RhError):
            c.set_max_w(5)
    finally:
        c.close()
    seq = random_seq(np.random.default_rng(3), 50, "ACGU")
    v = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    try:
        before = v.fold(seq)
        v.set_region_accessibility(True)
        after = v.fold(seq)
        assert not v.region_accessibility and v.max_w == 15
        assert all(np.array_equal(x, y) for x, y in zip(before[:2], after[:2])) and before[2] == after[2]
    finally:
        v.close()


def test_pipeline_predict_hands_the_widths_to_the_ilp(hotlib, monkeypatch):
    rng = np.random.default_rng(11)
    s1, s2 = random_seq(rng, 40, "ACGU"), random_seq(rng, 35, "ACGU")
    seen = []
    solve = ilp.solve

    def spy(*args, **kw):
        seen.append((args, kw))
        return solve(*args, **kw)

    monkeypatch.setattr(ilp, "solve", spy)
    opt = ilp.Options()
    out = pipeline.predict(s1, s2, model="contrafold", accessibility=True, options=opt)
    assert len(out[0]) == len(s1) and len(out[1]) == len(s2)
    ups = [a for a in list(seen[-1][0]) + list(seen[-1][1].values()) if isinstance(a, np.ndarray) and a.ndim == 2 and a.shape[1] == opt.max_w]
    assert [u.shape for u in ups] == [(len(s1), opt.max_w), (len(s2), opt.max_w)], "up1, up2 reach ilp.solve with every width"
    seen.clear()
    pipeline.predict(s1, s2, model="contrafold")
    assert not [a for a in list(seen[-1][0]) + list(seen[-1][1].values()) if isinstance(a, np.ndarray) and a.ndim == 2 and a.shape[1] == opt.max_w]
