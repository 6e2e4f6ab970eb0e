"""16-tile block products with one wavefront per tile (lin_far_inside_pk / lin_far_outside_pk, four accumulators summed in the order
the four wavefronts of the split-K form are summed) on packed tiles in the two-halves fragment order (ractip_amd/csrc/pk_layout.h):
the same BYTES as the split-K form (RH_FAR_WAVE=0: lin_far_*_pk4) and, without strips, as the products on gathered tiles.

  * batch 1: 66, 81, 97, 113, 145, 177, 209, 241 letters as four pairs.  66 is the shortest length with any product; the tiles have 1 to
    12 K steps, so every accumulator gets 0, 1, 2 and 3 steps and the loop of four meets every remainder; with batch 2 the block
    diagonals have 1..19 tiles, so both ragged and full groups of four wavefronts;
  * batch 2: 257, 273, 305, 330 letters under RH_FAR2=1, the two-level form: the inside read-modify-write needs J2 - I2 >= 4, hence
    n >= 257, the outside ones I2 >= 2 and 4 (J2 + 2) <= last block, both met from about 130 letters;
  * batch 3: batch 1 plus sixteen fillers of 60..71 letters: 24 sequences, a multiple of 8 (XCD-pinned grids), against 8 + 0;
    the first four pairs have the bytes of batch 1;
  * packed against gathered: under RH_STRIP=0, RH_FAR2=0 the products on packed tiles and RH_FAR_PK=0 (lin_far_*_mfma gathers each
    tile from the tables) have the same operands, split, MFMA order and final sum, so the fragment order is pinned to the tables;
  * Vienna-BL: one two-molecule batch (70 + 75 and 90 + 60 letters), whose joint sweeps drop the one-strand tiles per wavefront.
  * the suite's two shared contexts (conftest.py: ctx), after whatever earlier tests ran on them: the folds of the first pair.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENS1 = [66, 81, 97, 113, 145, 177, 209, 241]
LENS2 = [257, 273, 305, 330]
FILL = [60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 60, 65, 66, 71]
VIENNA = [(70, 75), (90, 60)]
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")
WAVE = ("lin_far_inside_pk", "lin_far_outside_pk")
SPLITK = ("lin_far_inside_pk4", "lin_far_outside_pk4")
GATHER = ("lin_far_inside_mfma", "lin_far_outside_mfma")
NO_STRIPS = {"RH_STRIP": "0", "RH_FAR2": "0"}


def rnd(rng, n):
    return "".join("ACGU"[k] for k in rng.randint(0, 4, n))


def batches():
    """name -> pairs (CONTRAfold model); 3 = 1 + fillers"""
    rng = np.random.RandomState(977)
    s1, s2, fill = [rnd(rng, n) for n in LENS1], [rnd(rng, n) for n in LENS2], [rnd(rng, n) for n in FILL]
    pair_up = lambda s: [(s[q], s[q + 1]) for q in range(0, len(s), 2)]
    out = {1: pair_up(s1), 2: pair_up(s2), 3: pair_up(s1 + fill)}
    assert 2 * len(out[1]) % 8 == 0 and 2 * len(out[3]) == 24
    out["vienna"] = [(rnd(rng, a), rnd(rng, b)) for a, b in VIENNA]
    return out


def compute(env, pairs, vienna=False):
    """Results of one batch on a context created under `env`"""
    import ractip_amd
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL) if vienna else ractip_amd.Context(device=0)
    finally:
        mp.undo()
    try:
        if vienna:
            c.set_hybrid(True)   # hp of the two-molecule ensemble: joint sweeps over s1 + s2
        c.batch_upload(pairs)
        c.batch_compute()
        assert c.last_path() == 1 and c.batch_fallbacks(0) == [] and c.batch_fallbacks(2) == [], (env, c.last_path())
        return dict(res=[c.batch_results(p) for p in range(len(pairs))], kernels=c.batch_kernels(), launches=tuple(c.batch_timings()[1]))
    finally:
        c.close()


@pytest.fixture(scope="module")
def runs(hotlib):
    """Every GPU result of this file, computed once"""
    b = batches()
    out = {}
    for form, env in (("wave", {}), ("splitk", {"RH_FAR_WAVE": "0"})):
        out[form, 1] = compute(env, b[1])
        out[form, 2] = compute(dict(env, RH_FAR2="1"), b[2])
        out[form, "vienna"] = compute(env, b["vienna"], vienna=True)
    out["wave", 3] = compute({}, b[3])
    out["packed", 1] = compute(NO_STRIPS, b[1])
    out["gathered", 1] = compute(dict(NO_STRIPS, RH_FAR_PK="0"), b[1])
    return out


def assert_same_bytes(a, b, what):
    assert len(a) == len(b)
    for p, (r, r0) in enumerate(zip(a, b)):
        for key in KEYS:
            assert r[key].tobytes() == r0[key].tobytes(), (what, p, key)


def far_names(run):
    return run["kernels"][0][1], run["kernels"][1][1]


@pytest.mark.parametrize("batch", [1, 2], ids=["one_level", "two_level"])
def test_wave_form_same_bytes_as_split_k(runs, batch):
    a, b = runs["wave", batch], runs["splitk", batch]
    assert far_names(a) == WAVE and far_names(b) == SPLITK, (a["kernels"], b["kernels"])
    # the reports differ in the block-product name only
    assert [(k[0], k[2]) for k in a["kernels"]] == [(k[0], k[2]) for k in b["kernels"]] and a["kernels"][2] == b["kernels"][2], (a["kernels"], b["kernels"])
    assert a["launches"] == b["launches"] and a["kernels"][0][2] > 0 and a["kernels"][1][2] > 0, (a["launches"], b["launches"], a["kernels"])
    assert_same_bytes(a["res"], b["res"], "RH_FAR_WAVE=0")
    for r in a["res"]:
        assert np.isfinite(r["logZ"]).all() and np.isfinite(r["bp1"]).all() and np.isfinite(r["bp2"]).all()


def test_batch_size_does_not_matter(runs):
    """the four pairs of batch 1: the same bytes next to eight more pairs and on the other grid mapping"""
    assert far_names(runs["wave", 3]) == WAVE
    assert_same_bytes(runs["wave", 3]["res"][:len(runs["wave", 1]["res"])], runs["wave", 1]["res"], "24 against 8 sequences")


def test_packed_tiles_same_bytes_as_gathered(runs):
    a, b = runs["packed", 1], runs["gathered", 1]
    assert far_names(a) == WAVE and far_names(b) == GATHER, (a["kernels"], b["kernels"])
    assert_same_bytes(a["res"], b["res"], "RH_FAR_PK=0")


def test_vienna_two_molecule_batch(runs):
    a, b = runs["wave", "vienna"], runs["splitk", "vienna"]
    assert a["launches"] == b["launches"], (a["launches"], b["launches"])
    assert_same_bytes(a["res"], b["res"], "Vienna-BL RH_FAR_WAVE=0")
    for r in a["res"]:
        assert np.isfinite(r["logZ"]).all() and np.isfinite(r["hp"]).all() and r["hp"].max() > 0


_shared = []   # the suite's shared contexts stay referenced to the end of the session: a context's id() must not come back for another one
               # while tests/test_gpu_indexed_batch.py caches results by it


def test_shared_contexts_of_the_suite(runs, ctx):
    """conftest.py's session contexts, which every earlier test has used: the first pair of batch 1 on the linear path ("auto") has the
    fold bytes of this file's fresh context and reports the wave products; the log-space path agrees on the folds' log Z to the suite's 1e-9"""
    _shared.append(ctx)
    pairs = batches()[1][:1]
    ctx.batch_upload(pairs)
    ctx.batch_compute()
    r, ref = ctx.batch_results(0), runs["wave", 1]["res"][0]
    if ctx.path_name == "auto":
        assert ctx.last_path() == 1 and tuple(k[1] for k in ctx.batch_kernels()[:2]) == WAVE, (ctx.last_path(), ctx.batch_kernels())
        # (the folds only: what an earlier test left of the context's duplex and accessibility settings is not this test's)
        assert r["bp1"].tobytes() == ref["bp1"].tobytes() and r["bp2"].tobytes() == ref["bp2"].tobytes()
        assert r["logZ"][:2].tobytes() == ref["logZ"][:2].tobytes(), (r["logZ"], ref["logZ"])
    else:
        assert np.all(np.abs(r["logZ"][:2] - ref["logZ"][:2]) <= 1e-9 * np.maximum(1.0, np.abs(ref["logZ"][:2]))), (r["logZ"], ref["logZ"])
