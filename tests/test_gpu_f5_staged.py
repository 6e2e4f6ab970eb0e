"""Exterior-sum passes with staged operands (lin_f5i_pass / lin_f5o_pass fetch FCA as row segments through an LDS chunk buffer,
ractip_amd/csrc/f5_stage.h): the same BYTES as under RH_F5_PASS=0 (lin_f5i_tail / lin_f5o_head), at the lengths that
tests/test_gpu_f5_pass.py does not have.

  * sixteen consecutive lengths 130..145: every n mod 16, so every entry count of the last block of sixteen and every alignment of
    F5o's first block (k0 = n-1) and of the row segments against the 128-byte lines;
  * the chunk edges: a block's band has up to n-2 table rows and goes through LDS in chunks of STAGE_ROWS rows (kF5StageRows; all of
    it at every ld of this file), so n = R+1, R+2, R+3 and 2R+3 have R-1, R, R+1 and 2R+1 rows in their widest band;
  * one sequence of 1025 letters paired with one of 40: five terms per thread, the largest LDS request here, and a batch ld far above
    the short sequence's own;
  * a sequence count that is a multiple of 8 (XCD-pinned grids) and one that is not, over the same sequences.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGE_ROWS = 128   # kF5StageRows (ractip_amd/csrc/f5_stage.h)
CONSECUTIVE = list(range(130, 146))
CHUNK_EDGES = [STAGE_ROWS + 1, STAGE_ROWS + 2, STAGE_ROWS + 3, 2 * STAGE_ROWS + 3]
LENS = CONSECUTIVE + [n for n in CHUNK_EDGES if n not in CONSECUTIVE]
FILL = [60, 61, 70, 71, 80, 81]
LONG_SHORT = (1025, 40)
STRIPS = ("lin_inside_strip<8, 8, 1>", "lin_outside_strip<8, 8, 1>")
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")


def rnd(rng, n):
    return "".join("ACGU"[k] for k in rng.randint(0, 4, n))


def batches():
    """pinned -> pairs: 18 sequences (not a multiple of 8) and the same plus six fillers (24: XCD-pinned grids); "long": 1025 with 40"""
    rng = np.random.RandomState(533)
    seqs = [rnd(rng, n) for n in LENS]
    fill = [rnd(rng, n) for n in FILL]
    assert len(seqs) == 18 and len(seqs + fill) % 8 == 0
    plain = [(seqs[q], seqs[q + 1]) for q in range(0, len(seqs), 2)]
    return {False: plain, True: plain + [(fill[q], fill[q + 1]) for q in range(0, len(fill), 2)],
            "long": [(rnd(rng, LONG_SHORT[0]), rnd(rng, LONG_SHORT[1]))]}


def compute(env, pairs):
    """Results of one batch on a context created under `env`"""
    import ractip_amd
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        c = ractip_amd.Context(device=0)
    finally:
        mp.undo()
    try:
        c.batch_upload(pairs)
        c.batch_compute()
        assert c.last_path() == 1 and c.batch_fallbacks(0) == [] and c.batch_fallbacks(2) == [], (env, c.last_path())
        return dict(res=[c.batch_results(p) for p in range(len(pairs))], kernels=c.batch_kernels(), launches=tuple(c.batch_timings()[1]))
    finally:
        c.close()


@pytest.fixture(scope="module")
def runs(hotlib):
    """Every GPU result of this file, computed once: each batch under the pass kernels and under RH_F5_PASS=0"""
    out = {}
    for key, pairs in batches().items():
        out["pass", key] = compute({}, pairs)
        out["serial", key] = compute({"RH_F5_PASS": "0"}, pairs)
    return out


def assert_same_bytes(a, b, what):
    assert len(a) == len(b)
    for p, (r, r0) in enumerate(zip(a, b)):
        for key in KEYS:
            assert r[key].tobytes() == r0[key].tobytes(), (what, p, key)


@pytest.mark.parametrize("key", [True, False, "long"], ids=["multiple_of_8", "not_multiple_of_8", "1025_with_40"])
def test_staged_same_bytes_as_serial_kernels(runs, key):
    a, b = runs["pass", key], runs["serial", key]
    assert (a["kernels"][0][0], a["kernels"][1][0]) == STRIPS, a["kernels"]
    assert a["kernels"] == b["kernels"] and a["launches"] == b["launches"], (a["kernels"], b["kernels"], a["launches"], b["launches"])
    assert_same_bytes(a["res"], b["res"], "RH_F5_PASS=0")
    for r in a["res"]:
        assert np.isfinite(r["logZ"]).all() and np.isfinite(r["bp1"]).all() and np.isfinite(r["bp2"]).all()


def test_batch_size_does_not_matter(runs):
    """the 18 sequences of the smaller batch: the same bytes next to six more sequences and on the other grid mapping"""
    assert_same_bytes(runs["pass", True]["res"][:len(runs["pass", False]["res"])], runs["pass", False]["res"], "24 against 18 sequences")
