"""GPU suite: rh_batch_results_packed_f32 -- the dense results of a batch narrowed to float on the device and packed as
rh_batch_packed_layout says.  Throughout, the expected image is built in numpy from the doubles of the existing batch_results_all():
np.float32 of every block, placed at the offsets of batch_packed_layout(), zeros elsewhere; it is compared with the fetched buffers
as uint32 words, whole buffers, padding included.  (float)x is one correctly rounded IEEE conversion on both sides, so the bits are
equal or the kernel is wrong."""
import ctypes
import os

import numpy as np
import pytest

import ractip_amd
from ractip_amd import hot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [(1, 1), (2, 3), (5, 4), (7, 64), (65, 31), (113, 53), (130, 1)]


def rnd(n, seed):
    return "".join(np.random.RandomState(seed).choice(list("ACGU"), n))


def ragged_pairs(lens=RAGGED, seed=700):
    return [(rnd(a, seed + 2 * k), rnd(b, seed + 2 * k + 1)) for k, (a, b) in enumerate(lens)]


def expected_image(ctx):
    """(bp, up, hp) float32 images from the doubles of batch_results_all(), and its logZ (npairs, 3)"""
    bo, uo, ho, tot = ctx.batch_packed_layout()
    img = [np.zeros(int(t), dtype=np.float32) for t in tot]

    def put(kind, at, block):
        flat = np.ascontiguousarray(block, dtype=np.float64).ravel().astype(np.float32)
        img[kind][int(at):int(at) + flat.size] = flat

    res = ctx.batch_results_all()
    if isinstance(res, dict):                       # indexed upload: per distinct sequence, per pair
        for k in range(len(res["bp"])):
            put(0, bo[k], res["bp"][k])
            put(1, uo[k], res["up"][k])
        for p in range(len(res["hp"])):
            put(2, ho[p], res["hp"][p])
        return img, np.array(res["logZ"])
    for p, r in enumerate(res):
        put(0, bo[2 * p], r["bp1"]); put(0, bo[2 * p + 1], r["bp2"])
        put(1, uo[2 * p], r["up1"]); put(1, uo[2 * p + 1], r["up2"])
        put(2, ho[p], r["hp"])
    return img, np.array([r["logZ"] for r in res])


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def assert_image(ctx, bufs=None):
    """fetch, compare the whole buffers and the views with the expected image; returns the fetch"""
    want, logz = expected_image(ctx)
    got = ctx.batch_results_packed_f32(bufs)
    for kind, name in enumerate(("bp", "up", "hp")):
        assert same_bits(got["bufs"][kind], want[kind]), "%s image differs in %d of %d words" % (
            name, int(np.count_nonzero(got["bufs"][kind].view(np.uint32) != want[kind].view(np.uint32))), want[kind].size)
    assert np.array_equal(got["logZ"], logz)
    return got


def release(ctx, got):
    for b in got["bufs"]:
        ctx.pinned_free(b)


def test_ragged_batch_has_the_bits_of_the_narrowed_doubles(ctx):
    """Block sizes T(1) = 3, T(2) = 6, T(5) = 21 (no multiples of 4); hp pitches n2+1 = 2, 4, 5, 32, 54, 65 against an even source
    pitch; hp of (113, 53) and bp of 130 span several workgroups with a partial last one; the shortest problem next to the longest."""
    pairs = ragged_pairs()
    ctx.batch_upload(pairs)
    bo, uo, ho, tot = ctx.batch_packed_layout()          # valid before the compute
    assert all(int(x) % 4 == 0 for off in (bo, uo, ho) for x in off)
    assert [int(bo[k + 1] - bo[k]) for k in (0, 2, 4)] == [4, 8, 24] and sorted({b + 1 for _, b in RAGGED}) == [2, 4, 5, 32, 54, 65]
    assert 114 * 54 > 4 * 256 * 4 and 131 * 132 // 2 > 4 * 256 * 4                    # more than one workgroup of 256 threads x 4 groups
    ctx.batch_compute()
    got = assert_image(ctx)
    # the views: slices of the buffers with the shapes of batch_results
    assert len(got["bp"]) == len(got["up"]) == 2 * len(pairs) and len(got["hp"]) == len(pairs)
    for p, (a, b) in enumerate(RAGGED):
        one = ctx.batch_results(p)
        assert got["hp"][p].shape == (a + 1, b + 1) and got["hp"][p].base is not None
        assert same_bits(got["hp"][p], one["hp"].astype(np.float32))
        assert same_bits(got["bp"][2 * p], one["bp1"].astype(np.float32)) and same_bits(got["bp"][2 * p + 1], one["bp2"].astype(np.float32))
        assert same_bits(got["up"][2 * p], one["up1"].astype(np.float32)) and same_bits(got["up"][2 * p + 1], one["up2"].astype(np.float32))
        assert np.shares_memory(got["hp"][p], got["bufs"][2]) and np.shares_memory(got["bp"][2 * p], got["bufs"][0])
    release(ctx, got)


def test_float_subnormals_and_values_that_round_to_zero(ctx):
    """OxyS / fhlA: hp holds entries in the float-subnormal range and positive entries below half the smallest subnormal.  A
    flush-to-zero mode in the build would turn this red."""
    fa = [l.strip() for l in open(os.path.join(ROOT, "ractip_amd", "data", "config5_OxyS_fhlA.fa")) if not l.startswith(">")]
    ctx.batch_upload([(fa[0], fa[1])])
    ctx.batch_compute()
    hp = ctx.batch_results(0)["hp"]
    assert np.count_nonzero((hp >= 1.4e-45) & (hp < 1.17e-38)) >= 1
    assert np.count_nonzero((hp > 0) & (hp < 7e-46)) >= 1
    got = assert_image(ctx)
    f = got["hp"][0]
    assert np.count_nonzero((f > 0) & (f < np.float32(1.17e-38))) >= 1            # subnormal floats arrived as such
    release(ctx, got)


@pytest.fixture(scope="module")
def vienna(hotlib):
    c = ractip_amd.Context(device=0, model=hot.RH_MODEL_VIENNA_BL)
    yield c
    c.close()


@pytest.mark.parametrize("cofold", [True, False], ids=["cofold", "duplex"])
@pytest.mark.parametrize("max_w", [1, 15, 64])
def test_vienna_model_every_width_both_hybrid_sources(vienna, cofold, max_w):
    """three pairs; n = 1 and n = 17 are shorter than max_w = 64 (up blocks of n * max_w entries, rows longer than the sequence)"""
    vienna.set_hybrid(cofold)
    vienna.set_max_w(max_w)
    vienna.batch_upload(ragged_pairs([(1, 17), (40, 33), (70, 64)], seed=810))
    vienna.batch_compute()
    got = assert_image(vienna)
    assert got["up"][0].shape == ((1, max_w) if max_w > 1 else (1,)) and got["up"][1].shape == ((17, max_w) if max_w > 1 else (17,))
    release(vienna, got)


def test_indexed_batch_blocks_per_distinct_sequence_and_per_pair(ctx):
    seqs = [rnd(n, 900 + n) for n in (12, 9, 30, 40)]
    index = [(0, 1), (1, 0), (2, 2), (0, 2), (1, 1)]        # 1 (and 0, 2) as s1 and as s2; sequence 3 in no pair
    ctx.batch_upload_indexed(seqs, index)
    ctx.batch_compute()
    bo, uo, ho, tot = ctx.batch_packed_layout()
    assert len(bo) == len(uo) == len(seqs) + 1 and len(ho) == len(index) + 1
    got = assert_image(ctx)
    assert len(got["bp"]) == len(got["up"]) == 4 and len(got["hp"]) == 5
    assert [x.size for x in got["bp"]] == [hot.tri_size(len(s)) for s in seqs]
    assert [x.shape for x in got["hp"]] == [(len(seqs[a]) + 1, len(seqs[b]) + 1) for a, b in index]
    assert np.count_nonzero(got["bp"][3]) > 0              # the sequence no pair uses is folded and fetched all the same
    release(ctx, got)


def test_reuse_leaves_nothing_of_an_earlier_image(ctx):
    big = ragged_pairs([(130, 127), (128, 131), (129, 130), (133, 126), (130, 130), (127, 129), (131, 128), (132, 125)], seed=40)
    ctx.batch_upload(big)
    ctx.batch_compute()
    first = assert_image(ctx)
    keep = [b.copy() for b in first["bufs"]]
    doubles = ctx.batch_results_all()
    again = ctx.batch_results_packed_f32(first["bufs"])                    # two consecutive fetches: the same buffers, the same bits
    assert all(x is y for x, y in zip(again["bufs"], first["bufs"]))
    assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, k.view(np.uint32) if k.dtype == np.float32 else k)
               for a, k in zip(again["bufs"], keep))
    after = ctx.batch_results_all()                                        # the double tables are only read
    for r0, r1 in zip(doubles, after):
        assert all(np.array_equal(r0[k], r1[k]) for k in ("bp1", "bp2", "up1", "up2", "hp", "logZ"))
    ctx.batch_upload(ragged_pairs([(2, 3)], seed=41))                      # a tiny batch on the same context and staging buffer
    ctx.batch_compute()
    small = assert_image(ctx, again["bufs"])                               # whole buffers equal the expected image, padding included
    assert [b.size for b in small["bufs"][:3]] == [8 + 12, 4 + 4, 12]
    release(ctx, small)


def test_null_pointers_fetch_the_rest(ctx):
    ctx.batch_upload(ragged_pairs([(5, 4), (33, 18)], seed=50))
    ctx.batch_compute()
    full = assert_image(ctx)
    want = [b.copy() for b in full["bufs"]]
    names = ("bp", "up", "hp", "logz")
    for skip in range(4):
        for b in full["bufs"]:
            b.view(np.uint8)[...] = 0xA5
        got = ctx.batch_results_packed_f32(full["bufs"], want=tuple(n for k, n in enumerate(names) if k != skip))
        for k, b in enumerate(got["bufs"]):
            if k == skip:
                assert np.all(b.view(np.uint8) == 0xA5), names[k] + " was written though its pointer was NULL"
            else:
                assert np.array_equal(b.view(np.uint8), want[k].view(np.uint8)), names[k]
    for b in full["bufs"]:
        b.view(np.uint8)[...] = 0xA5
    ctx.batch_results_packed_f32(full["bufs"], want=())                    # nothing asked for: nothing to do, no error
    assert all(np.all(b.view(np.uint8) == 0xA5) for b in full["bufs"])
    release(ctx, full)


def test_errors_before_a_compute_and_without_a_batch(ctx, hotlib):
    ctx.batch_upload(ragged_pairs([(5, 4)], seed=60))
    bo, uo, ho, tot = ctx.batch_packed_layout()                            # the layout is known from the lengths
    assert [int(t) for t in tot] == [24 + 16, 8 + 4, 32]
    with pytest.raises(ractip_amd.RhError, match="no computed pair batch"):
        ctx.batch_results_packed_f32()
    ctx.batch_compute()
    release(ctx, assert_image(ctx))
    fresh = ractip_amd.Context(device=0)
    try:
        out = np.zeros(64, dtype=np.float32)
        rc = hotlib.rh_batch_results_packed_f32(fresh.h, out.ctypes.data, None, None, None)
        assert rc == -1 and b"no computed pair batch" in hotlib.rh_last_error(fresh.h)
        rc = hotlib.rh_batch_packed_layout(fresh.h, None, None, None, None)
        assert rc == -1 and b"no pair batch" in hotlib.rh_last_error(fresh.h)
        ms = ctypes.c_double()
        assert hotlib.rh_batch_pack_time(fresh.h, ctypes.byref(ms)) == -1
    finally:
        fresh.close()
