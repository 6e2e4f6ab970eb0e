"""GPU suite (-m gpu): sequences of uploads on ONE context.  Everything that reaches the GPU is staged by stage()
(ractip_amd/csrc/staging.hip) from a checked request: every step on the shared context -- plain, constrained and indexed batches,
the one-shot calls, batches that switch the short-sequence routing on and off -- is compared with the same call on a freshly
created context, over the bytes of bp1 / bp2 / up1 / up2 / hp / logZ, batch_fallbacks(0..3) and rh_batch_layout, which also equals
the restatement of tests/test_batch_request_cpu.py.  An upload that fails behind the checks (out of memory) leaves no batch, one the
checks reject leaves the previous one."""
import ctypes

import numpy as np
import pytest

from test_batch_request_cpu import batch_layout_restated

pytestmark = pytest.mark.gpu
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")


def rnd(n, seed, plant=()):
    s = list(np.random.RandomState(seed).choice(list("ACGU"), n))
    for pos, ch in plant:
        s[pos] = ch
    return "".join(s)


def line(n, marks):
    c = ["."] * n
    for pos, ch in marks.items():
        c[pos] = ch
    return "".join(c)


def layout(c):
    ts, hs, uld, hld = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int()
    c._check(c.L.rh_batch_layout(c.h, ctypes.byref(ts), ctypes.byref(uld), ctypes.byref(hs), ctypes.byref(hld)))
    return ts.value, uld.value, hs.value, hld.value


def snapshot(c, lens1, lens2, nmax=None):
    """what a computed pair batch shows, as bytes"""
    c.batch_compute()
    lay = layout(c)
    assert lay == batch_layout_restated(list(lens1), list(lens2), c.max_w, nmax), (lay, lens1, lens2)
    res = [c.batch_results(p) for p in range(len(lens1))]
    return dict(results=[{k: (r[k].shape, r[k].tobytes()) for k in KEYS} for r in res], fallbacks=[c.batch_fallbacks(w) for w in range(4)], layout=lay)


def plain(pairs, **kw):
    def step(c):
        c.batch_upload(pairs, **kw)
        return snapshot(c, [len(a) for a, _ in pairs], [len(b) for _, b in pairs])
    return step


def indexed(seqs, index, **kw):
    def step(c):
        c.batch_upload_indexed(seqs, index, **kw)
        return snapshot(c, [len(seqs[a]) for a, _ in index], [len(seqs[b]) for _, b in index], nmax=max(len(s) for s in seqs))
    return step


def same(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        assert got[k] == want[k], "%s: %s differs from the fresh context" % (what, k)


def run_steps(make, steps):
    """every step on one context and on a context of its own; returns the shared context's snapshots"""
    out = []
    shared = make()
    try:
        for k, step in enumerate(steps):
            got = step(shared)
            fresh = make()
            try:
                same(got, step(fresh), "step %d" % (k + 1))
            finally:
                fresh.close()
            out.append(got)
    finally:
        shared.close()
    return out


# ---- Vienna-BL: plain, constrained, plain, indexed, indexed under constraints, the one-shot calls, the first batch again
S1 = [rnd(61, 1, [(2, "G"), (20, "C"), (50, "G")]), rnd(13, 2), rnd(40, 3)]
S2 = [rnd(45, 4, [(10, "C")]), rnd(29, 5), rnd(17, 6)]
PAIRS = list(zip(S1, S2))
FOLD = [(line(61, {2: "(", 20: ")", 30: "x", 31: "x", 32: "x"}), None), (None, line(29, {5: "x", 6: "x", 10: "<"})), None]
JOINT = [line(61 + 45, {5: "x", 50: "(", 61 + 10: ")"}), None, None]
SEQS = [rnd(33, 7, [(5, "G")]), rnd(7, 8, [(3, "C")]), rnd(58, 9), rnd(20, 10)]
INDEX = [(0, 1), (2, 2), (1, 0), (3, 2), (1, 3)]          # (2, 2): a sequence with itself; 0, 1, 2, 3 in both roles
I_FOLD = [None, None, None, line(20, {1: "x", 3: "<", 7: ">"})]
I_FIRST = [line(33, {5: "(", 9: "x"}), None, None, None]    # one '(' left open by s1 of pair 0 ...
I_SECOND = [None, line(7, {3: ")"}), "x..", None]           # ... and closed by its s2; sequence 2 as s2 of pairs 1 and 3
ONE = ("GGGAAAACCCAUAU", "(((....)))....")
CO = ("G" + rnd(14, 11), rnd(15, 12) + "C", "(" + "." * 29 + ")")


@pytest.mark.parametrize("cofold", [True, False], ids=["cofold", "duplex"])
def test_vienna_uploads_in_turn_equal_fresh_contexts(hotlib, cofold):
    import ractip_amd

    def make():
        c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL)
        c.set_hybrid(cofold)
        return c

    def masks(fold, joint):
        def check(c):
            assert (c.debug_allow_mask(0, 0) is not None) == fold and (c.debug_allow_mask(1, 0) is not None) == (joint and cofold)
        return check

    def with_masks(step, check):
        def both(c):
            got = step(c)
            check(c)
            return got
        return both

    def one_shot(c):
        bp, up, z = c.fold(*ONE)
        hp, zz = c.cofold(*CO)
        return dict(fold=(bp.tobytes(), np.asarray(up).tobytes(), z), cofold=(hp.tobytes(), zz))
    assert len(ONE[0]) == 14 and (len(CO[0]), len(CO[1])) == (15, 16) and (2, 2) in INDEX and len(SEQS) == 4 and len(INDEX) == 5
    steps = [with_masks(plain(PAIRS), masks(False, False)),
             with_masks(plain(PAIRS, constraints=FOLD, co_constraints=JOINT), masks(True, True)),
             with_masks(plain(PAIRS[:2]), masks(False, False)),            # the masks of the step before are gone
             with_masks(indexed(SEQS, INDEX), masks(False, False)),
             indexed(SEQS, INDEX, constraints=I_FOLD, co_first=I_FIRST, co_second=I_SECOND),
             one_shot,
             plain(PAIRS)]
    got = run_steps(make, steps)
    same(got[6], got[0], "the first batch again")
    assert got[1]["results"] != got[0]["results"], "the constraints of step 2 are meant to bind"


# ---- CONTRAfold model: the short-sequence routing on, off and on again (n_short, nmax_short, nmax_sweep belong to the upload)
def test_contrafold_routing_belongs_to_the_upload(hotlib):
    import ractip_amd
    shapes = [[(130, 35)], [(39, 39)], [(40, 8), (64, 64)], [(109, 53)]]
    batches = [[(rnd(a, 100 * k + p), rnd(b, 100 * k + p + 50)) for p, (a, b) in enumerate(sh)] for k, sh in enumerate(shapes)]
    run_steps(lambda: ractip_amd.Context(device=0), [plain(b) for b in batches])


# ---- an upload that fails behind the checks: the context holds no batch, and the next upload finds it as if nothing had happened
def test_a_failed_upload_leaves_no_batch(hotlib):
    import ractip_amd
    pair = [(rnd(64, 21), rnd(64, 22))]
    huge = [("A" * 60000, "U" * 60000)]   # 14 tables of 60 002^2 doubles per sequence: 403 GB each, refused from the free-memory figure before any allocation
    c = ractip_amd.Context(device=0)
    try:
        first = plain(pair)(c)
        with pytest.raises(ractip_amd.RhError, match=r"error -3: batch needs \d+ MiB of HBM"):      # RH_ERR_OOM
            c.batch_upload(huge)
        with pytest.raises(ractip_amd.RhError, match="no batch uploaded"):
            c.batch_compute()
        with pytest.raises(ractip_amd.RhError, match="no computed pair batch"):
            c.batch_results(0)
        with pytest.raises(ractip_amd.RhError, match="no computed pair batch"):
            c.batch_logz()
        with pytest.raises(ractip_amd.RhError, match="no pair batch"):
            layout(c)
        again = plain(pair)(c)
    finally:
        c.close()
    same(again, first, "the batch after a failed upload")
    fresh = ractip_amd.Context(device=0)
    try:
        same(again, plain(pair)(fresh), "the batch after a failed upload")
    finally:
        fresh.close()


# ---- an upload the checks reject: the previous batch stays, results, fallbacks and layout
def test_a_rejected_upload_leaves_the_batch_usable(hotlib):
    import ractip_amd
    c = ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL)
    try:
        before = plain(PAIRS, constraints=FOLD)(c)
        with pytest.raises(ractip_amd.RhError, match=r"error -1: sequence 3: unbalanced '\('"):
            c.batch_upload(PAIRS, constraints=[None, (None, "..((.."), None])
        lay = layout(c)
        res = [c.batch_results(p) for p in range(len(PAIRS))]
        assert c.debug_allow_mask(0, 0) is not None
        after = dict(results=[{k: (r[k].shape, r[k].tobytes()) for k in KEYS} for r in res], fallbacks=[c.batch_fallbacks(w) for w in range(4)], layout=lay)
        same(after, before, "the batch before a rejected upload")
        same(snapshot(c, [len(a) for a, _ in PAIRS], [len(b) for _, b in PAIRS]), before, "the batch before a rejected upload, computed again")
    finally:
        c.close()
