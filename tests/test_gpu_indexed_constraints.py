"""GPU suite (-m gpu): structure constraints on indexed batches -- rh_batch_upload_indexed_constrained, the kernel that composes
the joint constraints of the pairs from the shares of the distinct sequences (joint_cons_gather, ractip_amd/csrc/allow_mask.hip),
and the callers above it (hot.Context.batch_upload_indexed with constraints, pipeline.screen with structure lines).

The batch is tests/_indexed_constraint_cases.py.  Its masks are compared byte for byte with tests/_oracle.py:constraint_mask on
the materialised strings and with the masks of the expanded rh_batch_upload_constrained batch; its results have the bits of that
expanded batch (the guarantee of indexed batches, margin zero) and go against oracle/vienna_oracle.c at the project's tolerances:
REL = 1e-6 on bp and hp, REL with abs_floor = 1e-11 on up, 1e-9 relative on log Z."""
import numpy as np
import pytest

import _indexed_constraint_cases as cases
from _oracle import OraclePool, assert_prob_close
from test_gpu_batch_constraints import MODE_IDS, MODES, REL, SCANS, assert_same_bits, expected_image, logz_close, vcontext

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opool():
    p = OraclePool()
    yield p
    p.close()


@pytest.fixture(scope="module")
def B():
    """the batch, its expanded form and the joint strings (read only)"""
    seqs, cons, co_first, co_second, index = cases.batch()
    pairs, pair_cons, joint = cases.expanded(seqs, cons, co_first, co_second, index)
    return dict(seqs=seqs, cons=cons, co_first=co_first, co_second=co_second, index=index, pairs=pairs, pair_cons=pair_cons, joint=joint)


def upload(c, B, **over):
    kw = dict(constraints=B["cons"], co_first=B["co_first"], co_second=B["co_second"])
    kw.update(over)
    c.batch_upload_indexed(B["seqs"], B["index"], **kw)


def run_indexed(c, B, **over):
    upload(c, B, **over)
    c.batch_compute()
    return [c.batch_results(p) for p in range(len(B["index"]))]


def run_expanded(c, B):
    c.batch_upload(B["pairs"], constraints=B["pair_cons"], co_constraints=B["joint"])
    c.batch_compute()
    return [c.batch_results(p) for p in range(len(B["pairs"]))]


def small(B):
    """a smaller batch of the same kind: the distinct sequences 3..7 and the pairs among them"""
    keep = [k for k in range(3, 8)]
    index = [(a - 3, b - 3) for a, b in B["index"] if a in keep and b in keep]
    S = dict(seqs=B["seqs"][3:8], cons=B["cons"][3:8], co_first=B["co_first"][3:8], co_second=B["co_second"][3:8], index=index)
    S["pairs"], S["pair_cons"], S["joint"] = cases.expanded(S["seqs"], S["cons"], S["co_first"], S["co_second"], index)
    return S


# ---- 1. the bytes of the masks
def test_mask_bytes_by_index(hotlib, B):
    seqs, index = B["seqs"], B["index"]
    shares = set(B["co_first"]) | set(B["co_second"])
    assert None in shares and any(len(t) < len(s) for s, t in zip(seqs, B["co_first"]) if t) and len(B["co_first"][7]) > len(seqs[7])
    assert sorted({len(cases.open_brackets(t, len(s), True)) for s, t in zip(seqs, B["co_first"])}) == [0, 1, 2, 3]
    assert set("".join(B["joint"])) >= set("x()<>|.")
    used = [k for pr in index for k in pr]
    assert (4, 4) in index and used.count(3) == 4 and 8 not in used and 4 in [a for a, _ in index] and 4 in [b for _, b in index]
    a = len(seqs[0])
    assert B["joint"][0][:a].count("(") == 4 and B["joint"][0][a:].count(")") == 4 and "x" in B["joint"][0][:a] and "x" in B["joint"][0][a:]
    c = vcontext(hybrid=True)
    e = vcontext(hybrid=True)
    try:
        upload(c, B)
        e.batch_upload(B["pairs"], constraints=B["pair_cons"], co_constraints=B["joint"])
        assert c.batch_index() == (len(seqs), index)
        for k, s in enumerate(seqs):
            m = c.debug_allow_mask(0, k)
            n, ld = len(s), m.shape[0]
            assert m.shape == (ld, ld) and ld >= max(cases.LENS) + 2
            assert np.array_equal(m, expected_image(B["cons"][k], n, ld)), ("sequence", k, B["cons"][k])
        for p, (i, j) in enumerate(index):
            m = c.debug_allow_mask(1, p)
            n, ld = len(seqs[i]) + len(seqs[j]), m.shape[0]
            assert ld >= 65 + 64 + 2
            assert np.array_equal(m, expected_image(B["joint"][p], n, ld)), ("pair", p, B["joint"][p])
            assert np.array_equal(m, e.debug_allow_mask(1, p)), ("pair vs the expanded batch", p)
            assert np.array_equal(c.debug_allow_mask(0, i), e.debug_allow_mask(0, 2 * p)), ("s1 vs the expanded batch", p)
            assert np.array_equal(c.debug_allow_mask(0, j), e.debug_allow_mask(0, 2 * p + 1)), ("s2 vs the expanded batch", p)
        # only one kind of constraint: only that kind of mask
        upload(c, B, constraints=None)
        assert c.debug_allow_mask(0, 0) is None and np.array_equal(c.debug_allow_mask(1, 3), e.debug_allow_mask(1, 3))
        upload(c, B, co_first=None, co_second=None)
        assert c.debug_allow_mask(1, 0) is None and np.array_equal(c.debug_allow_mask(0, 1), e.debug_allow_mask(0, 2))
        # under pf_duplex the shares are checked and not staged
        c.set_hybrid(False)
        upload(c, B)
        assert c.debug_allow_mask(0, 0) is not None and c.debug_allow_mask(1, 0) is None
    finally:
        c.close()
        e.close()


# ---- 2. the bits of the expanded batch
@pytest.mark.parametrize("name,mode,path", MODES, ids=MODE_IDS)
def test_same_bits_as_the_expanded_constrained_batch(hotlib, B, name, mode, path):
    got, want = {}, {}
    for out, runner in ((got, run_indexed), (want, run_expanded)):
        c = vcontext(mode, hybrid=True)
        try:
            out["res"] = runner(c, B)
            assert c.last_path() == path, (c.last_path(), path)
            out["logz"] = c.batch_logz()
            out["cand"] = []
            for which, th in SCANS:
                rec, first = c.batch_candidates_all(which, th)
                out["cand"].append((rec.copy(), first.copy()))
        finally:
            c.close()
    assert_same_bits(got["res"], want["res"], name)
    assert np.array_equal(got["logz"], want["logz"])
    found = 0
    for (which, _), (rec, first), (rec0, first0) in zip(SCANS, got["cand"], want["cand"]):
        assert np.array_equal(first, first0) and np.array_equal(rec, rec0), which
        found += len(rec)
    assert found > 0


# ---- 3. against the CPU restatement
def test_indexed_constrained_batch_vs_oracle(hotlib, opool, B):
    seqs, index = B["seqs"], B["index"]
    for s in seqs:
        opool.mccaskill(s)
    for s1, s2 in B["pairs"]:
        opool.cofold(s1, s2)
    c = vcontext(hybrid=True)
    try:
        assert c.max_w == 15
        res = run_indexed(c, B)
        whole = c.batch_results_all()
        zs = c.batch_logz()
    finally:
        c.close()
    assert len(whole["bp"]) == len(seqs) and np.array_equal(zs[:, 2], [r["logZ"][2] for r in res])
    seen = {8: (whole["bp"][8], whole["up"][8], None)}          # the sequence no pair uses is folded under its constraint all the same
    for p, (i, j) in enumerate(index):
        seen.setdefault(i, (res[p]["bp1"], res[p]["up1"], res[p]["logZ"][0]))
        seen.setdefault(j, (res[p]["bp2"], res[p]["up2"], res[p]["logZ"][1]))
    assert sorted(seen) == list(range(len(seqs)))
    for k, (bp, up, z) in sorted(seen.items()):
        s, cs = seqs[k], B["cons"][k]
        o = opool.mccaskill(s).result() if cs is None else opool.constrained("mccaskill", s, 15, constraint=cs)
        w = "sequence %d n=%d" % (k, len(s))
        assert z is None or logz_close(z, o["logZ"]), (w, z, o["logZ"])
        assert np.array_equal(bp, whole["bp"][k]) and np.array_equal(up, whole["up"][k]), w
        assert_prob_close(bp, o["post"], rel=REL, what="bp " + w)
        assert_prob_close(up, o["up"], rel=REL, abs_floor=1e-11, what="up " + w)
    binding = 0
    for p, ((s1, s2), r) in enumerate(zip(B["pairs"], res)):
        cj = B["joint"][p]
        free = opool.cofold(s1, s2).result()
        o = opool.constrained("cofold", s1, s2, constraint=cj)
        w = "pair %d (%d, %d)" % (p, len(s1), len(s2))
        print("%s: logZ %.12g oracle %.12g unconstrained %.12g" % (w, r["logZ"][2], o["logZ"], free["logZ"]))
        assert logz_close(r["logZ"][2], o["logZ"]), (w, r["logZ"][2], o["logZ"])
        assert_prob_close(r["hp"], o["hp"], rel=REL, what="hp " + w)
        if p in cases.OPEN_PAIRS:
            assert abs(r["logZ"][2] - free["logZ"]) > 1e-3 and abs(o["logZ"] - free["logZ"]) > 1e-3, (w, "the joint constraint does not bind")
            binding += 1
        for a, ch in enumerate(cj[:len(s1)]):
            if ch == "x":
                assert r["hp"][a + 1].max() == 0, (w, a)                    # hp rows and columns of 'x' letters are 0
        for b, ch in enumerate(cj[len(s1):]):
            if ch == "x":
                assert r["hp"][:, b + 1].max() == 0, (w, b)
    assert binding >= 3


# ---- 4. nothing lingers
def test_uploads_of_every_kind_alternate_without_traces(hotlib, B):
    """One context: constrained indexed, plain indexed, constrained plain, then a smaller constrained indexed batch.  A stale mask,
    stale shares or rows of the composed constraints, or a seed left off would change a bit against fresh contexts."""
    S = small(B)
    assert 1 < len(S["index"]) < len(B["index"])
    c = vcontext(hybrid=True)
    try:
        first = run_indexed(c, B)
        plain = run_indexed(c, B, constraints=None, co_first=None, co_second=None)
        assert c.debug_allow_mask(0, 0) is None and c.debug_allow_mask(1, 0) is None
        third = run_expanded(c, B)
        fourth = run_indexed(c, S)
        masks = [c.debug_allow_mask(1, p) for p in range(len(S["index"]))]
    finally:
        c.close()
    fresh = []
    for runner, arg, kw in ((run_indexed, B, {}), (None, B, {}), (run_expanded, B, {}), (run_indexed, S, {})):
        c = vcontext(hybrid=True)
        try:
            if runner is None:
                c.batch_upload_indexed(arg["seqs"], arg["index"])
                c.batch_compute()
                fresh.append([c.batch_results(p) for p in range(len(arg["index"]))])
            else:
                fresh.append(runner(c, arg, **kw))
        finally:
            c.close()
    assert_same_bits(first, fresh[0], "constrained indexed vs a fresh context")
    assert_same_bits(plain, fresh[1], "plain indexed after a constrained one vs batch_upload_indexed on a fresh context")
    assert_same_bits(third, fresh[2], "constrained plain batch after indexed ones vs a fresh context")
    assert_same_bits(fourth, fresh[3], "a smaller constrained indexed batch after larger ones vs a fresh context")
    for p, (i, j) in enumerate(S["index"]):
        n, ld = len(S["seqs"][i]) + len(S["seqs"][j]), masks[p].shape[0]
        assert np.array_equal(masks[p], expected_image(S["joint"][p], n, ld)), p
    assert any(not np.array_equal(a["hp"], b["hp"]) for a, b in zip(first, plain))


# ---- 5. no constraint at all
def test_all_none_is_the_plain_indexed_upload(hotlib, B):
    ns = len(B["seqs"])
    c = vcontext(hybrid=True)
    try:
        c.batch_upload_indexed(B["seqs"], B["index"])
        c.batch_compute()
        want = [c.batch_results(p) for p in range(len(B["index"]))]
        for kw in (dict(constraints=[None] * ns, co_first=[None] * ns, co_second=[None] * ns), dict(constraints=[None] * ns, co_first=None, co_second=None),
                   dict(constraints=None, co_first=None, co_second=[None] * ns)):
            got = run_indexed(c, B, **kw)
            assert c.debug_allow_mask(0, 0) is None and c.debug_allow_mask(1, 0) is None
            assert_same_bits(got, want, "entries all None")
    finally:
        c.close()


# ---- 6. rejected uploads
def test_rejections_name_the_sequence_or_pair_and_leave_the_batch(hotlib, B):
    import ractip_amd
    seqs, index = B["seqs"], B["index"]

    def changed(what, k, value):
        out = list(B[what])
        out[k] = value
        return out
    c = vcontext(hybrid=True)
    try:
        good = run_indexed(c, B)

        def still_there():
            assert c.batch_index() == (len(seqs), index)
            assert_same_bits([c.batch_results(p) for p in range(len(index))], good, "after a rejected upload")
        with pytest.raises(ractip_amd.RhError, match=r"sequence 5: unbalanced '\('"):
            upload(c, B, constraints=changed("cons", 5, "..((.."))
        still_there()
        with pytest.raises(ractip_amd.RhError, match=r"sequence 6: unbalanced '\)'"):
            upload(c, B, constraints=changed("cons", 6, ".)"))
        # sequence 3 leaves one '(' open as s1; as s2 of pair 2 = (1, 3) it now leaves one ')' open where sequence 1 leaves two '('
        with pytest.raises(ractip_amd.RhError, match=r"pair 2: unbalanced '\('.*2 open in the first share, 1 in the second"):
            upload(c, B, co_second=changed("co_second", 3, B["co_second"][4]))
        still_there()
        # a ')' left open in a first share: sequence 2 is s1 of pair 3 first
        with pytest.raises(ractip_amd.RhError, match=r"pair 3: unbalanced '\)'.*first share"):
            upload(c, B, co_first=changed("co_first", 2, "...)" + B["co_first"][2][4:]))
        with pytest.raises(ractip_amd.RhError, match=r"pair 6: unbalanced '\('.*second share"):
            upload(c, B, co_second=changed("co_second", 4, B["co_second"][4][:28] + "(" + B["co_second"][4][29:]))
        still_there()
        # G-G across the cut: the open ')' of sequence 4 as s2 moved onto a G (pair 6 = (3, 4) is the first to use it)
        g = seqs[4].index("G", 13)
        with pytest.raises(ractip_amd.RhError, match=r"pair 6: a forced pair of non-complementary letters"):
            upload(c, B, co_second=changed("co_second", 4, "." * g + ")"))
        # ... and inside a share: sequence 5 as s1, first in pair 9
        a = seqs[5].index("C", 8)
        with pytest.raises(ractip_amd.RhError, match=r"pair 9: a forced pair of non-complementary letters"):
            upload(c, B, co_first=changed("co_first", 5, "." * a + "(" + "." * (14 - a) + ")"))
        with pytest.raises(ractip_amd.RhError, match="8 constraints for 9 sequences"):
            upload(c, B, constraints=B["cons"][:8])
        with pytest.raises(ractip_amd.RhError, match="8 constraints for 9 sequences"):
            upload(c, B, co_second=B["co_second"][:8])
        with pytest.raises(ractip_amd.RhError, match=r"pair 1 = \(1, 9\)"):
            c.batch_upload_indexed(seqs, [(0, 1), (1, 9)], constraints=B["cons"])
        still_there()
    finally:
        c.close()
    cf = vcontext(model=ractip_amd.hot.RH_MODEL_CONTRAFOLD)
    try:
        cf.batch_upload_indexed(seqs, index)
        cf.batch_compute()
        before = [cf.batch_results(p) for p in range(len(index))]
        for kw in (dict(constraints=B["cons"]), dict(co_first=B["co_first"]), dict(co_second=B["co_second"])):
            with pytest.raises(ractip_amd.RhError, match="Vienna-BL model only"):
                cf.batch_upload_indexed(seqs, index, **kw)
        assert cf.batch_index() == (len(seqs), index)
        assert_same_bits([cf.batch_results(p) for p in range(len(index))], before, "CONTRAfold model after rejected uploads")
        cf.batch_upload_indexed(seqs, index, constraints=[None] * len(seqs))      # no constraint at all: any model
        cf.batch_compute()
        assert_same_bits([cf.batch_results(p) for p in range(len(index))], before, "CONTRAfold model, entries all None")
    finally:
        cf.close()


# ---- 7. the screen
def test_screen_with_structure_lines_equals_predict_per_pair(hotlib):
    from ractip_amd import pipeline
    rng = np.random.RandomState(5)

    def planted(n, line, mate):
        s = list(rng.choice(list("ACGU"), n))
        for i, j in cases.inner_pairs(line):
            s[i], s[j] = "G", "C"
        for k, ch in enumerate(line):
            if ch in "[]":
                s[k] = mate[ch]
        return "".join(s)
    tq = ["((..))...[[.....", "..[[......"]            # every line of a cross product forces the same number of pairs
    tt = ["xxxx...]]..((...))", "..]]....xx", ".]]"]
    queries = [planted(22, tq[0], {"[": "G"}), planted(17, tq[1], {"[": "G"})]
    targets = [planted(24, tt[0], {"]": "C"}), planted(15, tt[1], {"]": "C"}), planted(9, tt[2], {"]": "C"})]
    c = vcontext()
    try:
        got = pipeline.screen(queries, targets, ctx=c, query_structures=tq, target_structures=tt)
        assert c.debug_allow_mask(1, 0) is not None
        for qi, q in enumerate(queries):
            for ti, t in enumerate(targets):
                want = pipeline.predict(q, t, ctx=c, structures=(tq[qi], tt[ti]))
                assert got[qi][ti] == want, (qi, ti, got[qi][ti], want)
    finally:
        c.close()
