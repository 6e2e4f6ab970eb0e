"""CPU suite: structure constraints on indexed batches, host side -- the per-share pass and the composition the kernel
joint_cons_gather evaluates (ractip_amd/csrc/constraint_prepass.h) against the pre-pass of the materialised joint string
(tools/joint_compose_check.cpp), hot.index_pairs_structured, and pipeline.screen with structure lines on a recording context."""
import os
import subprocess

import pytest

import _indexed_constraint_cases as cases
from ractip_amd import hot, ilp, pipeline
from test_indexed_cpu import RecordingContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shares_compose_to_the_joint_string(tmp_path):
    """share_prepass + joint_pair_check accept exactly what constraint_prepass accepts on pad(share1) + pad(share2), and
    compose_joint_letter + allow_pair then give its mask, every cell of it: the program's own cases (4000 random share pairs of
    1..40 letters over "x().<>|" among them) and the share pairs of the GPU batch."""
    exe = str(tmp_path / "joint_compose_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "ractip_amd", "csrc"),
                           os.path.join(ROOT, "tools", "joint_compose_check.cpp"),
                           os.path.join(ROOT, "ractip_amd", "csrc", "constraint_prepass.cpp"), "-o", exe])
    seqs, _, co_first, co_second, index = cases.batch()
    args = []
    for a, b in index:
        args += [seqs[a], co_first[a] or "", seqs[b], co_second[b] or ""]
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.endswith(", 0 failures") and int(last.split()[0]) >= 3000 + len(index), last
    bad = subprocess.run([exe, "GA", "(.", "GAC"], capture_output=True, text=True)      # (the program does report what it finds)
    assert bad.returncode == 1 and "FAIL" in bad.stdout


def test_index_pairs_structured_keys_on_sequence_and_structure():
    a, b, c = "GGGAAACCC", "UUUUCC", "ACGU"
    pairs = [((a, "(((...)))"), (b, "")), ((a, ""), (b, "")), ((c, ""), (a, "(((...)))")), ((a, "(((...)))"), (a, "")), ((b, "]]...."), (b, ""))]
    seqs, lines, first, second = hot.index_pairs_structured(pairs)
    assert [((seqs[i], lines[i]), (seqs[j], lines[j])) for i, j in zip(first, second)] == pairs
    assert list(zip(seqs, lines)) == [(a, "(((...)))"), (b, ""), (a, ""), (c, ""), (b, "]]....")]      # first-appearance order
    assert seqs.count(a) == 2 and len(set(zip(seqs, lines))) == len(seqs)                               # one sequence, two lines: two entries
    assert hot.index_pairs_structured([]) == ([], [], [], [])
    import ractip_amd
    assert ractip_amd.index_pairs_structured is hot.index_pairs_structured
    plain = [(p[0][0], p[1][0]) for p in pairs[:2]]                    # without lines it is index_pairs
    seqs, lines, first, second = hot.index_pairs_structured([((s1, ""), (s2, "")) for s1, s2 in plain])
    assert (seqs, first, second) == hot.index_pairs(plain) and lines == [""] * len(seqs)


class StructuredRecorder(RecordingContext):
    def batch_upload_indexed(self, seqs, index_pairs, constraints=None, co_first=None, co_second=None):
        self.uploads.append((list(seqs), list(index_pairs)))
        self.constraint_args = (constraints, co_first, co_second)


def test_screen_hands_structure_lines_over_once_per_distinct_entry(monkeypatch):
    monkeypatch.setattr(ilp, "solve", lambda s1, s2, bp1, bp2, hp, up1, up2, opt: (s1, s2, hp.shape))
    queries, tq = ["GGGAAACCCAGG", "UGGGAA", "GGGAAACCCAGG"], ["(((...)))[[.", "", "(((...)))[[."]
    targets, tt = ["ACGUACGUCC", "UGGGAA", "GGGAAACCCAGG"], ["xx..(..)]]", "", "..e......l]]xx"]       # the last line is longer than its sequence
    ctx = StructuredRecorder()
    out = pipeline.screen(queries, targets, ctx=ctx, query_structures=tq, target_structures=tt)
    assert ctx.plain_uploads == [] and len(ctx.uploads) == 1
    seqs, index = ctx.uploads[0]
    # a repeated (query, line) is one entry; the same string under another line is a second one; "UGGGAA" with "" is query and target
    assert seqs == ["GGGAAACCCAGG", "ACGUACGUCC", "UGGGAA", "GGGAAACCCAGG"]
    lines = ["(((...)))[[.", "xx..(..)]]", "", "..e......l]]xx"]
    assert [(seqs[i], seqs[j]) for i, j in index] == [(q, t) for q in queries for t in targets]
    assert index[2] == (0, 3) and index[4] == (2, 2)
    cons, first, second = ctx.constraint_args
    assert cons == [pipeline.fold_constraint(t, len(s)) for s, t in zip(seqs, lines)] == ["(((...)))xx.", "xx..(..)xx", "......", "..x......lxx"]
    assert first == ["xxx...xxx((.", "xx..x..x..", "......", ".........x.."]
    assert second == ["xxx...xxx...", "xx..x..x))", "......", ".........x))"]
    for p, (i, j) in enumerate(index):          # the two shares of a pair are the halves of joint_constraint
        assert first[i] + second[j] == pipeline.joint_constraint(lines[i], len(seqs[i]), lines[j], len(seqs[j])), p
    assert [len(row) for row in out] == [3, 3, 3] and out[1][2] == ("UGGGAA", "GGGAAACCCAGG", (7, 13))
    # one side only: the other side's lines are ""
    ctx = StructuredRecorder()
    pipeline.screen(queries[:2], targets[:1], ctx=ctx, query_structures=tq[:2])
    assert ctx.constraint_args[0] == ["(((...)))xx.", "..........", "......"] and ctx.constraint_args[2] == ["xxx...xxx...", "..........", "......"]
    with pytest.raises(ValueError, match="one structure line per"):
        pipeline.screen(queries, targets, ctx=StructuredRecorder(), query_structures=tq[:2])


def test_screen_with_structures_is_for_the_vienna_model_only():
    ctx = StructuredRecorder()
    with pytest.raises(ValueError, match="Vienna-BL"):
        pipeline.screen(["GGGAAACCC"], ["UUUU"], model="contrafold", ctx=ctx, query_structures=["(((...)))"])
    with pytest.raises(ValueError, match="Vienna-BL"):
        pipeline.screen(["GGGAAACCC"], ["UUUU"], model="contrafold", ctx=ctx, target_structures=[""])
    assert ctx.uploads == []


def test_screen_without_structures_makes_the_two_argument_call(monkeypatch):
    monkeypatch.setattr(ilp, "solve", lambda s1, s2, bp1, bp2, hp, up1, up2, opt: None)
    ctx = RecordingContext()                                            # its batch_upload_indexed(seqs, index_pairs) takes nothing else
    pipeline.screen(["GGGAAACCCA", "UGGGAA"], ["ACGUACGU"], ctx=ctx, query_structures=None, target_structures=None)
    assert len(ctx.uploads) == 1 and ctx.uploads[0] == (["GGGAAACCCA", "ACGUACGU", "UGGGAA"], [(0, 1), (2, 1)])


def test_joint_share_is_half_of_joint_constraint():
    t1, t2 = "[[..((...))..xle", "l..]]....(...)..e.xx"
    for n1, n2 in ((len(t1), len(t2)), (len(t1) + 3, len(t2) - 4), (5, 30)):
        assert pipeline.joint_share(t1, n1, True) + pipeline.joint_share(t2, n2, False) == pipeline.joint_constraint(t1, n1, t2, n2)
        assert len(pipeline.joint_share(t1, n1, True)) == n1 and len(pipeline.joint_share(t2, n2, False)) == n2
    assert pipeline.joint_share("[]", 2, True) == "(." and pipeline.joint_share("[]", 2, False) == ".)"
