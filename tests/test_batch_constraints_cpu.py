"""CPU suite: the host side of the batched structure constraints -- the FASTA structure line, its two translations (Python pipeline
and C++ adapter) against the reference's rules (src/ractip.cpp:275-287, 409-440), the --use-constraint flag, and the O(n) pre-pass
with the per-cell rule of the mask kernel against the rectangle-clearing restatement (tools/constraint_prepass_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from _oracle import ractip_constraint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ractip_amd", "host")

# hand-written structure lines: (str1, n1, str2, n2, fold constraint of s1, of s2, joint constraint)
LINES = [
    ("[[.e(x)]", 10, "]].)e", 6, "xx.x(x)x..", "xx.)x.", "((..xxx..." + ")).x.."),
    ("..((..))..[[[..ll..", 19, "]]]...(())xx", 12, "..((..))..xxx..ll..", "xxx...(())xx", "..xx..xx..(((..xx.." + ")))...xxxxxx"),
    ("", 4, "....", 4, "....", "....", "........"),
    ("[[[[[[", 3, "]", 2, "xxx", "x.", "(((" + ")."),      # lines longer than the sequence are cut, shorter ones padded
    ("<|>.e", 5, "e|<>", 5, "<|>.x", "x|<>.", "....." + "....."),
]


def test_read_fasta_with_structure(tmp_path):
    from ractip_amd import pipeline
    a = tmp_path / "a.fa"
    a.write_text(">sRNA one\nGGGAAA\nCCCUUU\n((..[[....))\n>second\nACGU\n....\n")
    assert pipeline.read_fasta_with_structure(str(a)) == ("sRNA one", "GGGAAACCCUUU", "((..[[....))")
    b = tmp_path / "b.fa"
    b.write_text(">plain\nGGGAAA\nCCCUUU\n\n>second\nACGU\n")
    assert pipeline.read_fasta_with_structure(str(b)) == ("plain", "GGGAAACCCUUU", "")
    c = tmp_path / "c.fa"
    c.write_text(">letters only\nGGGAAACCC\nxxxlllexx\n")       # 'x' 'l' 'e' are structure characters, no nucleotide codes
    assert pipeline.read_fasta_with_structure(str(c)) == ("letters only", "GGGAAACCC", "xxxlllexx")
    # read_fasta stays as it is: it knows no structure line
    assert pipeline.read_fasta(str(a)) == ("sRNA one", "GGGAAACCCUUU((..[[....))")
    assert pipeline.read_fasta(str(b)) == ("plain", "GGGAAACCCUUU")


def test_read_fasta_unchanged_on_the_bundled_file(golden):
    from ractip_amd import pipeline
    path = os.path.join(ROOT, "ractip_amd", "data", "config5_OxyS_fhlA.fa")
    name, seq = pipeline.read_fasta(path)
    assert name == "OxyS" and seq == str(golden["mc/OxyS/seq"])
    assert pipeline.read_fasta_with_structure(path) == (name, seq, "")


def test_python_structure_line_translations():
    from ractip_amd import pipeline
    for t1, n1, t2, n2, c1, c2, cj in LINES:
        assert pipeline.fold_constraint(t1, n1) == c1 == ractip_constraint(t1, n1)
        assert pipeline.fold_constraint(t2, n2) == c2 == ractip_constraint(t2, n2)
        assert pipeline.joint_constraint(t1, n1, t2, n2) == cj and len(cj) == n1 + n2


@pytest.fixture(scope="module")
def cli():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "prob_cli")


def test_cpp_structure_line_translations(cli):
    """fold_constraint / joint_constraint of ractip_amd/host (what rnafold, rnaduplex_cofold and the batched member share)"""
    def out(*args):
        return subprocess.run([cli] + list(args), check=True, capture_output=True, text=True).stdout.rstrip("\n")
    for t1, n1, t2, n2, c1, c2, cj in LINES:
        assert out("constraint", t1, str(n1)) == c1 and out("constraint", t2, str(n2)) == c2
        assert out("joint", t1, str(n1), t2, str(n2)) == cj


class StubContext:
    """Stands for hot.Context: records what predict hands to the batch interface."""

    def __init__(self, n1, n2):
        self.uploads, self.n1, self.n2 = [], n1, n2

    def set_max_w(self, w):
        self.w = w

    def set_hybrid(self, on):
        self.hybrid = on

    def batch_upload(self, pairs, constraints=None, co_constraints=None):
        self.uploads.append((pairs, constraints, co_constraints))

    def batch_compute(self):
        pass

    def batch_results(self, p):
        return dict(bp1=np.zeros(1), bp2=np.zeros(1), hp=np.zeros((self.n1 + 1, self.n2 + 1)), up1=np.ones((self.n1, self.w)),
                    up2=np.ones((self.n2, self.w)))


def test_predict_hands_structures_to_the_batch_upload(monkeypatch):
    from ractip_amd import ilp, pipeline
    monkeypatch.setattr(ilp, "solve", lambda *a, **k: ("r1", "r2", 0.0))
    s1, s2 = "GGGAAACCCA", "UGGGAA"
    t1, _, t2, _, c1, c2, cj = LINES[0]
    ctx = StubContext(len(s1), len(s2))
    assert pipeline.predict(s1, s2, ctx=ctx, structures=(t1, t2))[:2] == ("r1", "r2")
    assert pipeline.predict(s1, s2, ctx=ctx)[:2] == ("r1", "r2")
    assert ctx.uploads == [([(s1, s2)], [(c1, c2)], [cj]), ([(s1, s2)], None, None)]
    with pytest.raises(ValueError):
        pipeline.predict(s1, s2, model="contrafold", ctx=ctx, structures=(t1, t2))


def test_use_constraint_flag(monkeypatch, tmp_path, capsys):
    from ractip_amd import pipeline
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_text(">a\nGGGAAACCCA\n[[.e(x)]\n")
    b.write_text(">b\nUGGGAA\n]].)e\n")
    seen = []

    def fake_predict(s1, s2, **kw):
        seen.append((s1, s2, kw.get("structures"), kw.get("duplex"), kw.get("model")))
        return "." * len(s1), "." * len(s2), 0.0
    monkeypatch.setattr(pipeline, "predict", fake_predict)
    pipeline.main(["--use-constraint", str(a), str(b)])
    pipeline.main([str(a), str(b), "--duplex"])
    assert seen == [("GGGAAACCCA", "UGGGAA", ("[[.e(x)]", "]].)e"), False, "vienna"), ("GGGAAACCCA", "UGGGAA", None, True, "vienna")]
    assert capsys.readouterr().out.startswith(">a\nGGGAAACCCA\n..........\n>b\nUGGGAA\n")


def test_prepass_and_cell_rule_against_rectangle_clearing(tmp_path):
    """The host pre-pass (ractip_amd/csrc/constraint_prepass.cpp: ch, P, enc and every rejection) and allow_pair, the rule the mask
    kernel evaluates per byte, on the program's built-in strings, 3000 random ones and the constraint strings of the GPU suite."""
    from test_gpu_batch_constraints import PARITY_EXTRA, ragged_batch
    _, cons, joint = ragged_batch(PARITY_EXTRA)
    exe = str(tmp_path / "constraint_prepass_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ractip_amd", "csrc"),
                           os.path.join(ROOT, "tools", "constraint_prepass_check.cpp"),
                           os.path.join(ROOT, "ractip_amd", "csrc", "constraint_prepass.cpp"), "-o", exe])
    args = [c for pr in cons for c in pr if c] + [j for j in joint if j]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
