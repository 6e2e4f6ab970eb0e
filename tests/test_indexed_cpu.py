"""CPU suite: the host side of indexed batches -- hot.index_pairs and pipeline.screen on a recording fake context."""
import numpy as np

from ractip_amd import hot, ilp, pipeline


def test_index_pairs_round_trips():
    pairs = [("GGGAAACCC", "UUUU"), ("ACGU", "UUUU"), ("UUUU", "GGGAAACCC"), ("GGGAAACCC", "GGGAAACCC"), ("acgu", "ACGU")]
    seqs, first, second = hot.index_pairs(pairs)
    assert [(seqs[i], seqs[j]) for i, j in zip(first, second)] == pairs
    assert len(set(seqs)) == len(seqs) and set(seqs) == {s for pr in pairs for s in pr}
    assert seqs == ["GGGAAACCC", "UUUU", "ACGU", "acgu"]           # first-appearance order; strings are compared as they are
    assert hot.index_pairs([]) == ([], [], [])
    import ractip_amd
    assert ractip_amd.index_pairs is hot.index_pairs


class RecordingContext:
    """Stands for hot.Context: records what screen hands to the batch interface."""

    def __init__(self):
        self.uploads, self.plain_uploads, self.asked = [], [], []

    def set_max_w(self, w):
        self.w = w

    def set_hybrid(self, on):
        self.hybrid = on

    def batch_upload(self, pairs, constraints=None, co_constraints=None):
        self.plain_uploads.append(pairs)

    def batch_upload_indexed(self, seqs, index_pairs):
        self.uploads.append((list(seqs), list(index_pairs)))

    def batch_compute(self):
        pass

    def batch_results(self, p):
        self.asked.append(p)
        seqs, index = self.uploads[-1]
        n1, n2 = len(seqs[index[p][0]]), len(seqs[index[p][1]])
        return dict(bp1=np.zeros(1), bp2=np.zeros(1), hp=np.zeros((n1 + 1, n2 + 1)), up1=np.ones((n1, self.w)), up2=np.ones((n2, self.w)))


def test_screen_uploads_each_distinct_string_once(monkeypatch):
    monkeypatch.setattr(ilp, "solve", lambda s1, s2, bp1, bp2, hp, up1, up2, opt: (s1, s2, hp.shape))
    queries = ["GGGAAACCCA", "UGGGAA", "GGGAAACCCA"]               # a repeated query ...
    targets = ["ACGUACGU", "UGGGAA"]                               # ... and a target that is also a query
    ctx = RecordingContext()
    out = pipeline.screen(queries, targets, ctx=ctx)
    assert ctx.plain_uploads == [] and len(ctx.uploads) == 1
    seqs, index = ctx.uploads[0]
    assert seqs == ["GGGAAACCCA", "ACGUACGU", "UGGGAA"]
    assert [(seqs[i], seqs[j]) for i, j in index] == [(q, t) for q in queries for t in targets]
    assert ctx.asked == list(range(6)) and ctx.hybrid is True and ctx.w == ilp.Options().max_w
    assert [len(row) for row in out] == [2, 2, 2]
    for qi, q in enumerate(queries):
        for ti, t in enumerate(targets):
            assert out[qi][ti] == (q, t, (len(q) + 1, len(t) + 1))
    assert pipeline.screen([], targets, ctx=ctx) == [] and pipeline.screen(queries, [], ctx=ctx) == [[], [], []]
    assert len(ctx.uploads) == 1
