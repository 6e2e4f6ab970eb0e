"""CPU suite: bench.py --dump-outputs -- the layout of the written arrays and the 64 MB bound on all of them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CAND = np.dtype([("i", np.int32), ("j", np.int32), ("p", np.float32)])   # rh_cand, as Context.batch_candidates_all returns it


def fake_scans(counts_per_pair, seed=0):
    g = np.random.default_rng(seed)
    out = {}
    for name in bench.SCAN_NAMES:
        first = np.concatenate([[0], np.cumsum(counts_per_pair)]).astype(np.int32)
        rec = np.zeros(first[-1], dtype=CAND)
        rec["i"], rec["j"], rec["p"] = g.integers(0, 500, first[-1]), g.integers(0, 500, first[-1]), g.random(first[-1])
        out[name] = (rec, first)
    return out


def test_rows_are_pair_i_j_p_in_path_order(tmp_path):
    scans = fake_scans([3, 0, 2])
    logz = np.arange(9.0).reshape(3, 3)
    bench.dump_outputs(str(tmp_path), scans, logz)
    for name in bench.SCAN_NAMES:
        a = np.load(tmp_path / (name + ".npy"))
        rec, first = scans[name]
        assert a.dtype == np.float64 and a.shape == (5, 4)
        assert list(a[:, 0]) == [0, 0, 0, 2, 2]
        assert (a[:, 1] == rec["i"]).all() and (a[:, 2] == rec["j"]).all() and (a[:, 3] == rec["p"]).all()
    assert (np.load(tmp_path / "logZ.npy") == logz).all()


def test_large_outputs_are_a_fixed_sample_under_64_MB(tmp_path):
    limit = 4 * 10 ** 5
    scans = fake_scans([4000] * 10)   # 5 x 40 000 rows x 32 B = 6.4 MB
    bench.dump_outputs(str(tmp_path / "a"), scans, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), scans, limit=limit)
    total = 0
    for name in bench.SCAN_NAMES:
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.shape == b.shape and (a == b).all() and 0 < len(a) < 40000
        assert (np.diff(a[:, 0]) >= 0).all()   # the sample keeps the path's order
        rec = scans[name][0]
        assert np.isin(a[:, 3], rec["p"].astype(np.float64)).all()
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert total <= limit + 5 * 128   # (128 B of .npy header per file)
    assert bench.DUMP_LIMIT_BYTES + 6 * 128 <= 64 * 10 ** 6
