"""GPU suite: what rh_batch_compute schedules -- the three products (CONTRAfold folds + duplex, Vienna-BL folds + pf_duplex,
Vienna-BL folds + two-molecule ensemble), every mode, and every route a problem outside the double range can take -- gives the
bits and the bookkeeping it gave before the scheduling code was split into one schedule per product.

tests/golden/compute_schedule_parent.json was recorded on an MI355X from the commit before that split: the library of that
commit, built from a checkout of it, run through this module's own entry point

    RACTIP_HOT_LIB=<parent checkout>/ractip_amd/libractip_hot.so python tests/test_gpu_compute_schedule.py record [OUT.json]

over the scenario list below, which serves recording and testing alike.  Per compute it holds rh_last_path, rh_last_hybrid_path,
rh_batch_fallbacks(0..3), the names and block-product launches of rh_batch_kernels, the launch counts of rh_batch_timings, one
SHA-256 per pair over the bytes of bp1, bp2, up1, up2, hp and logZ, and logZ in clear so that a mismatch can be read.  The test
asserts equality with all of it and that the phase times are finite and non-negative; `expect` states what each scenario is
there for and is checked when recording too (a scenario whose bookkeeping is not what it claims is a wrong scenario).

Ordinary sequences: seeded random ACGU, ragged, 35..130 letters (35: below the 40 letters from which the strips start, so the
per-sequence routing is on).  The overflowing inputs are the smallest the suite already proves to overflow: the G*348 + AAAA +
C*348 helix and the GC 600-mer with its reverse complement of test_mixed_batch_only_the_flagged_problems_fall_back, ("GC"*350,
"GC"*350) of test_vienna_bl_linear_duplex_path_and_its_fallback, the hairpins(900) chain of
test_vienna_bl_flagged_pairs_are_recomputed_alone and G*120 / C*120 of test_auto_recomputes_in_log_space_what_leaves_the_double_range."""
import contextlib
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "compute_schedule_parent.json")
KEYS = ("bp1", "bp2", "up1", "up2", "hp", "logZ")
INHERIT, AUTO, LOG, LINEAR = -1, 0, 1, 2

pytestmark = pytest.mark.gpu


# ---- inputs
def _rnd(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), n))


def _revcomp(s):
    return "".join({"A": "U", "U": "A", "G": "C", "C": "G"}[ch] for ch in reversed(s))


def _ordinary():
    rng = np.random.RandomState(2718)
    return [(_rnd(rng, a), _rnd(rng, b)) for a, b in ((130, 97), (35, 64), (88, 41), (63, 120))]


def _gc_duplex(seed):
    """a random GC 600-mer and its reverse complement: the duplex overflows, the folds do not"""
    a = _rnd(np.random.RandomState(seed), 600, "GC")
    return a, _revcomp(a)


def _hairpin_chain():
    """hairpins(900) of test_vienna_bl_flagged_pairs_are_recomputed_alone: the same generator in the same state"""
    rng = np.random.default_rng(9)
    for n in (300, 260, 150, 333, 64, 65, 400, 90, 220, 210, 900, 190, 128, 127, 77, 300):   # (its ordinary sequences come first)
        rng.choice(list("ACGU"), size=n)
    s = ""
    while len(s) < 900:
        stem = "".join(rng.choice(list("GC"), size=10))
        s += stem + "AAAA" + _revcomp(stem) + "AA"
    return s[:900]


ORD = _ordinary()
HELIX = "G" * 348 + "AAAA" + "C" * 348
_more = np.random.RandomState(314)
SIX = ORD + [(_rnd(_more, 77), _rnd(_more, 52)), (_rnd(_more, 101), _rnd(_more, 38))]
SIX_HELIX = SIX[:3] + [(HELIX, SIX[3][1])] + SIX[4:]                  # sequence 6
MOSTLY_HELIX = [(HELIX, HELIX), (HELIX, ORD[1][1])]                    # sequences 0, 1, 2 of four
GC_AMONG = ORD[:2] + [_gc_duplex(17)] + ORD[2:3]                       # pair 2 of four
MOSTLY_GC = [_gc_duplex(17), ORD[1], _gc_duplex(18)]                   # pairs 0, 2 of three
VIENNA_GC = ORD[:2] + [("GC" * 350, "GC" * 350)]                       # pair 2 of three
CHAIN = [ORD[0], (_hairpin_chain(), ORD[1][1]), ORD[2], ORD[3]]        # sequence 2, pair 1 of four
V2X = ORD[:3] + [("G" * 120, "C" * 120)]                               # pair 3 of four


def S(name, model, pairs, steps=((AUTO, INHERIT),), hybrid=False, env=None, constraints=None, overlap=True, timed=None,
      bits_of=None, **expect):
    """One scenario: a context of `model`, `env` set while it lives, one upload, one compute per step (mode, duplex mode).
    bits_of: the scenario whose results the LAST compute must reproduce bit for bit.  expect: of the last compute --
    path / hybrid_path, and f0..f3 = rh_batch_fallbacks(0..3): a list (equal to it) or a set (contained in it)."""
    return dict(name=name, model=model, pairs=pairs, steps=steps, hybrid=hybrid, env=env or {}, constraints=constraints,
                overlap=overlap, timed=timed, bits_of=bits_of, expect=expect)


NO_LADDER = {"RH_SCALE_LADDER": "0"}
SCENARIOS = [
    # CONTRAfold folds + duplex
    S("cf_auto", "contrafold", ORD, path=1, hybrid_path=1, f0=[], f1=[], f2=[], f3=[]),
    S("cf_log", "contrafold", ORD, steps=((LOG, INHERIT),), path=2, hybrid_path=2),
    S("cf_linear", "contrafold", ORD, steps=((LINEAR, INHERIT),), path=1, hybrid_path=1),
    S("cf_auto_duplex_log", "contrafold", ORD, steps=((AUTO, LOG),), path=1, hybrid_path=2),
    S("cf_log_duplex_auto", "contrafold", ORD, steps=((LOG, AUTO),), path=2, hybrid_path=1),
    S("cf_helix_fold_ladder", "contrafold", SIX_HELIX, path=3, f0=[], f2=[6]),
    S("cf_helix_fold_subbatch_log", "contrafold", SIX_HELIX, env=NO_LADDER, path=3, f0=[6], f2=[]),
    S("cf_helix_fold_whole_batch_log", "contrafold", MOSTLY_HELIX, env=NO_LADDER, path=3, f0=[0, 1, 2], f2=[]),
    S("cf_gc_duplex_ladder", "contrafold", GC_AMONG, hybrid_path=3, f1=[], f3=[2]),
    S("cf_gc_duplex_subbatch_log", "contrafold", GC_AMONG, env=NO_LADDER, hybrid_path=3, f1=[2], f3=[]),
    S("cf_gc_duplex_whole_batch_log", "contrafold", MOSTLY_GC, env=NO_LADDER, hybrid_path=3, f1=[0, 2], f3=[]),
    S("cf_log_then_auto_on_one_upload", "contrafold", ORD, steps=((LOG, INHERIT), (AUTO, INHERIT)), bits_of="cf_auto", path=1, hybrid_path=1),
    S("cf_auto_phases_apart", "contrafold", ORD, overlap=False, bits_of="cf_auto", path=1, hybrid_path=1),
    S("cf_auto_inside_kernels_timed", "contrafold", ORD, timed=0, bits_of="cf_auto", path=1, hybrid_path=1),
    # Vienna-BL folds + pf_duplex
    S("vd_auto", "vienna", ORD, path=1, hybrid_path=1, f0=[], f1=[], f2=[]),
    S("vd_log", "vienna", ORD, steps=((LOG, INHERIT),), path=2, hybrid_path=2),
    S("vd_gc_duplex_whole_batch_log", "vienna", VIENNA_GC, hybrid_path=3, f1={2}),
    # Vienna-BL folds + two-molecule ensemble
    S("vc_seeded", "vienna", ORD, hybrid=True, path=1, hybrid_path=1, f0=[], f1=[], f2=[]),
    S("vc_unseeded", "vienna", ORD, hybrid=True, env={"RH_CO_SEED": "0"}, path=1, hybrid_path=1),
    S("vc_constrained_unseeded", "vienna", ORD, hybrid=True, constraints=[("..xx....x", None), None, None, None], path=1, hybrid_path=1),
    S("vc_log", "vienna", ORD, hybrid=True, steps=((LOG, INHERIT),), path=2, hybrid_path=2),
    S("vc_seeded_phases_apart", "vienna", ORD, hybrid=True, overlap=False, bits_of="vc_seeded", path=1, hybrid_path=1),
    S("vc_chain_whole_batch_ladder", "vienna", CHAIN, hybrid=True, env={"RH_PAIR_HELPER": "0"}, path=3, f0=[], f2={2}),
    S("vc_chain_helper", "vienna", CHAIN, hybrid=True, env={"RH_PAIR_HELPER": "2"}, path=3, f0_or_f2=[2, 3]),
    S("vc_chain_log", "vienna", CHAIN, hybrid=True, env=NO_LADDER, path=3, hybrid_path=3, f2=[]),
    # ViennaRNA-2.x energies: log-space folds, pf_duplex on the linear kernels on request
    S("v2x_duplex_auto_overflow", "vienna2x", V2X, steps=((LOG, AUTO),), path=2, hybrid_path=3, f1=[3]),
]
BY_NAME = {s["name"]: s for s in SCENARIOS}


# ---- running one
@contextlib.contextmanager
def _environment(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _context(model, par20):
    import ractip_amd
    if model == "contrafold":
        return ractip_amd.Context(device=0)
    if model == "vienna":
        return ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL)
    return ractip_amd.Context(device=0, model=ractip_amd.hot.RH_MODEL_VIENNA_BL, param_file=par20, vienna=dict(use_bl_param=False))


def _synthetic_par20(directory):
    """the synthetic 2.x parameter file of tests/test_gpu_duplex2x_linear.py"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import vienna2x as v2
    path = os.path.join(str(directory), "synthetic_v20.par")
    v2.write_par_v20(path, v2.random_tables(23))
    return path


def _snapshot(c, npairs):
    res = [c.batch_results(p) for p in range(npairs)]
    ms, launches = c.batch_timings()
    digests = []
    for r in res:
        h = hashlib.sha256()
        for k in KEYS:
            h.update(np.ascontiguousarray(r[k], dtype=np.float64).tobytes())
        digests.append(h.hexdigest())
    snap = dict(last_path=c.last_path(), last_hybrid_path=c.last_hybrid_path(), fallbacks=[c.batch_fallbacks(w) for w in range(4)],
                kernels=[list(k) for k in c.batch_kernels()], launches=launches, sha256=digests,
                logZ=[[float(z) for z in r["logZ"]] for r in res])
    return snap, ms


def run_scenario(s, par20):
    """[(snapshot, phase times)] of the scenario's computes"""
    out = []
    with _environment(s["env"]):
        c = _context(s["model"], par20)
        try:
            if s["hybrid"]:
                c.set_hybrid(True)
            if not s["overlap"]:
                c.set_overlap(False)
            c.batch_upload(s["pairs"], constraints=s["constraints"])
            for mode, duplex_mode in s["steps"]:
                c.set_mode(mode)
                c.set_duplex_mode(duplex_mode)
                if s["timed"] is None:
                    c.batch_compute()
                else:
                    c.kernel_class_times(s["timed"], 1)     # (one compute with event pairs around that class, phases apart)
                out.append(_snapshot(c, len(s["pairs"])))
        finally:
            c.close()
    return out


def check_expectation(s, snap):
    e, f = s["expect"], snap["fallbacks"]
    if "path" in e:
        assert snap["last_path"] == e["path"], (s["name"], "last_path", snap["last_path"])
    if "hybrid_path" in e:
        assert snap["last_hybrid_path"] == e["hybrid_path"], (s["name"], "last_hybrid_path", snap["last_hybrid_path"])
    for w in range(4):
        want = e.get("f%d" % w, ())
        if isinstance(want, list):
            assert f[w] == want, (s["name"], "fallbacks", w, f[w])
        elif isinstance(want, set):
            assert want <= set(f[w]), (s["name"], "fallbacks", w, f[w])
    if "f0_or_f2" in e:     # the helper's pair, whichever mechanism held it there
        assert sorted(f[0] + f[2]) == e["f0_or_f2"], (s["name"], f)


def record(path):
    wrong = []
    with tempfile.TemporaryDirectory() as tmp:
        par20 = _synthetic_par20(tmp)
        done = {}
        for s in SCENARIOS:
            runs = run_scenario(s, par20)
            last = runs[-1][0]
            done[s["name"]] = [snap for snap, _ in runs]
            print("%-34s path %d hybrid %d fallbacks %s launches %s" % (s["name"], last["last_path"], last["last_hybrid_path"], last["fallbacks"],
                                                                  last["launches"]), flush=True)
            try:
                check_expectation(s, last)
                if s["bits_of"]:
                    assert last["sha256"] == done[s["bits_of"]][-1]["sha256"], (s["name"], "bits of", s["bits_of"])
            except AssertionError as e:
                wrong.append(e)
                print("NOT AS DESCRIBED:", e, flush=True)
    with open(path, "w") as f:
        json.dump(dict(scenarios=done), f, indent=0, sort_keys=True)
        f.write("\n")
    if wrong:
        sys.exit("%d scenario(s) do not do what they claim: fix the scenarios, then record again" % len(wrong))


# ---- the test
@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)["scenarios"]


@pytest.fixture(scope="module")
def par20(tmp_path_factory):
    return _synthetic_par20(tmp_path_factory.mktemp("par"))


def test_fixture_covers_the_scenario_list(parent):
    assert sorted(parent) == sorted(BY_NAME)
    for s in SCENARIOS:
        assert len(parent[s["name"]]) == len(s["steps"])
        if s["bits_of"]:
            assert parent[s["name"]][-1]["sha256"] == parent[s["bits_of"]][-1]["sha256"]


@pytest.mark.parametrize("name", [s["name"] for s in SCENARIOS])
def test_same_bits_and_bookkeeping_as_before_the_split(hotlib, parent, par20, name):
    s = BY_NAME[name]
    runs = run_scenario(s, par20)
    check_expectation(s, runs[-1][0])
    for step, ((got, ms), want) in enumerate(zip(runs, parent[name])):
        for p, (a, b) in enumerate(zip(got["logZ"], want["logZ"])):
            print("%s compute %d pair %d: logZ %s, recorded %s" % (name, step, p, a, b))
        for key in ("last_path", "last_hybrid_path", "fallbacks", "kernels", "launches"):
            assert got[key] == want[key], (name, step, key, got[key], want[key])
        assert np.array_equal(np.array(got["logZ"]), np.array(want["logZ"]), equal_nan=True), (name, step, "logZ")
        assert got["sha256"] == want["sha256"], (name, step, [p for p, (a, b) in enumerate(zip(got["sha256"], want["sha256"])) if a != b])
        assert len(ms) == 4 and all(np.isfinite(t) and t >= 0 for t in ms), (name, step, ms)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if len(sys.argv) < 2 or sys.argv[1] != "record":
        sys.exit("usage: RACTIP_HOT_LIB=<library of the parent commit> python tests/test_gpu_compute_schedule.py record [OUT.json]")
    record(sys.argv[2] if len(sys.argv) > 2 else FIXTURE)
