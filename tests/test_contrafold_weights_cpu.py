"""The weight files and inputs of tests/test_gpu_contrafold_weights.py, pinned on the CPU oracle alone (no GPU, no gpu mark).

What is asserted here and not taken on trust: the generator is reproducible and moves every row; the never-read rows are derived from
the names and are exactly the zero letter-indexed rows of the bundled file, and moving them changes no bit of any oracle result; under
the committed scrambled file the 496 in-budget loop shapes keep their stems (>= 0.9) and the shapes one letter past the budget lose the
outer stem; the 0.5 keep rule leaves out at most 5 % of each planted family; every name-level mutant moves a compared quantity of every
family that reads its table by MARGIN = 100 GPU tolerances; the scrambled file is another model on every input (|d log Z| > 1e-3).

That a written file loads in rh_create is asserted where a context can be created: rh_create asks for a HIP device before it reads
the file, so every test of tests/test_gpu_contrafold_weights.py is that check."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _contrafold_cases as cc
import _contrafold_weight_cases as wc
import _contrafold_weights as cw
from _oracle import ORACLE_WORKERS, Oracle
from _vienna18_cases import MARGIN, PLANTED_MAY_DROP, movement, planted_kept

PLANTED = ("letters", "hairpin", "exterior", "multiloop")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> path: the bundled rows rewritten (shuffled), the scrambled rows, and both with the never-read rows moved by 0.3"""
    d = tmp_path_factory.mktemp("cf_weights")
    rows = {"bundled": cw.read(), "scrambled": cw.scrambled()}
    out = {}
    for k, r in rows.items():
        out[k] = cw.write(d / (k + ".params"), r, seed=1)
        out[k + " unread moved"] = cw.write(d / (k + "_unread.params"), cw.with_unread_moved(r, 0.3), seed=2)
    out["dir"] = d
    return out


@pytest.fixture(scope="module")
def results(files):
    return {k: wc.oracle_results(files[k]) for k in ("bundled", "scrambled")}


@pytest.fixture(scope="module")
def kept(results):
    """family -> kept indices under the scrambled file (the cap is asserted in its own test)"""
    out = {}
    for fam in PLANTED:
        cases = wc.letter_cases() if fam == "letters" else [c for c, _ in wc.junction_cases()[fam]]
        out[fam] = planted_kept(cases, [r["post"] for _, r in results["scrambled"][fam]])
    return out


def test_generator_is_reproducible_moves_every_row_and_its_files_load(files):
    base, a, b = cw.read(), cw.scrambled(), cw.scrambled()
    assert a == b and len(a) == len(base) == cw.NROWS == len({n for n, _ in a})
    assert [n for n, _ in a] == [n for n, _ in base]
    assert cw.scrambled(cw.SEED + 1) != a
    moved = np.array([v - v0 for (_, v), (_, v0) in zip(a, base)])
    numbered = np.array([cw.is_numbered(n) for n, _ in base])
    assert (moved != 0.0).all() and np.abs(moved[numbered]).max() <= cw.AMP_NUMBERED and np.abs(moved[~numbered]).max() <= cw.AMP_LETTERS
    assert numbered.sum() == 31 + 30 + 29 + 15 + 28 + 10 and np.abs(moved[~numbered]).max() > cw.AMP_NUMBERED
    back = cw.read(files["scrambled"])
    assert dict(back) == dict(a) and [n for n, _ in back] != [n for n, _ in a], "bit for bit, in another order"
    for k in ("bundled", "scrambled", "bundled unread moved", "scrambled unread moved"):
        Oracle(params=files[k])     # (asserts the load: no name missing)
    s = wc.fold_seqs()[0]
    assert Oracle(params=files["bundled"]).inference(s)["logZ"] == Oracle().inference(s)["logZ"], "the rewritten bundled file is the bundled model"


def test_unread_rows_are_derived_from_the_names_and_are_the_zero_letter_rows_of_the_bundled_file():
    rows = cw.read()
    un = cw.unread_rows()
    counts = {}
    for n in un:
        counts[cw.split_letters(n)[0]] = counts.get(cw.split_letters(n)[0], 0) + 1
    assert counts == cw.UNREAD_COUNTS and len(un) == 372
    total = {t: sum(cw.split_letters(n)[0] == t for n, _ in rows) for t in counts}
    assert total == {"terminal_mismatch": 256, "dangle_left": 64, "dangle_right": 64, "helix_stacking": 136, "helix_closing": 16, "base_pair": 10}
    assert set(un) == {n for n, v in rows if v == 0.0 and cw.split_letters(n)[1] is not None}
    moved = dict(cw.with_unread_moved(cw.scrambled(), 0.3))
    for n, v in cw.scrambled():
        assert moved[n] == (v + 0.3 if n in set(un) else v)


@pytest.mark.parametrize("which", ["bundled", "scrambled"])
def test_moving_the_unread_rows_changes_no_bit_of_any_oracle_result(files, results, which):
    """every input of every family, under both files: log Z, the whole posterior, hp and both duplex log Z; and the clone oracle of the
    accessibility inputs (a clone letter pairs with nothing either): every region the GPU module compares"""
    got = wc.oracle_results(files[which + " unread moved"])
    n = 0
    for fam in wc.FAMILIES:
        assert len(got[fam]) == len(results[which][fam]) > 0
        for (what, a), (_, b) in zip(results[which][fam], got[fam]):
            for key in a:
                assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (which, fam, what, key)
            n += 1
    rows = cw.read() if which == "bundled" else cw.scrambled()
    clones = {fam: (wc.CloneOracle(fam, files["dir"], rows, files[which]),
                    wc.CloneOracle(fam, files["dir"], cw.with_unread_moved(rows, 0.3), files[which + " unread moved"])) for fam in ("AU", "CG")}
    regions = sorted({(fam, seq, i, w) for fam, seq, _, entries in wc.acc_jobs() for i, w in entries})      # every accessibility input of the GPU module
    assert len(regions) > 2000 and {len(seq) for _, seq, _, _ in regions} >= set(wc.ACC_LENGTHS)

    def both(r):
        fam, seq, i, w = r
        c0, c1 = clones[fam]
        return c0.logz_clone(c0.recoded(seq, i, w)), c1.logz_clone(c1.recoded(seq, i, w)), c0.logz(seq), c1.logz(seq)

    with ThreadPoolExecutor(max_workers=ORACLE_WORKERS) as pool:
        for r, (z0, z1, f0, f1) in zip(regions, pool.map(both, regions)):
            assert z0 == z1 and f0 == f1, (which, r[0], len(r[1]), r[2], r[3])
    n += len(regions)
    print("%s: %d inputs, not a bit" % (which, n))


def test_in_budget_shapes_keep_their_stems_under_the_scrambled_file(results):
    """the 1e-9 bar on log Z resolves one loop weight only while that loop carries the partition function"""
    shapes = cc.shape_set()
    lo, per = 1.0, []
    for c, (_, r) in zip(shapes, results["scrambled"]["shapes"]):
        per.append(r["logZ"] / len(c.seq))
        if c.l1 + c.l2 <= cc.BUDGET:
            lo = min(lo, float(r["stems"].min()))
    print("seed %d at %.2f / %.2f: smallest stem probability of the 496 in-budget shapes %.4f, log Z per letter %.3f .. %.3f"
          % (cw.SEED, cw.AMP_LETTERS, cw.AMP_NUMBERED, lo, min(per), max(per)))
    assert sum(c.l1 + c.l2 <= cc.BUDGET for c in shapes) == 496 and lo >= 0.9


def test_one_letter_past_the_budget_the_outer_stem_falls_under_the_scrambled_file(files):
    """the property tests/test_gpu_contrafold_edges.py asserts under the bundled file (<= 0.6 of the probability at the budget)"""
    o = Oracle(params=files["scrambled"])
    worst = 0.0
    for at, past in cc.past_budget_pairs():
        p_at = cc.stem_probs(o.inference(at.seq)["post"], at)
        p_past = cc.stem_probs(o.inference(past.seq)["post"], past)
        worst = max(worst, p_past[0] / p_at[0])
        assert min(p_at) >= 0.9 and p_past[0] <= 0.6 * p_at[0], (past.what, p_at, p_past)
    print("one letter past the budget the outer stem keeps at most %.3f of its probability" % worst)


@pytest.mark.parametrize("which", ["bundled", "scrambled"])
def test_the_keep_rule_leaves_out_at_most_five_percent(results, which):
    for fam in PLANTED:
        cases = wc.letter_cases() if fam == "letters" else [c for c, _ in wc.junction_cases()[fam]]
        k = planted_kept(cases, [r["post"] for _, r in results[which][fam]])
        print("%s, %s: %d of %d left out" % (which, fam, len(cases) - len(k), len(cases)))
        assert len(cases) - len(k) <= PLANTED_MAY_DROP * len(cases), (which, fam)
        wc.kept(cases, [r["post"] for _, r in results[which][fam]])
    assert len(wc.letter_cases()) == 876


def test_the_scrambled_file_is_another_model_on_every_input(results):
    lo = min(abs(a["logZ"] - b["logZ"]) for fam in wc.FAMILIES for (_, a), (_, b) in zip(results["bundled"][fam], results["scrambled"][fam]))
    print("smallest |d log Z| between the bundled and the scrambled file over all inputs: %.3g" % lo)
    assert lo > 1e-3


MUTANT_NAMES = sorted(cw.MUTANT_FAMILIES)


def quantities(r):
    """what movement() weighs: log Z against 1e-9, every other entry as a probability (the outside log Z of a duplex is neither)"""
    return {k: v for k, v in r.items() if k != "logZ_out"}


def test_the_mutant_list():
    m = cw.mutants(cw.scrambled())
    assert sorted(m) == MUTANT_NAMES and len(m) == 16
    base = dict(cw.scrambled())
    for name, rows in m.items():     # a rewrite of names: the same 708 names, the same multiset of values, another assignment
        assert [n for n, _ in rows] == list(base) and sorted(v for _, v in rows) == sorted(base.values()) and dict(rows) != base, name


@pytest.mark.parametrize("name", MUTANT_NAMES)
def test_the_inputs_notice_every_mutant(files, results, kept, name):
    """The oracle under the scrambled file against the oracle under the mutated scrambled file: in every family that reads the table,
    log Z or a compared probability of at least 1e-6 moves by MARGIN = 100 GPU tolerances or more (movement of _vienna18_cases.py; a
    family's figure is the largest movement over its kept inputs).  DESIGN.md 5.1o lists every figure."""
    families = cw.MUTANT_FAMILIES[name]
    own = "mutant_%s.params" % "".join(ch if ch.isalnum() else "_" for ch in name)
    path = cw.write(files["dir"] / own, cw.mutants(cw.scrambled())[name], seed=3)
    got = wc.oracle_results(path, families=families, small_duplex=True, far2=False)
    for fam in families:
        keep = set(kept[fam]) if fam in kept else None
        base = dict(results["scrambled"][fam])       # (the mutants run on the folds up to 209 letters and on the small duplex pairs)
        mv = max(movement(quantities(base[what]), quantities(b)) for k, (what, b) in enumerate(got[fam]) if keep is None or k in keep)
        print("%-48s %-10s moves by %.3g tolerances" % (name, fam, mv))
        assert mv >= MARGIN, (name, fam, mv)
