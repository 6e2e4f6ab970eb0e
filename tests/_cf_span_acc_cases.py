"""The cases of tests/test_gpu_span_cf_acc.py, shared with tests/test_cf_span_acc_cpu.py, which checks on the CPU that every
reference they use lies above 1e-9 (no entry is judged by the absolute floor of assert_prob_close).

A case is (kind, parameter, L, max_w[, count]): "every" -- every region of random_seq(parameter); "rand" -- `count` seeded regions of
random_seq(parameter); "side" -- the planted interior loop with a side of `parameter` letters (the entries of
tests/test_gpu_cf_accessibility.py, every fourth of them where L is not the length); "multi" -- the planted multiloop with
`parameter` branches; "forty" -- the hairpin with a loop of forty, every letter at widths 1, 2, 8, 15."""
import _cf_span_acc_ref as acc
import _span_cases as sc

EVERY_CASES = [("every", 41, 20, 15), ("every", 33, 12, 15), ("every", 13, 10, 15)]
MULTILOOP_L = [86, 85, 84, 83, 40]
# side 30: the loop's outer pair (7, n - 6) spans 45 letters, in the band at L = 46 and not at L = 45
SIDE_CASES = [("side", 29, 57, 32), ("side", 30, 58, 32), ("side", 31, 59, 32), ("side", 30, 46, 32), ("side", 30, 45, 32)]
FORTY_L = [56, 50, 49, 48]
EDGE_CASES = [("rand", 130, 63, 15, 30), ("rand", 130, 64, 15, 30), ("rand", 130, 65, 15, 30),      # the wavefront edge of the banded rows
              ("rand", 64, 70, 15, 40), ("rand", 65, 70, 15, 40), ("rand", 66, 70, 15, 40), ("rand", 129, 40, 15, 40),   # exterior blocks
              ("rand", 257, 20, 15, 24),                                                              # two workgroup columns
              ("rand", 47, 20, 15, 40),                                                               # unpadded rows
              ("rand", 90, 31, 33, 30), ("rand", 90, 32, 33, 30), ("rand", 90, 33, 33, 30), ("rand", 90, 34, 33, 30),   # the loop budget
              ("rand", 70, 70, 64, 40), ("rand", 70, 33, 64, 40)]
SCRAMBLED_CASES = [("every", 33, 12, 15), ("multi", 3, 85, 15), ("multi", 3, 84, 15), ("side", 30, 58, 32)]
ALL_CASES = (EVERY_CASES + [("multi", 3, L, 15) for L in MULTILOOP_L] + [("multi", 4, 106, 15)] + SIDE_CASES +
             [("forty", 56, L, 15) for L in FORTY_L] + EDGE_CASES)


def case_seq(case):
    kind, p = case[0], case[1]
    if kind in ("every", "rand"):
        return sc.random_seq(p)
    if kind == "side":
        return acc.planted_side(p)[0]
    if kind == "multi":
        return acc.planted_multiloop(p)[0]
    return acc.hairpin_of_forty()


def case_entries(case):
    kind, p, L, max_w = case[:4]
    if kind == "every":
        return acc.every(p, max_w)
    if kind == "rand":
        return acc.sampled(p, max_w, case[4], seed=1000 * p + L)
    if kind == "side":
        seq, entries, _ = acc.planted_side(p)
        return entries if L == len(seq) else entries[::4]
    if kind == "multi":
        return acc.multiloop_entries(*acc.planted_multiloop(p))
    n = len(acc.hairpin_of_forty())
    return [(i, w) for i in range(n) for w in (0, 1, 7, 14) if i + w < n]
