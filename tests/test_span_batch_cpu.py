"""CPU suite of the plan of a batch of span folds (rh_span_fold_batch): span_batch_plan of ractip_amd/csrc/span_fold.{h,cpp} through
the stand-alone program tools/span_batch_check.cpp built with the host sanitizers -- every rejection with its text and the item it
names, the per-item plans against span_check / span_acc_check, the result offsets as running sums, the greedy chunks at the budgets
where they change, and the sizes of 8 x (n = 10^6, L = 1000) as size_t."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ractip_amd", "csrc")
RH_ERR_ARG = -1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bin") / "span_batch_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "span_batch_check.cpp"), os.path.join(CSRC, "span_fold.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def plan(exe, L, max_w, budget, lens):
    """dict(head, items, singles, chunks) of integer lists"""
    out = dict(items=[], singles=[], chunks=[])
    for line in run(exe, L, max_w, budget, *lens).splitlines():
        kind, rest = line.split()[0], [int(x) for x in line.split()[1:]]
        if kind == "ok":
            out["head"] = rest
        else:
            out[kind + "s"].append(rest)
    return out


def item_bytes(n, L, max_w):
    """the plan formula: 13 tables of Le * ldn doubles, plus the gap sums (2 * 32 rows of ldn doubles) where widths above one are asked for"""
    Le, ldn = min(n, L), -(-(n + 1) // 16) * 16
    return 13 * Le * ldn * 8 + (2 * 32 * ldn * 8 if max_w > 1 else 0)


@pytest.mark.parametrize("args,text", [
    ((20, 5, 0), "span fold batch: the batch has 0 items (must be >= 1)"),
    ((20, 5, 0, "nullseqs"), "span fold batch: the array of sequences is NULL"),
    ((20, 5, 0, "nulllens"), "span fold batch: the array of lengths is NULL"),
    ((1, 5, 0, 40, 50), "span fold batch: max_span 1 (must be >= 2)"),
    ((-7, 5, 0, 40, 50), "span fold batch: max_span -7 (must be >= 2)"),
    ((20, 0, 0, 40, 50), "span fold batch: max_w 0 (must be 1..64)"),
    ((20, 65, 0, 40, 50), "span fold batch: max_w 65 (must be 1..64)"),
    ((20, -3, 0, 40, 50), "span fold batch: max_w -3 (must be 1..64)"),
    ((20, 5, 0, 40, "null", 50), "span fold batch: item 1: the sequence is NULL"),
    ((20, 5, 0, "null"), "span fold batch: item 0: the sequence is NULL"),
    ((20, 5, 0, 40, 50, 0), "span fold batch: item 2: the sequence has length 0 (must be >= 1)"),
    ((20, 5, 0, -3, 50), "span fold batch: item 0: the sequence has length -3 (must be >= 1)"),
    ((20, 5, 0, 40, 2 ** 31 - 1), "span fold batch: item 1: the length 2147483647 overflows the row pitch"),
    ((2 ** 30, 5, 0, 40, 40, 40, 2 ** 30), "span fold batch: item 3: the tables of 1073741824 letters at max_span 1073741824 overflow size_t"),
    ((2 ** 28, 1, 0) + (2 ** 28,) * 32, "span fold batch: item 31: the results of the items up to it overflow size_t"),
])
def test_every_rejection_with_its_text(exe, args, text):
    assert run(exe, *args) == "err %d %s\n" % (RH_ERR_ARG, text)


@pytest.mark.parametrize("L,max_w,lens", [(20, 1, [40, 1, 257, 47, 13]), (70, 15, [300, 1, 2, 64, 65, 129]), (500, 64, [70, 10])])
def test_the_items_are_the_single_plans_and_the_offsets_running_sums(exe, L, max_w, lens):
    p = plan(exe, L, max_w, 0, lens)
    assert p["head"][:3] == [len(lens), L, max_w] and len(p["items"]) == len(p["singles"]) == len(lens)
    band = up = 0
    for k, (n, item, single) in enumerate(zip(lens, p["items"], p["singles"])):
        Le, ldn = min(n, L), -(-(n + 1) // 16) * 16
        gaps = 64 * ldn if max_w > 1 else 0
        assert single == [k, n, Le, ldn, Le * ldn, 13 * Le * ldn, n * Le, 2 * (n + 1), n * max_w, gaps]
        assert item[:10] == single, "the plan of item %d is that of the single call" % k
        assert item[10:] == [band, up, item_bytes(n, L, max_w)]
        band += n * Le
        up += n * max_w
    assert p["head"][3:5] == [band, up]


def test_chunks_at_the_budgets_where_they_change(exe):
    L, max_w, n = 70, 15, 300
    one = item_bytes(n, L, max_w)
    ldn = 304
    # everything fits; the default budget too
    for budget in (3 * one, 0):
        p = plan(exe, L, max_w, budget, [n] * 3)
        assert p["chunks"] == [[0, 3, 3 * 13 * 70 * ldn, 3 * 64 * ldn, 3 * 2 * 301, 3 * 304, 70, 300, ldn]]
    # exactly two of three equal items
    for budget in (2 * one, 3 * one - 1):
        p = plan(exe, L, max_w, budget, [n] * 3)
        assert [c[:2] for c in p["chunks"]] == [[0, 2], [2, 1]]
        assert p["chunks"][0][2:4] == [2 * 13 * 70 * ldn, 2 * 64 * ldn] and p["chunks"][1][2:4] == [13 * 70 * ldn, 64 * ldn]
    # smaller than every item: one item per chunk, however large the item
    for budget in (1, one - 1):
        p = plan(exe, L, max_w, budget, [n, 40, n])
        assert [c[:2] for c in p["chunks"]] == [[0, 1], [1, 1], [2, 1]]
    # first fails at the last item
    lens = [40, 129, 300, 13, 257]
    total = sum(item_bytes(m, L, max_w) for m in lens)
    assert [c[:2] for c in plan(exe, L, max_w, total, lens)["chunks"]] == [[0, 5]]
    p = plan(exe, L, max_w, total - 1, lens)
    assert [c[:2] for c in p["chunks"]] == [[0, 4], [4, 1]]
    assert p["chunks"][0][6:] == [70, 300, 304] and p["chunks"][1][6:] == [70, 257, 272]
    assert p["chunks"][0][4:6] == [2 * (41 + 130 + 301 + 14), 48 + 144 + 304 + 16]
    # a result does not depend on the chunks: the offsets are those of one chunk
    assert p["items"] == plan(exe, L, max_w, total, lens)["items"]


def test_a_chunk_is_cut_at_the_grid_dimension(exe):
    p = plan(exe, 5, 1, 0, [3] * 65537)
    assert [c[:2] for c in p["chunks"]] == [[0, 65535], [65535, 2]]


def test_the_sizes_of_eight_times_a_million_letters_are_size_t(exe):
    n, L, max_w = 10 ** 6, 1000, 15
    ldn, one = 1000016, item_bytes(n, L, max_w)
    assert one == 13000208000 * 8 + 64 * ldn * 8 > 2 ** 36
    p = plan(exe, L, max_w, 0, [n] * 8)                     # an item is larger than the default budget of 16 GiB: a chunk each
    assert p["head"] == [8, L, max_w, 8 * 10 ** 9, 8 * n * max_w, 8]
    for k, item in enumerate(p["items"]):
        assert item == [k, n, 1000, ldn, 1000016000, 13000208000, 10 ** 9, 2000002, n * max_w, 64 * ldn, k * 10 ** 9, k * n * max_w, one]
    assert p["chunks"] == [[k, 1, 13000208000, 64 * ldn, 2000002, 1000016, 1000, n, ldn] for k in range(8)]
    p = plan(exe, L, max_w, 8 * one, [n] * 8)
    assert p["chunks"] == [[0, 8, 8 * 13000208000, 8 * 64 * ldn, 8 * 2000002, 8 * 1000016, 1000, n, ldn]]
    assert p["chunks"][0][2] * 8 > 2 ** 39 and p["items"][7][10] * 8 > 2 ** 32   # neither fits 32 bits, nor do the bytes of an offset
