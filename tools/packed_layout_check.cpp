// packed_layout_check.cpp -- CPU check of packed_layout (ractip_amd/csrc/batch.h), the layout of the packed float image that
// rh_batch_results_packed_f32 fills.  Host only; built with the host sanitizers by tests/test_packed_layout_cpu.py.
//   packed_layout_check self                               the properties below over ragged batches, 512 and 2048 pairs of 2000 + 2000
//   packed_layout_check offsets MAX_W NSEQ n.. NPAIRS a b ..   the offsets and totals of one batch, for a restatement to compare with
// Properties, per batch: offsets ascend and are multiples of 4; block k spans exactly its tight size up to less than 4 floats of padding
// (so blocks neither overlap nor leave room for another block); the totals are the last offsets; and the bytes of the three float
// images together never exceed half of the bytes of the padded double tables rh_batch_layout describes for the same batch.
// That last bound is on the sum.  A block is padded by at most 3 floats.  up never exceeds its half (pad4(n w) <= (n + 2) w rounded up to
// even); a bp block exceeds its half, by at most 2 floats, only when the sequence is the longest of the batch and T(n) mod 4 is 1 or 2,
// and then n >= 2; an hp table leaves (n1max + 2) * ldd - pad4((n1 + 1)(n2 + 1)) >= n1 + n2 floats.  So the bound holds for every batch
// in which each sequence belongs to a pair -- every plain upload, and the indexed ones checked here; an indexed batch of very short
// sequences most of which no pair uses can exceed it by two floats per such sequence, and is not claimed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "batch.h"

using namespace rh;

struct Batch {
    std::vector<int> lens, pair_seq;
    int max_w = 1;
    int nseq() const { return (int)lens.size(); }
    int npairs() const { return (int)pair_seq.size() / 2; }
};

struct Layout {
    std::vector<size_t> bp, up, hp;
    size_t totals[3];
};

static Layout layout_of(const Batch& b)
{
    Layout L;
    L.bp.assign(b.nseq() + 1, ~(size_t)0); L.up.assign(b.nseq() + 1, ~(size_t)0); L.hp.assign(b.npairs() + 1, ~(size_t)0);
    packed_layout(b.nseq(), b.lens.data(), b.npairs(), b.pair_seq.data(), b.max_w, L.bp.data(), L.up.data(), L.hp.data(), L.totals);
    return L;
}

static int failures = 0;
#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAIL %s: ", name);                           \
            std::printf(__VA_ARGS__);                                 \
            std::printf("  [%s]\n", #cond);                           \
            failures++;                                               \
        }                                                             \
    } while (0)

// offsets of one kind against the tight sizes of its blocks
static void check_kind(const char* name, const char* kind, const std::vector<size_t>& off, const std::vector<size_t>& tight, size_t total)
{
    CHECK(off.size() == tight.size() + 1, "%s: %zu offsets for %zu blocks", kind, off.size(), tight.size());
    CHECK(off[0] == 0, "%s: first offset %zu", kind, off[0]);
    for (size_t k = 0; k < tight.size(); k++) {
        CHECK(off[k] % 4 == 0, "%s block %zu starts at %zu", kind, k, off[k]);
        CHECK(off[k + 1] >= off[k] + tight[k], "%s block %zu of %zu floats overlaps the next one (%zu -> %zu)", kind, k, tight[k], off[k], off[k + 1]);
        CHECK(off[k + 1] - off[k] - tight[k] < 4, "%s block %zu of %zu floats spans %zu", kind, k, tight[k], off[k + 1] - off[k]);
    }
    CHECK(off.back() % 4 == 0 && total == off.back(), "%s total %zu, last offset %zu", kind, total, off.back());
}

static void check_batch_layout(const char* name, const Batch& b, bool half_bound)
{
    const Layout L = layout_of(b);
    std::vector<size_t> tbp, tup, thp;
    int nmax = 0, n1max = 0, n2max = 0;
    for (int n : b.lens) {
        tbp.push_back((size_t)(n + 1) * (n + 2) / 2);
        tup.push_back((size_t)n * b.max_w);
        if (n > nmax) nmax = n;
    }
    for (int p = 0; p < b.npairs(); p++) {
        const int n1 = b.lens[b.pair_seq[2 * p]], n2 = b.lens[b.pair_seq[2 * p + 1]];
        thp.push_back(((size_t)n1 + 1) * ((size_t)n2 + 1));
        if (n1 > n1max) n1max = n1;
        if (n2 > n2max) n2max = n2;
    }
    check_kind(name, "bp", L.bp, tbp, L.totals[0]);
    check_kind(name, "up", L.up, tup, L.totals[1]);
    check_kind(name, "hp", L.hp, thp, L.totals[2]);
    if (!half_bound) return;
    // the padded double tables of the same batch (what rh_batch_layout reports: tri_stride, ld * max_w, tab_stride)
    const McBatch M = mc_layout(b.nseq(), nmax, 1);
    const DxBatch D = dx_layout(b.npairs(), n1max, n2max, seq_lds(nmax), 1);
    const size_t padded = sizeof(double) * ((M.tri_stride + (size_t)M.ld * b.max_w) * b.nseq() + D.tab_stride * b.npairs());
    const size_t packed = sizeof(float) * (L.totals[0] + L.totals[1] + L.totals[2]);
    CHECK(2 * packed <= padded, "packed %zu bytes, padded %zu bytes", packed, padded);
}

static Batch plain(const std::vector<int>& lens, int max_w)
{
    Batch b;
    b.lens = lens; b.max_w = max_w;
    for (int k = 0; k < (int)lens.size(); k++) b.pair_seq.push_back(k);
    return b;
}

static int self_check()
{
    char name[128];
    const int widths[] = {1, 2, 15, 64};
    // every single pair of 1..70 x 1..70 letters: block sizes of every residue mod 4, the smallest tables
    for (int w : widths)
        for (int n1 = 1; n1 <= 70; n1++)
            for (int n2 = 1; n2 <= 70; n2++) {
                std::snprintf(name, sizeof name, "pair %d+%d max_w %d", n1, n2, w);
                check_batch_layout(name, plain({n1, n2}, w), true);
            }
    // ragged plain batches: the shortest and the longest problem side by side
    const std::vector<std::vector<int>> ragged = {
        {1, 1, 2, 3, 5, 4, 7, 64, 65, 31, 113, 53, 130, 1},
        {2, 2, 2, 2, 2, 2},
        {500, 1, 1, 500, 3, 3},
        {2000, 1999, 17, 1, 64, 64, 109, 110},
    };
    for (int w : widths)
        for (size_t k = 0; k < ragged.size(); k++) {
            std::snprintf(name, sizeof name, "ragged %zu max_w %d", k, w);
            check_batch_layout(name, plain(ragged[k], w), true);
        }
    // indexed batches (every sequence in a pair): a sequence in both roles, a self pair, a cross product
    for (int w : widths) {
        Batch b;
        b.max_w = w; b.lens = {33, 7, 58, 20}; b.pair_seq = {0, 1, 2, 2, 1, 0, 3, 2, 1, 3};
        std::snprintf(name, sizeof name, "indexed max_w %d", w);
        check_batch_layout(name, b, true);
        Batch x;
        x.max_w = w;
        for (int k = 0; k < 64; k++) x.lens.push_back(500 - 3 * k);
        for (int q = 0; q < 32; q++) for (int t = 32; t < 64; t++) { x.pair_seq.push_back(q); x.pair_seq.push_back(t); }
        std::snprintf(name, sizeof name, "cross product max_w %d", w);
        check_batch_layout(name, x, true);
        Batch u;   // a sequence that no pair uses: the layout properties (the byte bound is not claimed, see the head of this file)
        u.max_w = w; u.lens = {5, 17, 1, 64}; u.pair_seq = {0, 1, 1, 0, 1, 1, 0, 0, 2, 1};
        std::snprintf(name, sizeof name, "indexed with an unused sequence max_w %d", w);
        check_batch_layout(name, u, false);
    }
    // 512 pairs of 2000 + 2000: 2.05e9 hp entries, 8.2e9 bytes -- past 32-bit byte offsets and close to 2^31 entries; 2048 such pairs
    // are past 2^32 entries in bp and in hp.  The totals are exact.
    {
        std::strcpy(name, "512 pairs of 2000 + 2000");
        const Batch b = plain(std::vector<int>(1024, 2000), 15);
        check_batch_layout(name, b, true);
        const Layout L = layout_of(b);
        const size_t hp1 = 2001ull * 2001ull, hp1p = (hp1 + 3) / 4 * 4, bp1 = 2001ull * 2002ull / 2, bp1p = (bp1 + 3) / 4 * 4;
        CHECK(L.totals[2] == 512 * hp1p && L.totals[2] == 2050050048ull && sizeof(float) * L.totals[2] > (1ull << 32), "hp total %zu", L.totals[2]);
        CHECK(L.totals[0] == 1024 * bp1p && L.totals[1] == 1024ull * 30000, "bp total %zu, up total %zu", L.totals[0], L.totals[1]);
        CHECK(L.hp[511] == 511 * hp1p && L.hp[300] > (1ull << 30), "hp offset of pair 511: %zu", L.hp[511]);
    }
    {
        std::strcpy(name, "2048 pairs of 2000 + 2000");
        const Batch b = plain(std::vector<int>(4096, 2000), 64);
        check_batch_layout(name, b, true);
        const Layout L = layout_of(b);
        const size_t hp1p = (2001ull * 2001ull + 3) / 4 * 4, bp1p = (2001ull * 2002ull / 2 + 3) / 4 * 4;
        CHECK(L.totals[2] == 2048 * hp1p && L.totals[2] > (1ull << 32), "hp total %zu", L.totals[2]);
        CHECK(L.totals[0] == 4096 * bp1p && L.totals[0] > (1ull << 32), "bp total %zu", L.totals[0]);
        CHECK(L.totals[1] == 4096ull * 128000, "up total %zu", L.totals[1]);
        CHECK(L.hp[2047] == 2047 * hp1p && L.bp[4095] == 4095 * bp1p, "last offsets %zu %zu", L.hp[2047], L.bp[4095]);
    }
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "self")) return self_check();
    if (argc >= 5 && !std::strcmp(argv[1], "offsets")) {
        Batch b;
        int at = 2;
        b.max_w = std::atoi(argv[at++]);
        const int ns = std::atoi(argv[at++]);
        for (int k = 0; k < ns && at < argc; k++) b.lens.push_back(std::atoi(argv[at++]));
        const int np = at < argc ? std::atoi(argv[at++]) : 0;
        for (int k = 0; k < 2 * np && at < argc; k++) b.pair_seq.push_back(std::atoi(argv[at++]));
        if ((int)b.lens.size() != ns || (int)b.pair_seq.size() != 2 * np || at != argc) { std::fprintf(stderr, "bad batch\n"); return 2; }
        for (int x : b.pair_seq) if (x < 0 || x >= ns) { std::fprintf(stderr, "bad index\n"); return 2; }
        const Layout L = layout_of(b);
        for (const std::vector<size_t>* v : {&L.bp, &L.up, &L.hp}) {
            for (size_t x : *v) std::printf("%zu ", x);
            std::printf("\n");
        }
        std::printf("%zu %zu %zu\n", L.totals[0], L.totals[1], L.totals[2]);
        return 0;
    }
    std::fprintf(stderr, "usage: packed_layout_check self | offsets MAX_W NSEQ n.. NPAIRS first second ..\n");
    return 2;
}
