// span_cons_check.cpp -- stand-alone host program around the structure constraints of span folds: the packed per-letter records
// (ConsRec, allow_pair_rec in ractip_amd/csrc/constraint_prepass.h) against allow_pair on the unpacked arrays, and the checks of
// span_cons_records / span_cons_batch (ractip_amd/csrc/span_fold.h, span_cons.cpp).  No GPU, no HIP; meant to be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/span_cons_check.cpp \
//       ractip_amd/csrc/span_cons.cpp ractip_amd/csrc/span_fold.cpp ractip_amd/csrc/constraint_prepass.cpp -o span_cons_check
//
//   span_cons_check rule SEQ CONS          every pair (a, b), 0 <= a, b <= n + 1, on the records against allow_pair; the records of
//                                          span_cons_records (max_span n + 1) against cons_rec_pack.  Prints "ok N" and the n rows
//                                          a = 1..n of the allowed-pair mask as '0' / '1' over b = 1..n.
//   span_cons_check big                    n = 10^6 letters under helices, x, < and > runs all along the sequence and two brackets
//                                          that enclose nearly everything: random pairs, every forced pair and its neighbours.
//                                          Prints "ok TESTED ALLOWED MAXINDEX".
//   span_cons_check single L SEQ CONS      span_cons_records: "err CODE TEXT", or "ok RESTRICTS RECORDS"   (CONS "null": NULL)
//   span_cons_check batch L SEQ CONS ..    span_cons_batch: "err CODE TEXT", or "ok" and one "item K RECORDS" per item
//   span_cons_check batch L nullcons SEQ ..   the array of constraints is NULL
// tests/test_span_cons_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "span_fold.h"

using namespace rh::host;

static int die(const char* what, int a, int b)
{
    std::printf("FAIL %s at (%d, %d)\n", what, a, b);
    return 1;
}

struct Unpacked {
    std::vector<uint8_t> ch;
    std::vector<int> P, enc;
    std::vector<ConsRec> rec;
};

static bool unpack(const std::string& seq, const std::string& cons, Unpacked* U, std::string* why)
{
    const int n = (int)seq.size();
    U->ch.assign((size_t)n + 2, (uint8_t)'.');
    U->P.assign((size_t)n + 2, 0);
    U->enc.assign((size_t)n + 2, 0);
    if (!constraint_prepass(seq.c_str(), n, cons.c_str(), U->ch.data(), U->P.data(), U->enc.data(), why)) return false;
    U->rec.resize((size_t)n + 2);
    for (size_t k = 0; k < U->rec.size(); k++) U->rec[k] = cons_rec_pack(U->ch[k], U->P[k], U->enc[k]);
    return true;
}

// the records decide (a, b) as allow_pair does; -1: they differ
static int same(const Unpacked& U, int n, int a, int b)
{
    const bool want = allow_pair(a, b, n, U.ch.data(), U.P.data(), U.enc.data());
    const bool got = allow_pair_rec(a, b, n, U.rec[(size_t)a], U.rec[(size_t)b]);
    return want == got ? (want ? 1 : 0) : -1;
}

static int rule(const std::string& seq, const std::string& cons)
{
    const int n = (int)seq.size();
    Unpacked U;
    std::string why;
    if (!unpack(seq, cons, &U, &why)) { std::printf("err %s\n", why.c_str()); return 0; }
    for (int k = 0; k <= n + 1; k++) {
        const ConsRec r = U.rec[(size_t)k];
        if (cons_rec_partner(r) != U.P[(size_t)k] || cons_rec_enc(r) != U.enc[(size_t)k]) return die("a record does not unpack to its P and enc", k, k);
    }
    std::vector<ConsRec> rec;
    bool restricts = false;
    if (span_cons_records(seq.c_str(), n, cons.c_str(), n + 1, &rec, &restricts, &why)) return die(why.c_str(), 0, 0);
    if (restricts && (rec.size() != U.rec.size() || std::memcmp(rec.data(), U.rec.data(), sizeof(ConsRec) * rec.size()))) return die("span_cons_records packs other records", 0, 0);
    if (!restricts && !rec.empty()) return die("records without a restriction", 0, 0);
    std::vector<std::string> rows((size_t)n, std::string((size_t)n, '0'));
    bool any = false;
    for (int a = 0; a <= n + 1; a++)
        for (int b = 0; b <= n + 1; b++) {
            const int v = same(U, n, a, b);
            if (v < 0) return die("the records and allow_pair differ", a, b);
            if (v) rows[(size_t)a - 1][(size_t)b - 1] = '1';
            if (!v && a >= 1 && a < b && b <= n) any = true;
        }
    if (any && !restricts) return die("a pair is excluded and restricts does not say so", 0, 0);
    std::printf("ok %d\n", n);
    for (const std::string& r : rows) std::printf("%s\n", r.c_str());
    return 0;
}

static int big()
{
    const int n = 1000000;
    std::string seq((size_t)n, 'A'), cons((size_t)n, '.');
    const auto pair = [&](int a, int b) { cons[(size_t)a - 1] = '('; cons[(size_t)b - 1] = ')'; seq[(size_t)a - 1] = 'G'; seq[(size_t)b - 1] = 'C'; };
    pair(2, n - 1);                  // enc = 2 nearly everywhere ...
    pair(524287, 1048575 - 100000);  // ... and 524287 behind 2^19 - 1: indices that need 20 bits
    std::mt19937 rng(20261021);
    for (int at = 1000; at + 200 < n; at += 997) {
        if (at <= 524287 && at + 200 >= 524287) continue;
        if (at <= 948575 && at + 200 >= 948575) continue;
        switch (rng() % 4) {
            case 0: for (int k = 0; k < 5; k++) pair(at + k, at + 40 - k); break;
            case 1: for (int k = 0; k < 7; k++) cons[(size_t)(at + k) - 1] = 'x'; break;
            case 2: for (int k = 0; k < 4; k++) cons[(size_t)(at + k) - 1] = '<'; break;
            default: for (int k = 0; k < 4; k++) cons[(size_t)(at + k) - 1] = '>'; break;
        }
    }
    Unpacked U;
    std::string why;
    if (!unpack(seq, cons, &U, &why)) { std::printf("err %s\n", why.c_str()); return 1; }
    long tested = 0, allowed = 0;
    int max_index = 0;
    const auto test = [&](int a, int b) -> bool {
        if (a < 0 || b < 0 || a > n + 1 || b > n + 1) return true;
        const int v = same(U, n, a, b);
        tested++;
        if (v > 0) allowed++;
        return v >= 0;
    };
    for (int k = 1; k <= n; k++) {   // every forced pair and its neighbours
        const int p = U.P[(size_t)k];
        max_index = std::max(max_index, std::max(p, U.enc[(size_t)k]));
        if (p <= k) continue;
        for (int da = -1; da <= 1; da++)
            for (int db = -1; db <= 1; db++)
                if (!test(k + da, p + db)) return die("the records and allow_pair differ", k + da, p + db);
    }
    for (int t = 0; t < 2000000; t++) {   // random pairs: any two letters, and pairs within 60 letters
        const int a = (int)(rng() % (unsigned)(n + 2));
        const int b = t % 2 ? (int)(rng() % (unsigned)(n + 2)) : a + (int)(rng() % 60u);
        if (!test(a, b)) return die("the records and allow_pair differ", a, b);
    }
    if (max_index < (1 << 19)) return die("no index needs 20 bits", max_index, 0);
    std::vector<ConsRec> rec;
    bool restricts = false;
    if (span_cons_records(seq.c_str(), n, cons.c_str(), n, &rec, &restricts, &why) || !restricts) return die("span_cons_records refuses the long constraint", 0, 0);
    if (rec.size() != U.rec.size() || std::memcmp(rec.data(), U.rec.data(), sizeof(ConsRec) * rec.size())) return die("span_cons_records packs other records", 0, 0);
    std::printf("ok %ld %ld %d\n", tested, allowed, max_index);
    return 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "rule" && argc == 4) return rule(argv[2], argv[3]);
    if (mode == "big" && argc == 2) return big();
    if (mode == "single" && argc == 5) {
        const std::string seq = argv[3];
        std::vector<ConsRec> rec;
        bool restricts = false;
        std::string why;
        const int rc = span_cons_records(seq.c_str(), (int)seq.size(), std::strcmp(argv[4], "null") ? argv[4] : nullptr, std::atoi(argv[2]), &rec, &restricts, &why);
        if (rc) std::printf("err %d %s\n", rc, why.c_str());
        else std::printf("ok %d %zu\n", restricts ? 1 : 0, rec.size());
        return 0;
    }
    if (mode == "batch" && argc >= 4) {
        const bool nullcons = !std::strcmp(argv[3], "nullcons");
        std::vector<const char*> seqs, cons;
        std::vector<int> lens;
        for (int a = nullcons ? 4 : 3; a < argc; a += nullcons ? 1 : 2) {
            seqs.push_back(argv[a]);
            lens.push_back((int)std::strlen(argv[a]));
            if (!nullcons) cons.push_back(a + 1 < argc && std::strcmp(argv[a + 1], "null") ? argv[a + 1] : nullptr);
        }
        std::vector<std::vector<ConsRec>> recs;
        std::string why;
        const int rc = span_cons_batch(seqs.data(), lens.data(), (int)seqs.size(), nullcons ? nullptr : cons.data(), std::atoi(argv[2]), &recs, &why);
        if (rc) { std::printf("err %d %s\n", rc, why.c_str()); return 0; }
        std::printf("ok\n");
        for (size_t k = 0; k < recs.size(); k++) std::printf("item %zu %zu\n", k, recs[k].size());
        return 0;
    }
    std::fprintf(stderr, "usage: span_cons_check rule SEQ CONS | big | single L SEQ CONS | batch L [nullcons] SEQ [CONS] ..\n");
    return 2;
}
