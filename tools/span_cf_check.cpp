// span_cf_check.cpp -- stand-alone host program around what span folds under the CONTRAfold model add to the host side of
// ractip_amd/csrc/span_fold.{h,cpp}: the plans sized by the model's table count, and the exterior passes on a table that carries the
// unpaired step's weight (span_fold.h).  No GPU, no HIP; meant to be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/span_cf_check.cpp \
//       ractip_amd/csrc/span_fold.cpp -o span_cf_check
//
//   span_cf_check plan MODEL L MAX_W BUDGET N ..     MODEL: vienna | contrafold | default (the call without a table count)
//       ok COUNT CHUNKS
//       item K n Le ldn table tables band ext bytes            (one line per item; the same item through span_check must agree)
//       chunk FIRST COUNT tables
//   span_cf_check ext N LE S FILE                    FILE: LE rows of N + 2 doubles, row d column i = FCA~ of cell (i, d), binary
//       gi[N] go[0]                                  (%.17g) of span_ext_pass_host in both directions
// tests/test_span_cf_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "span_fold.h"

using namespace rh::host;

static int plan(int argc, char** argv)
{
    const std::string model = argv[2];
    const int L = std::atoi(argv[3]), max_w = std::atoi(argv[4]);
    const size_t budget = (size_t)std::strtoull(argv[5], nullptr, 10);
    const std::string letters(1, 'A');   // the plan reads nothing of a sequence but whether it is NULL
    std::vector<const char*> seqs;
    std::vector<int> lens;
    for (int a = 6; a < argc; a++) { seqs.push_back(letters.c_str()); lens.push_back(std::atoi(argv[a])); }
    const int tables = model == "contrafold" ? kSpanCfTables : kSpanTables;
    SpanBatchPlan B;
    std::string why;
    const int rc = model == "default" ? span_batch_plan(seqs.data(), lens.data(), (int)seqs.size(), L, max_w, budget, &B, &why)
                                      : span_batch_plan(seqs.data(), lens.data(), (int)seqs.size(), L, max_w, budget, &B, &why, tables);
    if (rc) { std::printf("err %d %s\n", rc, why.c_str()); return 0; }
    std::printf("ok %d %zu\n", B.count, B.chunks.size());
    for (int k = 0; k < B.count; k++) {
        const SpanBatchItem& I = B.items[(size_t)k];
        SpanPlan P;
        const int rs = model == "default" ? span_check(seqs[(size_t)k], lens[(size_t)k], L, &P, &why) : span_check(seqs[(size_t)k], lens[(size_t)k], L, &P, &why, tables);
        if (rs || P.tables != I.P.tables || P.table != I.P.table || P.ldn != I.P.ldn || P.Le != I.P.Le) { std::printf("item %d differs from its single plan\n", k); return 1; }
        std::printf("item %d %d %d %zu %zu %zu %zu %zu %zu\n", k, I.P.n, I.P.Le, I.P.ldn, I.P.table, I.P.tables, I.P.band, I.P.ext, I.bytes);
    }
    for (const SpanChunk& C : B.chunks) std::printf("chunk %d %d %zu\n", C.first, C.count, C.tables);
    return 0;
}

static int ext(char** argv)
{
    const int n = std::atoi(argv[2]), Le = std::atoi(argv[3]);
    const double s = std::atof(argv[4]);
    const size_t ld = (size_t)n + 2;
    std::vector<double> fca((size_t)Le * ld);
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(fca.data(), sizeof(double), fca.size(), f) != fca.size()) { std::fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    std::fclose(f);
    std::vector<double> gi((size_t)n + 1), go((size_t)n + 1);
    const auto cell = [&](int d, int col) { return fca[(size_t)d * ld + (size_t)col]; };
    span_ext_pass_host(0, n, Le, s, gi.data(), cell);
    span_ext_pass_host(1, n, Le, s, go.data(), cell);
    std::printf("%.17g %.17g\n", gi[(size_t)n], go[0]);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 6 && !std::strcmp(argv[1], "plan")) return plan(argc, argv);
    if (argc == 6 && !std::strcmp(argv[1], "ext")) return ext(argv);
    std::fprintf(stderr, "usage: span_cf_check plan MODEL L MAX_W BUDGET N .. | span_cf_check ext N LE S FILE\n");
    return 2;
}
