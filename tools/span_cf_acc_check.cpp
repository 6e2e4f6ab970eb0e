// span_cf_acc_check.cpp -- stand-alone host program around the plans of span folds under the CONTRAfold model with region
// accessibility (ractip_amd/csrc/span_fold.{h,cpp}): a call at max_w > 1 is sized with the band tables of the accessibility stage
// (span_cf_tables: kSpanCfTables + kSpanCfAccTables), a call at max_w = 1 with the sweeps' eleven.  No GPU, no HIP; meant to be built
// with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/span_cf_acc_check.cpp \
//       ractip_amd/csrc/span_fold.cpp -o span_cf_acc_check
//
//   span_cf_acc_check tables                         "SWEEPS EXTRA": kSpanCfTables kSpanCfAccTables
//   span_cf_acc_check plan L MAX_W BUDGET N ..       the batch plan of a CONTRAfold context, as the launcher asks for it
//       ok COUNT CHUNKS
//       item K n Le ldn tables gaps bytes            (doubles, doubles, bytes; the same item through span_check must agree)
//       chunk FIRST COUNT tables gaps
// tests/test_cf_span_acc_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "span_fold.h"

using namespace rh::host;

static int plan(int argc, char** argv)
{
    const int L = std::atoi(argv[2]), max_w = std::atoi(argv[3]);
    const size_t budget = (size_t)std::strtoull(argv[4], nullptr, 10);
    const std::string letters(1, 'A');   // the plan reads nothing of a sequence but whether it is NULL
    std::vector<const char*> seqs;
    std::vector<int> lens;
    for (int a = 5; a < argc; a++) { seqs.push_back(letters.c_str()); lens.push_back(std::atoi(argv[a])); }
    const int tables = span_cf_tables(max_w);
    SpanBatchPlan B;
    std::string why;
    if (int rc = span_batch_plan(seqs.data(), lens.data(), (int)seqs.size(), L, max_w, budget, &B, &why, tables)) { std::printf("err %d %s\n", rc, why.c_str()); return 0; }
    std::printf("ok %d %zu\n", B.count, B.chunks.size());
    for (int k = 0; k < B.count; k++) {
        const SpanBatchItem& I = B.items[(size_t)k];
        SpanPlan P;
        SpanAccPlan Q;
        if (span_check(seqs[(size_t)k], lens[(size_t)k], L, &P, &why, tables) || span_acc_check(P, max_w, &Q, &why) || P.tables != I.P.tables || Q.gaps != I.Q.gaps) {
            std::printf("item %d differs from its single plan\n", k);
            return 1;
        }
        std::printf("item %d %d %d %zu %zu %zu %zu\n", k, I.P.n, I.P.Le, I.P.ldn, I.P.tables, I.Q.gaps, I.bytes);
    }
    for (const SpanChunk& C : B.chunks) std::printf("chunk %d %d %zu %zu\n", C.first, C.count, C.tables, C.gaps);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "tables")) { std::printf("%d %d\n", kSpanCfTables, kSpanCfAccTables); return 0; }
    if (argc >= 6 && !std::strcmp(argv[1], "plan")) return plan(argc, argv);
    std::fprintf(stderr, "usage: span_cf_acc_check tables | span_cf_acc_check plan L MAX_W BUDGET N ..\n");
    return 2;
}
