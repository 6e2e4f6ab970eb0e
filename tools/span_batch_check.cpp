// span_batch_check.cpp -- stand-alone host program around the plan of a batch of span folds (span_batch_plan in
// ractip_amd/csrc/span_fold.{h,cpp}; the launcher is in mccaskill_span.hip).  No GPU, no HIP; meant to be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/span_batch_check.cpp \
//       ractip_amd/csrc/span_fold.cpp -o span_batch_check
//
//   span_batch_check L MAX_W BUDGET [ITEM ..]    ITEM: a length, or "null" for a NULL sequence (of length 5).  No ITEM: count = 0.
//   span_batch_check L MAX_W BUDGET nullseqs     the array of sequences is NULL (count 2)
//   span_batch_check L MAX_W BUDGET nulllens     the array of lengths is NULL (count 2)
//
// prints "err CODE TEXT" as span_batch_plan answers, or
//   ok COUNT L MAX_W BAND UP CHUNKS
//   item K n Le ldn table tables band ext up gaps band_at up_at bytes      (one line per item)
//   single K n Le ldn table tables band ext up gaps                        (the same item through span_check / span_acc_check)
//   chunk FIRST COUNT tables gaps ext letters max_Le max_n max_ldn         (one line per chunk)
// tests/test_span_batch_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "span_fold.h"

using namespace rh::host;

int main(int argc, char** argv)
{
    if (argc < 4) {
        std::fprintf(stderr, "usage: span_batch_check L MAX_W BUDGET [ITEM .. | nullseqs | nulllens]\n");
        return 2;
    }
    const int L = std::atoi(argv[1]), max_w = std::atoi(argv[2]);
    const size_t budget = (size_t)std::strtoull(argv[3], nullptr, 10);
    const std::string letters(1, 'A');   // the plan reads nothing of a sequence but whether it is NULL
    std::vector<const char*> seqs;
    std::vector<int> lens;
    bool null_seqs = false, null_lens = false;
    for (int a = 4; a < argc; a++) {
        if (!std::strcmp(argv[a], "nullseqs")) { null_seqs = true; continue; }
        if (!std::strcmp(argv[a], "nulllens")) { null_lens = true; continue; }
        const bool null = !std::strcmp(argv[a], "null");
        seqs.push_back(null ? nullptr : letters.c_str());
        lens.push_back(null ? 5 : std::atoi(argv[a]));
    }
    if (null_seqs || null_lens) { seqs.assign(2, letters.c_str()); lens.assign(2, 5); }
    SpanBatchPlan B;
    std::string why;
    const int rc = span_batch_plan(null_seqs ? nullptr : seqs.data(), null_lens ? nullptr : lens.data(), (int)seqs.size(), L, max_w, budget, &B, &why);
    if (rc) { std::printf("err %d %s\n", rc, why.c_str()); return 0; }
    std::printf("ok %d %d %d %zu %zu %zu\n", B.count, B.L, B.max_w, B.band, B.up, B.chunks.size());
    for (int k = 0; k < B.count; k++) {
        const SpanBatchItem& I = B.items[(size_t)k];
        std::printf("item %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", k, I.P.n, I.P.Le, I.P.ldn, I.P.table, I.P.tables, I.P.band, I.P.ext, I.Q.up, I.Q.gaps,
                    I.band_at, I.up_at, I.bytes);
        SpanPlan P;
        SpanAccPlan Q;
        if (span_check(seqs[(size_t)k], lens[(size_t)k], L, &P, &why) || span_acc_check(P, max_w, &Q, &why)) { std::printf("single %d err %s\n", k, why.c_str()); continue; }
        std::printf("single %d %d %d %zu %zu %zu %zu %zu %zu %zu\n", k, P.n, P.Le, P.ldn, P.table, P.tables, P.band, P.ext, Q.up, Q.gaps);
    }
    for (const SpanChunk& C : B.chunks)
        std::printf("chunk %d %d %zu %zu %zu %zu %d %d %zu\n", C.first, C.count, C.tables, C.gaps, C.ext, C.letters, C.max_Le, C.max_n, C.max_ldn);
    return 0;
}
