// span_fold.cpp -- the argument checks and the sizes of rh_span_fold, rh_span_fold_acc and rh_span_fold_batch (span_fold.h).  Host only: no HIP, no context.
#include "span_fold.h"

#include <limits>

#include "../../include/ractip_hot.h"

namespace rh::host {

static int reject(std::string* why, const std::string& text) { *why = text; return RH_ERR_ARG; }

// a * b into *out, false where the product does not fit a size_t
static bool mul(size_t a, size_t b, size_t* out)
{
    if (a != 0 && b > std::numeric_limits<size_t>::max() / a) return false;
    *out = a * b;
    return true;
}

int span_check(const char* seq, int n, int max_span, SpanPlan* P, std::string* why, int n_tables)
{
    if (!seq) return reject(why, "span fold: the sequence is NULL");
    if (n < 1) return reject(why, "span fold: the sequence has length " + std::to_string(n) + " (must be >= 1)");
    if (max_span < 2) return reject(why, "span fold: max_span " + std::to_string(max_span) + " (must be >= 2)");
    if (n > std::numeric_limits<int>::max() - 2 * kSpanLine) return reject(why, "span fold: the length " + std::to_string(n) + " overflows the row pitch");
    SpanPlan S;
    S.n = n; S.L = max_span;
    S.Le = n < max_span ? n : max_span;
    S.ldn = ((size_t)n + 1 + kSpanLine - 1) / kSpanLine * kSpanLine;
    S.ext = 2 * ((size_t)n + 1);
    size_t bytes = 0;
    const bool fits = mul((size_t)S.Le, S.ldn, &S.table) && mul(S.table, (size_t)n_tables, &S.tables) && mul(S.tables, sizeof(double), &bytes) &&
                      mul((size_t)n, (size_t)S.Le, &S.band) && mul(S.band, sizeof(double), &bytes);
    if (!fits) return reject(why, "span fold: the tables of " + std::to_string(n) + " letters at max_span " + std::to_string(max_span) + " overflow size_t");
    *P = S;
    return RH_OK;
}

int span_acc_check(const SpanPlan& P, int max_w, SpanAccPlan* A, std::string* why)
{
    if (max_w < 1 || max_w > kSpanAccMaxW)
        return reject(why, "span fold: max_w " + std::to_string(max_w) + " (must be 1.." + std::to_string(kSpanAccMaxW) + ")");
    SpanAccPlan S;
    S.max_w = max_w;
    size_t bytes = 0;
    const bool fits = mul((size_t)P.n, (size_t)max_w, &S.up) && mul(S.up, sizeof(double), &bytes) &&
                      mul(P.ldn, (size_t)(2 * kSpanGapRows), &S.gaps) && mul(S.gaps, sizeof(double), &bytes);
    if (!fits) return reject(why, "span fold: the accessibilities of " + std::to_string(P.n) + " letters at max_w " + std::to_string(max_w) + " overflow size_t");
    if (max_w == 1) S.gaps = 0;
    *A = S;
    return RH_OK;
}

// a + b into *out, false where the sum does not fit a size_t
static bool add(size_t a, size_t b, size_t* out)
{
    if (b > std::numeric_limits<size_t>::max() - a) return false;
    *out = a + b;
    return true;
}

int span_batch_plan(const char* const* seqs, const int* n, int count, int max_span, int max_w, size_t budget, SpanBatchPlan* B, std::string* why, int n_tables)
{
    const std::string who = "span fold batch: ";
    if (count < 1) return reject(why, who + "the batch has " + std::to_string(count) + " items (must be >= 1)");
    if (!seqs) return reject(why, who + "the array of sequences is NULL");
    if (!n) return reject(why, who + "the array of lengths is NULL");
    if (max_span < 2) return reject(why, who + "max_span " + std::to_string(max_span) + " (must be >= 2)");
    if (max_w < 1 || max_w > kSpanAccMaxW) return reject(why, who + "max_w " + std::to_string(max_w) + " (must be 1.." + std::to_string(kSpanAccMaxW) + ")");
    if (budget == 0) budget = kSpanBatchBytes;
    SpanBatchPlan S;
    S.count = count; S.L = max_span; S.max_w = max_w;
    S.items.resize((size_t)count);
    for (int k = 0; k < count; k++) {
        SpanBatchItem& I = S.items[(size_t)k];
        std::string text;
        int rc = span_check(seqs[k], n[k], max_span, &I.P, &text, n_tables);
        if (!rc) rc = span_acc_check(I.P, max_w, &I.Q, &text);
        // (the single call's reason behind its "span fold: ")
        if (rc) return reject(why, who + "item " + std::to_string(k) + ": " + text.substr(text.rfind("span fold: ", 0) == 0 ? 11 : 0));
        I.band_at = S.band; I.up_at = S.up;
        size_t doubles = 0, bytes = 0;
        const bool fits = add(S.band, I.P.band, &S.band) && mul(S.band, sizeof(double), &bytes) && add(S.up, I.Q.up, &S.up) && mul(S.up, sizeof(double), &bytes) &&
                          add(I.P.tables, I.Q.gaps, &doubles) && mul(doubles, sizeof(double), &I.bytes);
        if (!fits) return reject(why, who + "item " + std::to_string(k) + ": the results of the items up to it overflow size_t");
    }
    size_t used = 0;   // bytes of the open chunk
    for (int k = 0; k < count; k++) {
        const SpanBatchItem& I = S.items[(size_t)k];
        size_t with = 0;
        const bool open = !S.chunks.empty() && S.chunks.back().count < kSpanChunkItems && add(used, I.bytes, &with) && with <= budget;
        if (!open) { S.chunks.emplace_back(); S.chunks.back().first = k; with = I.bytes; }
        used = with;
        SpanChunk& C = S.chunks.back();
        C.count++;
        C.tables += I.P.tables; C.gaps += I.Q.gaps;   // (below `used`, which fits)
        C.ext += I.P.ext;
        C.letters += ((size_t)I.P.n + 2 + 15) & ~(size_t)15;
        if (I.P.Le > C.max_Le) C.max_Le = I.P.Le;
        if (I.P.n > C.max_n) C.max_n = I.P.n;
        if (I.P.ldn > C.max_ldn) C.max_ldn = I.P.ldn;
    }
    *B = std::move(S);
    return RH_OK;
}

}  // namespace rh::host
