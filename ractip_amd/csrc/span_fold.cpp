// span_fold.cpp -- the argument checks and the sizes of rh_span_fold and rh_span_fold_acc (span_fold.h).  Host only: no HIP, no context.
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

int span_check(const char* seq, int n, int max_span, SpanPlan* P, std::string* why)
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
    const bool fits = mul((size_t)S.Le, S.ldn, &S.table) && mul(S.table, (size_t)(kSpanInside + kSpanOutside), &S.tables) && mul(S.tables, sizeof(double), &bytes) &&
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

}  // namespace rh::host
