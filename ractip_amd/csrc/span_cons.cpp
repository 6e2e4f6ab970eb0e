// span_cons.cpp -- structure constraints of span folds (span_fold.h): the pre-pass per item, the forced pairs against max_span, the
// packed per-letter records.  Host only: no HIP, no context.  (A file of its own: it needs constraint_prepass.cpp, the plan does not.)
#include "span_fold.h"

#include "../../include/ractip_hot.h"

namespace rh::host {

int span_cons_records(const char* seq, int n, const char* cons, int max_span, std::vector<ConsRec>* rec, bool* restricts, std::string* why)
{
    *restricts = false;
    rec->clear();
    if (!cons) return RH_OK;
    if (n > kConsRecMaxN) {
        *why = "span fold: a constraint over " + std::to_string(n) + " letters does not fit the per-letter records (at most " + std::to_string(kConsRecMaxN) + ")";
        return RH_ERR_ARG;
    }
    const size_t len = (size_t)n + 2;
    std::vector<uint8_t> ch(len, (uint8_t)'.');
    std::vector<int> P(len, 0), enc(len, 0);
    std::string text;
    if (!constraint_prepass(seq, n, cons, ch.data(), P.data(), enc.data(), &text)) {
        *why = "span fold: " + text;
        return RH_ERR_ARG;
    }
    for (int a = 1; a <= n; a++)
        if (P[(size_t)a] > a && P[(size_t)a] - a >= max_span) {
            *why = "span fold: the constraint pairs letters " + std::to_string(a) + " and " + std::to_string(P[(size_t)a]) + ", which max_span " +
                   std::to_string(max_span) + " excludes (a pair (a, b) needs b - a < max_span)";
            return RH_ERR_ARG;
        }
    rec->resize(len);
    for (size_t k = 0; k < len; k++) {
        (*rec)[k] = cons_rec_pack(ch[k], P[k], enc[k]);
        if ((*rec)[k].p & (kConsRecDown | kConsRecUp)) *restricts = true;   // (a matched bracket carries one of the two as well)
    }
    if (!*restricts) rec->clear();
    return RH_OK;
}

int span_cons_batch(const char* const* seqs, const int* n, int count, const char* const* cons, int max_span, std::vector<std::vector<ConsRec>>* recs, std::string* why)
{
    recs->assign((size_t)count, {});
    for (int k = 0; cons && k < count; k++) {
        bool restricts = false;
        std::string text;
        if (int rc = span_cons_records(seqs[k], n[k], cons[k], max_span, &(*recs)[(size_t)k], &restricts, &text)) {
            *why = "span fold batch: item " + std::to_string(k) + ": " + text.substr(text.rfind("span fold: ", 0) == 0 ? 11 : 0);
            return rc;
        }
    }
    return RH_OK;
}

}  // namespace rh::host
