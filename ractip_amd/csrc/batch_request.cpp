// batch_request.cpp -- the checks of an upload and the shape it has (batch_request.h).  Host only: no HIP, no context.
#include "batch_request.h"

#include <algorithm>

#include "../../include/ractip_hot.h"
#include "batch.h"
#include "constraint_prepass.h"

namespace rh::host {

static int reject(std::string* why, int code, const std::string& text) { *why = text; return code; }

// an array whose entries are all NULL is no constraint
static const char* const* some(const char* const* a, int count)
{
    for (int k = 0; a && k < count; k++)
        if (a[k]) return a;
    return nullptr;
}

int check_model(const BatchRequest& r, bool vienna, std::string* why)
{
    const int per_pair = r.first ? 0 : r.ns / 2;
    if (!vienna && (some(r.fold_cons, r.ns) || some(r.joint_cons, per_pair) || some(r.share_first, r.ns) || some(r.share_second, r.ns)))
        return reject(why, RH_ERR_UNSUPPORTED, "structure constraints apply to the Vienna-BL model only (RactIP::contrafold takes none)");
    return RH_OK;
}

// the shares of every distinct sequence in both roles, then per pair only what the partner decides: O(open brackets)
static int check_shares(const BatchRequest& r, BatchShape* S, std::string* why)
{
    SharePass& SH = S->share;
    for (int role = 0; role < 2; role++)
        for (int k = 0; k < r.ns; k++) {
            const char* const* from = role ? r.share_second : r.share_first;
            const size_t sh = (size_t)role * r.ns + k;
            std::vector<int> open;
            if (from && from[k] &&
                !share_prepass(r.seqs[k], r.lens[k], from[k], role, &SH.L.ch[sh * S->lds], &SH.L.P[sh * S->lds], &SH.L.enc[sh * S->lds], &open, &SH.why[sh]))
                open.clear();   // (reported below if a pair puts the sequence in this role; its row is not read otherwise)
            SH.pos.insert(SH.pos.end(), open.begin(), open.end());
            SH.off.push_back((int)SH.pos.size());
        }
    for (int p = 0; p < S->np; p++) {
        const int a = S->pair_seq[2 * (size_t)p], b = r.ns + S->pair_seq[2 * (size_t)p + 1];
        for (int sh : {a, b})
            if (!SH.why[sh].empty()) return reject(why, RH_ERR_ARG, "pair " + std::to_string(p) + ": " + SH.why[sh]);
        std::string w;
        if (!joint_pair_check(r.seqs[a], SH.pos.data() + SH.off[a], SH.off[a + 1] - SH.off[a], r.seqs[b - r.ns], SH.pos.data() + SH.off[b],
                              SH.off[b + 1] - SH.off[b], &w))
            return reject(why, RH_ERR_ARG, "pair " + std::to_string(p) + ": " + w);
    }
    return RH_OK;
}

int check_batch(const BatchRequest& r, bool vienna, BatchShape* S, std::string* why)
{
    if (int rc = check_model(r, vienna, why)) return rc;
    const int ns = r.ns;
    if (ns <= 0) return reject(why, RH_ERR_ARG, "empty batch");
    *S = BatchShape();
    for (int k = 0; k < ns; k++) {
        if (r.lens[k] < 1) return reject(why, RH_ERR_ARG, "sequence " + std::to_string(k) + " has length " + std::to_string(r.lens[k]) + " (must be >= 1)");
        if (!r.seqs[k]) return reject(why, RH_ERR_ARG, "sequence " + std::to_string(k) + " is NULL");
        S->nmax = std::max(S->nmax, r.lens[k]);
    }
    S->indexed = r.with_dx && r.first && r.second;
    if (r.with_dx && !S->indexed && (ns & 1)) return reject(why, RH_ERR_ARG, "duplex batch needs an even number of sequences");
    S->np = S->indexed ? r.npairs : r.with_dx ? ns / 2 : 0;
    if (S->indexed && S->np < 1) return reject(why, RH_ERR_ARG, "indexed batch of " + std::to_string(S->np) + " pairs (must be >= 1)");
    S->pair_seq.resize(2 * (size_t)S->np);
    for (int p = 0; p < S->np; p++) {   // lengths over the pairs, through the index
        const int a = S->indexed ? r.first[p] : 2 * p, b = S->indexed ? r.second[p] : 2 * p + 1;
        if (a < 0 || a >= ns || b < 0 || b >= ns)
            return reject(why, RH_ERR_ARG, "pair " + std::to_string(p) + " = (" + std::to_string(a) + ", " + std::to_string(b) + "): index outside [0, " + std::to_string(ns) + ")");
        S->pair_seq[2 * (size_t)p] = a; S->pair_seq[2 * (size_t)p + 1] = b;
        S->n1max = std::max(S->n1max, r.lens[a]); S->n2max = std::max(S->n2max, r.lens[b]);
        S->cut_min = p == 0 ? r.lens[a] : std::min(S->cut_min, r.lens[a]);
        S->cut_max = p == 0 ? r.lens[a] : std::max(S->cut_max, r.lens[a]);
    }
    const int lds = S->lds = seq_lds(S->nmax), co_lds = S->co_lds = seq_lds(S->n1max + S->n2max);
    // which constraints apply (check_model has left none under another model): fold constraints to the folds, per-pair strings to the
    // pairs of a plain batch, shares to those of an indexed one
    const char* const* fold = r.with_mc ? some(r.fold_cons, ns) : nullptr;
    const char* const* joint = r.with_dx && !S->indexed ? some(r.joint_cons, S->np) : nullptr;
    S->has_fold = fold != nullptr; S->has_joint = joint != nullptr;
    S->has_shares = S->indexed && (some(r.share_first, ns) || some(r.share_second, ns));
    S->fold = ConsPass(fold ? ns : 0, lds);
    S->joint = ConsPass(joint ? S->np : 0, co_lds);
    S->share = SharePass(S->has_shares ? ns : 0, lds);
    std::string w;
    for (int k = 0; fold && k < ns; k++)
        if (!constraint_prepass(r.seqs[k], r.lens[k], fold[k], &S->fold.ch[(size_t)k * lds], &S->fold.P[(size_t)k * lds], &S->fold.enc[(size_t)k * lds], &w))
            return reject(why, RH_ERR_ARG, "sequence " + std::to_string(k) + ": " + w);
    for (int p = 0; joint && p < S->np; p++) {   // over the concatenation s1+s2 (one string of n1+n2 characters per pair)
        const std::string both = std::string(r.seqs[2 * p], r.lens[2 * p]) + std::string(r.seqs[2 * p + 1], r.lens[2 * p + 1]);
        if (!constraint_prepass(both.c_str(), (int)both.size(), joint[p], &S->joint.ch[(size_t)p * co_lds], &S->joint.P[(size_t)p * co_lds],
                                &S->joint.enc[(size_t)p * co_lds], &w))
            return reject(why, RH_ERR_ARG, "pair " + std::to_string(p) + ": " + w);
    }
    if (S->has_shares)
        if (int rc = check_shares(r, S, why)) return rc;
    S->codes.assign((size_t)ns * lds, vienna ? 0 : 4);   // sentinel = the model's "no nucleotide" code
    for (int k = 0; k < ns; k++)
        for (int i = 0; i < r.lens[k]; i++) S->codes[(size_t)k * lds + 1 + i] = vienna ? vienna_code(r.seqs[k][i]) : nuc_code(r.seqs[k][i]);
    return RH_OK;
}

}  // namespace rh::host
