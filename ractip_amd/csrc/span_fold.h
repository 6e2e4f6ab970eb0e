// span_fold.h -- the host plan and the exterior recurrence of span-limited folding (rh_span_fold, rh_span_fold_acc; kernels in
// mccaskill_span.hip).
// Plain C++ (no HIP needed): tools/span_fold_check.cpp runs both on the CPU.
//
// Definition.  Inputs: n letters, max_span = L >= 2, Le = min(L, n).  The ensemble is that of rh_fold under the context's Vienna-BL
// model (1.8 semantics, BL* tables or a parameter file), unknown letters and end letters included, with one restriction: letters
// a < b (1-based) may pair only if b - a < L.  With L >= n it is the ensemble of rh_fold.  It is ONE ensemble of the whole sequence,
// with one log Z -- not the window average of rh_local_fold.
//
// Band tables.  Cell (i, d), 1 <= i <= n-1-d, is the pair of letters (i, i+d+1) (FC and its copies) or the letters i+1 .. i+d as a
// part of a multiloop (FM1, FMS, FM): [d * ldn + i], 0 <= d < Le, ldn >= n+1 padded to whole 128-byte lines.  A pair needs d + 1 < L,
// so the rows d < Le hold every cell of the ensemble.  Scaling as in mccaskill_vlin.hip: an inside value over len letters is stored
// times lam^len, lam = exp(-s), the weights come from the context's VLinModel.  The outside tables are stored divided by Z and times
// lam^-len, which the same weights carry from cell to cell: the posterior FC~ x FCo^ needs no global factor.
//
// Exterior sums.  F5i[j] (letters 1..j) and F5o[j] (letters j+1..n) over 20000 letters leave the double range under every single
// scale exponent as soon as the free energy is spread unevenly, so they are kept as logarithms gi[j] = log F5i[j], go[j] = log F5o[j]:
//     F5i[j] = F5i[j-1] + sum_k F5i[k] FCA(k+1, d),   d = j-k-2, 0 <= d < Le   (pair (k+1, j), FCA = FCA~ exp(s d))
//     F5o[k] = F5o[k+1] + sum_j F5o[j] FCA(k+1, d)
// in blocks of kSpanBlock = 64 consecutive entries, one lane per entry, relative to the last entry in front of the block (g_ref):
//   A  lane l sums the terms whose other end lies in front of the block, exp(g[..] - g_ref + s d) FCA~: the ratios are at most 1 and
//      at least 1/Z of a stretch of Le letters, which the band tables hold anyway.  kSpanWaves wavefronts share the work: wavefront w
//      adds the rows d = w, w + kSpanWaves, .. in ascending order, the partial sums are added in the order of the wavefronts;
//   B  the entries of the block follow one after the other as ratios R_l = F5[entry l] / F5[ref] >= 1, each from R_{l-1}, A_l and the
//      terms R_m FCA inside the block (m <= l-2), which lane m holds and the butterfly of wsum (dev_util.h) adds; g = g_ref + log R_l.
// A ratio stays below Z of 64 letters.  log Z = gi[n].  The exterior term of FCo^(i, d) is exp(gi[i-1] + go[i+d+1] - log Z + s d)
// times the stem weight.
//
// The CONTRAfold model (rh_set_span_contrafold; kernels in mccaskill_span_cf.hip).  The same definition over the ensemble of rh_fold on
// a CONTRAfold context (the derivations the inside recurrences of InferenceEngine.ipp count), a pair needing complementary letters and
// b - a < L; unknown letters are code 4, as in the batch path.  Band tables as above with the weights of LinModel (lin_model.h):
// FC FCX FCM FCA FM1 FM and FCO FCOX FMO FM1O FM2O, kSpanCfTables in all.  The exterior passes above take an unpaired step of
// weight 1, CONTRAfold's carries exp(eu), eu = external_unpaired.  With F5i'[j] = F5i[j] exp(-eu j) and F5o'[k] = F5o[k] exp(-eu (n-k))
// the factor moves into the cell: both recurrences hold for F5' over the table
//     FCA(k+1, d) = FC x base_pair x junction_a x exp(external_paired - eu (d + 2))        (FCM, the multiloop's stem, times ext_w(d))
// which is what the CONTRAfold inside sweep writes where the passes read (kSpanExtTable), so the passes run unchanged on gi = log F5i',
// go = log F5o'.  log Z = gi[n] + n eu.  F5i[i-1] F5o[j+1] / Z = exp(gi[i-1] + go[j+1] - gi[n]) exp(-eu (d + 2)): the exterior term of
// FCo^(i, d) is span_ext_outer times the same ext_w(d).
// Region accessibility under the CONTRAfold model (max_w > 1 with rh_set_region_accessibility on; kernels in
// mccaskill_span_cf_acc.hip): kSpanCfAccTables more band tables behind the eleven -- the hairpin suffix sums, the chain's S and its
// two vectors -- so a call is sized with span_cf_tables(max_w) tables.  The exterior term of a run a..b is
// exp(gi[a-1] + go[b] - gi[n]): F5i[a-1] exp(eu len) F5o[b] / Z with the three exp(eu ..) factors of F5' adding up to exp(eu n).
#pragma once
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "constraint_prepass.h"

#if defined(__HIPCC__)
#define RH_SF_HD __host__ __device__ inline
#else
#define RH_SF_HD inline
#endif

namespace rh::host {

constexpr int kSpanBlock = 64;        // entries per block of an exterior pass = lanes of its wavefront
constexpr int kSpanWaves = 16;        // wavefronts of an exterior pass: phase A row d belongs to wavefront d % kSpanWaves
constexpr int kSpanInside = 7;        // band tables of the inside sweep: FC FCX FCB FCA FM1 FMS FM
constexpr int kSpanOutside = 6;       // ... of the outside sweep: FCO FCOX FCOB FMSO FM1O FM2O
constexpr int kSpanTables = kSpanInside + kSpanOutside;   // band tables of an item under the Vienna-BL model
constexpr int kSpanCfTables = 11;     // ... under the CONTRAfold model: FC FCX FCM FCA FM1 FM, FCO FCOX FMO FM1O FM2O
constexpr int kSpanCfAccTables = 4;   // ... more for its region accessibility (max_w > 1): hairpin sums R, the chain's S, two A
constexpr int span_cf_tables(int max_w) { return max_w > 1 ? kSpanCfTables + kSpanCfAccTables : kSpanCfTables; }   // of a call, for span_check
constexpr int kSpanLine = 16;         // doubles per 128-byte line

struct SpanPlan {
    int n = 0, L = 0;          // as asked for
    int Le = 0;                // min(L, n): rows of the band tables, row pitch of bp_band
    size_t ldn = 0;            // row pitch of the band tables
    size_t table = 0;          // doubles of one band table = Le * ldn
    size_t tables = 0;         // doubles of all of them: n_tables of the model's sweeps
    size_t band = 0;           // doubles of bp_band = n * Le
    size_t ext = 0;            // doubles of gi and go together = 2 (n + 1)
};

// RH_OK with *P filled, or RH_ERR_ARG with the reason in *why; reads nothing of seq but whether it is NULL.  Sizes are size_t
// throughout (n = 1e6, L = 1000: 1e9 doubles per table); a size that does not fit is rejected.  n_tables: the band tables of the
// model's sweeps (kSpanTables, kSpanCfTables), so that an item is sized, and a batch chunked, by the bytes its model really uses.
int span_check(const char* seq, int n, int max_span, SpanPlan* P, std::string* why, int n_tables = kSpanTables);

// ---- region accessibility up[i][w] on the same ensemble (rh_span_fold_acc; kernels in mccaskill_span.hip)
constexpr int kSpanAccMaxW = 64;      // widest region, the range of rh_set_max_w
constexpr int kSpanGapRows = 32;      // rows of one side of the gap-sum buffer: gap lengths 1..30 at their own index

struct SpanAccPlan {
    int max_w = 0;             // as asked for
    size_t up = 0;             // doubles of up = n * max_w
    size_t gaps = 0;           // doubles of the gap sums GL and GR = 2 * kSpanGapRows * ldn; 0 at max_w = 1, which needs none
};

// The sizes of the accessibility stage over a checked plan: RH_OK with *A filled, or RH_ERR_ARG with the reason in *why.
int span_acc_check(const SpanPlan& P, int max_w, SpanAccPlan* A, std::string* why);

// ---- batches of span folds (rh_span_fold_batch): item k is the single call on (seqs[k], n[k]) at the batch's one max_span and max_w.
// The results of all items lie one behind the other in the batch's own buffers (band_at, up_at; log Z at the item's index); the band
// tables and gap sums are scratch and are laid out per CHUNK: greedy runs of consecutive items whose tables and gap sums together
// fit the byte budget (a chunk always holds at least one item, however large), at most kSpanChunkItems of them (a grid dimension).
constexpr size_t kSpanBatchBytes = (size_t)16 << 30;   // default budget of a chunk: a setting, not a tuned value
constexpr int kSpanChunkItems = 65535;

struct SpanBatchItem {
    SpanPlan P;
    SpanAccPlan Q;
    size_t band_at = 0, up_at = 0;   // doubles in front of the item in the batch's bp_band and up buffers
    size_t bytes = 0;                // of its tables and gap sums: what the budget counts
};

struct SpanChunk {
    int first = 0, count = 0;        // items first .. first + count - 1
    size_t tables = 0, gaps = 0;     // doubles of the chunk's tables and gap sums, item after item
    size_t ext = 0;                  // doubles of its gi and go
    size_t letters = 0;              // bytes of its letter codes: n + 2 per item, padded to 16
    int max_Le = 0, max_n = 0;
    size_t max_ldn = 0;
};

struct SpanBatchPlan {
    int count = 0, L = 0, max_w = 0;
    std::vector<SpanBatchItem> items;
    std::vector<SpanChunk> chunks;
    size_t band = 0, up = 0;         // doubles of all bands and of all up tables
};

// RH_OK with *B filled, or RH_ERR_ARG with the reason in *why (an item's reason names the item).  budget = 0: kSpanBatchBytes.
int span_batch_plan(const char* const* seqs, const int* n, int count, int max_span, int max_w, size_t budget, SpanBatchPlan* B, std::string* why,
                    int n_tables = kSpanTables);

// ---- structure constraints (rh_span_fold_constrained, rh_span_fold_batch_constrained): letters a < b may pair only if b - a < L AND
// allow_pair(a, b, n, ch, P, enc) of constraint_prepass.h holds.  There is no n x n mask: the sweeps test a pair on the packed records
// of its two letters (ConsRec, allow_pair_rec).  Both functions are in span_cons.cpp, which needs constraint_prepass.cpp.
//
// One item's constraint: the pre-pass, the forced pairs against L, the records.  RH_OK with rec holding n + 2 records (letters
// 0 .. n+1; those of 0 and n+1 restrict nothing) and *restricts saying whether any pair of the band is excluded at all -- a NULL
// constraint, or one of '.' and '|' only, restricts nothing and the caller runs the unconstrained kernels' path on it.
// RH_ERR_ARG with the reason in *why: the pre-pass's own (unbalanced brackets, a bracket pair of non-complementary letters), a
// matched bracket pair (a, b) with b - a >= L, a sequence of 2^30 letters or more.  seq, n and max_span have passed span_check.
int span_cons_records(const char* seq, int n, const char* cons, int max_span, std::vector<ConsRec>* rec, bool* restricts, std::string* why);

// The constraints of a batch over a plan that span_batch_plan accepted: recs[k] as above for item k, left empty where the item's
// constraint restricts nothing (cons or cons[k] NULL included).  An item's reason names the item.
int span_cons_batch(const char* const* seqs, const int* n, int count, const char* const* cons, int max_span, std::vector<std::vector<ConsRec>>* recs, std::string* why);

// ---- the exterior passes: what the kernel and the CPU check share.  dir 0: gi, entries ascending from 1; dir 1: go, entries
// descending from n-1.  Block b holds the entries span_ext_entry(dir, n, b, l), l = 0..63 (those inside 0..n).
RH_SF_HD int span_ext_blocks(int n) { return (n + kSpanBlock - 1) / kSpanBlock; }
RH_SF_HD int span_ext_entry(int dir, int n, int b, int l) { return dir == 0 ? 1 + b * kSpanBlock + l : n - 1 - b * kSpanBlock - l; }
// the pair of entry `at` with d letters inside: the other entry it reads and the column of its cell in row d
RH_SF_HD int span_ext_other(int dir, int at, int d) { return dir == 0 ? at - 2 - d : at + 2 + d; }
RH_SF_HD int span_ext_col(int dir, int at, int d) { return dir == 0 ? at - 1 - d : at + 1; }
// largest d of entry `at` whose other entry exists
RH_SF_HD int span_ext_dmax(int dir, int n, int Le, int at) { const int room = dir == 0 ? at - 2 : n - at - 2; return room < Le - 1 ? room : Le - 1; }
// phase A: the first row of lane l (entry l of the block) that wavefront w adds: the smallest d >= max(0, l - 1) with d % kSpanWaves = w
RH_SF_HD int span_ext_first(int l, int w) { const int lo = l >= 1 ? l - 1 : 0; return lo + ((w - lo) % kSpanWaves + kSpanWaves) % kSpanWaves; }
// phase A: one term; g_k the logarithm at the other entry, sd = s * d, fca = FCA~ of the cell (0: the pair does not exist)
RH_SF_HD double span_ext_term(double g_k, double g_ref, double sd, double fca) { return fca != 0.0 ? fca * exp(g_k - g_ref + sd) : 0.0; }
// phase B: the ratio of entry l from the one before, its phase-A sum and the sum of its terms inside the block
RH_SF_HD double span_ext_ratio(double r_prev, double a, double inner) { return r_prev + (a + inner); }
RH_SF_HD double span_ext_log(double g_ref, double ratio) { return g_ref + log(ratio); }
// the exterior term of FCo^ (before the stem weight): F5i[i-1] F5o[j+1] / Z x lam^-d
RH_SF_HD double span_ext_outer(double gi_left, double go_right, double logz, double sd) { return exp(gi_left + go_right - logz + sd); }

// A whole pass on the CPU, lane by lane in the kernel's order.  fca(d, col) is FCA~ of cell (col, d); g has n + 1 entries.
template <class Fca>
inline void span_ext_pass_host(int dir, int n, int Le, double s, double* g, Fca&& fca)
{
    g[dir == 0 ? 0 : n] = 0.0;
    double g_ref = 0.0;
    for (int b = 0; b < span_ext_blocks(n); b++) {
        double A[kSpanBlock], R[kSpanBlock];
        static double T[kSpanBlock][kSpanBlock];
        bool on[kSpanBlock];
        for (int l = 0; l < kSpanBlock; l++) {
            const int at = span_ext_entry(dir, n, b, l);
            on[l] = at >= 0 && at <= n;
            double acc = 0.0;
            for (int w = 0; w < kSpanWaves && on[l]; w++) {
                const int dmax = span_ext_dmax(dir, n, Le, at);
                double part = 0.0;
                for (int d = span_ext_first(l, w); d <= dmax; d += kSpanWaves)
                    part += span_ext_term(g[span_ext_other(dir, at, d)], g_ref, s * (double)d, fca(d, span_ext_col(dir, at, d)));
                acc = w == 0 ? part : acc + part;
            }
            A[l] = acc;
        }
        // T[l][m]: the term of entry l whose other end is entry m of the block, d = l - m - 2
        for (int m = 0; m < kSpanBlock; m++)
            for (int l = 0; l < kSpanBlock; l++) {
                const int d = l - m - 2, at = span_ext_entry(dir, n, b, l);
                T[l][m] = (d >= 0 && d < Le && on[l]) ? fca(d, span_ext_col(dir, at, d)) * exp(s * (double)d) : 0.0;
            }
        double r = 1.0;
        for (int l = 0; l < kSpanBlock && on[l]; l++) {
            double v[kSpanBlock], u[kSpanBlock];
            for (int m = 0; m < kSpanBlock; m++) v[m] = m <= l - 2 ? R[m] * T[l][m] : 0.0;
            for (int o = kSpanBlock / 2; o > 0; o >>= 1) {
                for (int m = 0; m < kSpanBlock; m++) u[m] = v[m] + v[m ^ o];
                for (int m = 0; m < kSpanBlock; m++) v[m] = u[m];
            }
            r = span_ext_ratio(r, A[l], v[0]);
            R[l] = r;
            g[span_ext_entry(dir, n, b, l)] = span_ext_log(g_ref, r);
        }
        g_ref = span_ext_log(g_ref, r);
    }
}

}  // namespace rh::host
