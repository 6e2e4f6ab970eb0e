// span_kernels.h -- what the kernels of span-limited folding share between mccaskill_span.hip (the Vienna-BL sweeps, the exterior
// passes, the finish, the launcher) and mccaskill_span_cf.hip (the CONTRAfold sweeps): the per-item descriptor and how a kernel
// fetches it.  Definition, table layout and the exterior representation: span_fold.h.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "constraint_prepass.h"
#include "lin_model.h"
#include "span_fold.h"

namespace rh {

constexpr int kSpanThreads = 256;
constexpr double kSpanHuge = 1e280, kSpanTiny = 1e-280;   // a band cell outside them raises the flag

struct SpanArgs {
    double* tab;           // the band tables of ts doubles each, [d * ldn + i]: SP_COUNT (Vienna-BL) or kSpanCfTables (CONTRAfold) of them
    size_t ldn, ts;
    const uint8_t* s;      // letters 1..n; the model's "no nucleotide" code at 0 and n+1
    int n, Le, L;
    int max_w;             // widths of up: [n][max_w]
    const double* hplen;   // hairpin length weight x lam^d, d < Le
    double* gi;            // log F5i [n+1]
    double* go;            // log F5o [n+1]
    double* band;          // bp_band [n][Le]
    double* up;            // [n][max_w]
    double* logz;          // [1]
    int* bad;
    double sc;             // the scale exponent s of the model
    double* gaps;          // GL, GR [2][kSpanGapRows][ldn] (max_w > 1)
    const host::ConsRec* cons;   // the constraint's records of letters 0..n+1; null: the item has no constraint
};
static_assert(sizeof(SpanArgs) == 128);   // two scalar loads of 16 dwords

// The table every model's inside sweep leaves for the exterior passes (span_ext_pass reads nothing else of the tables).
constexpr int kSpanExtTable = 3;

// The CONTRAfold band tables (span_fold.h): FCM is FC times the stem weight of a multiloop branch, FCA the same times the
// exterior's own factor of the row.
enum SpanCfTable { CF_FC = 0, CF_FCX, CF_FCM, CF_FCA, CF_FM1, CF_FM, CF_FCO, CF_FCOX, CF_FMO, CF_FM1O, CF_FM2O, CF_COUNT };
static_assert(CF_FCA == kSpanExtTable && CF_COUNT == host::kSpanCfTables);
// ... and, behind them, the band tables of the CONTRAfold accessibility stage (max_w > 1): the hairpin suffix sums R, the chain's
// S and its two vectors A in turn.
enum SpanCfAccTable { CFA_R = CF_COUNT, CFA_S, CFA_A0, CFA_A1, CFA_END };
static_assert(CFA_END == host::kSpanCfTables + host::kSpanCfAccTables);

namespace {

// Every kernel runs a batch of items, a single call a batch of one: the launch hands over a device array with one SpanArgs per item
// and the item is a grid dimension (y, or z where the kernel's own grid has two), so a workgroup belongs to ONE item.  The grid spans
// the widest item of the launch; a workgroup with nothing to do for its item leaves before its first load or store besides this
// one.  The address is uniform over the workgroup and the load is the kernel's first access: the descriptor arrives by scalar loads
// and stays in scalar registers.
// A pointer that comes out of memory could point anywhere as far as the compiler knows, and every access through it would be a flat
// one (which also waits on the LDS counter); all of these point to device memory, and saying so makes the accesses global ones.
template <class T> __device__ __forceinline__ T* span_global(T* p)
{
    typedef __attribute__((address_space(1))) T* G;
    return (T*)(G)(uintptr_t)p;   // (through the integer: a pointer cast there and back would fold away)
}
__device__ __forceinline__ SpanArgs span_item(const SpanArgs* __restrict__ items, unsigned item)
{
    SpanArgs A = items[item];
    A.tab = span_global(A.tab); A.s = span_global(A.s); A.hplen = span_global(A.hplen);
    A.gi = span_global(A.gi); A.go = span_global(A.go);
    A.band = span_global(A.band); A.up = span_global(A.up); A.logz = span_global(A.logz);
    A.bad = span_global(A.bad); A.gaps = span_global(A.gaps);
    if (A.cons) A.cons = span_global(A.cons);
    return A;
}

}  // namespace

// ---- mccaskill_span_cf.hip: the CONTRAfold sweeps, one launch per diagonal d, grid (columns of the widest row / kSpanThreads, items).
// ext_w = exp(external_paired - external_unpaired (d + 2)): the exterior's factor of row d (span_fold.h).
__global__ void span_cf_inside_diag(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M, int d, double ext_w);
__global__ void span_cf_outside_diag(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M, int d, double ext_w);
// behind span_finish: log Z = gi[n] + n external_unpaired.  One thread per item.
__global__ void span_cf_logz(const SpanArgs* __restrict__ items, int count, double eu);

// ---- mccaskill_span_cf_acc.hip: the CONTRAfold accessibility stage (max_w > 1) on finished band tables; M is the attempt's model.
// grid (columns / kSpanThreads, items): the hairpin suffix sums R
__global__ void span_cf_acc_hp(const SpanArgs* __restrict__ items);
// grid (letters / 128, 2 * kMaxSingle, items): the gap sums GL, GR of the loops with one enclosed pair (then span_acc_gsuf)
__global__ void span_cf_acc_gaps(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M);
// grid (n, items), one wavefront: column 0 = 1 - the row sums of the band
__global__ void span_cf_acc_col0(const SpanArgs* __restrict__ items);
// grid (letters / 256, max_w - 1, items): exterior, hairpin, one enclosed pair, leading multiloop letters of widths 2..max_w
__global__ void span_cf_acc_final(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M);
// one launch per diagonal d, grid (columns / kSpanThreads, items): S of the chain
__global__ void span_cf_acc_sdiag(const SpanArgs* __restrict__ items, int d);
// grid (columns / kSpanThreads, rows, items): table dst_t = w_mu x table src_t x S (first: src_t is FMO, the factor w_mu^2)
__global__ void span_cf_acc_link(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M, int src_t, int dst_t, int first);
// grid (letters / 256, items): adds the chain's term of width j + 1 from table src_t = A_j to column j, flags and clamps it
__global__ void span_cf_acc_close(const SpanArgs* __restrict__ items, int j, int src_t);

}  // namespace rh
