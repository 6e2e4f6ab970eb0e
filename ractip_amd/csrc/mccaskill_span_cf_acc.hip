// mccaskill_span_cf_acc.hip -- region accessibility up[i][w] of span folds under the CONTRAfold model (rh_span_fold_acc and
// rh_span_fold_batch at max_w > 1 on a context with rh_set_span_contrafold AND rh_set_region_accessibility; launcher: span_attempt in
// mccaskill_span.hip; declarations: span_kernels.h).
//
// up[(a-1) max_w + w] = Z(letters a .. b = a+w forbidden to pair) / Z over the derivations of the span ensemble (span_fold.h).  The
// five sources of mccaskill_acc.hip, on the band tables the sweeps of mccaskill_span_cf.hip leave: cell (i, d) is (i, j = i + d),
// d < Le, a cell that does not exist holds 0.  With len = w + 1:
//   exterior   exp(gi[a-1] + go[b] - gi[n])                      (the external_unpaired factors cancel: gi, go are logs of F5')
//   hairpin    sum_{i < a, j >= b, j - i < Le} FCOX(i, j) hplen[j - i]                 = sum_{i < a} R[b - i][i], R the suffix sums
//              over d of one column (CFA_R; FM is read by the chain, so R has a table of its own)
//   one pair   the gap sums of the loops with one enclosed pair, GL[l][i] (letters i+1 .. i+l the 5' gap of outer 5' letter i) and
//              GR[l][j] (letters j-l+1 .. j the 3' gap), outer spans below Le, turned into suffix sums over l by span_acc_gsuf:
//              sum_{i = b-30}^{a-1} GL[b - i][i] + sum_{j = b}^{a+29} GR[j - a + 1][j]
//   multi, leading letters of a branch   w_mu^len sum_j FM1O(a-1, j) FM1(b, j), j - (a-1) < Le
//   multi, trailing letters   the chain of mccaskill_acc.hip in the band: S(k, k') = delta + FM1(k, k') + sum_m FM1(k, m) S(m, k')
//              for k' - k < Le (CFA_S, diagonal by diagonal like FM2), A_0[b][k] = w_mu FMO(k, b), A_j = w_mu A_{j-1} S as banded
//              products (cell (k', b - k'); k from b - Le + 1 to k'), term of width j + 1 = sum_k' A_j[b][k'] FM(k', b - 1 - j).
//              A_0 is FMO times a constant, so the first link reads FMO and two tables (CFA_A0, CFA_A1) hold the rest in turn.
// Inside tables carry lam^len, outside tables lam^-len / Z and the weights of LinModel their own lam: every product above is a
// probability, whatever the exponent of the attempt.
//
// One lane per cell or per region, lanes over consecutive columns, so every operand of a sum is a contiguous row segment; the sums
// are plain loops of at most Le terms in a fixed order.  Every launch writes all it owns (zeros where no cell exists), nothing is
// cleared, and the only atomic is the flag.  Column 0 is the width-1 call's 1 - row sums, summed as span_finish sums it.
#include <hip/hip_runtime.h>

#include "dev_util.h"
#include "span_kernels.h"

namespace rh {

using namespace host;

// ---- R[d][p] = sum_{d' >= d} FCOX(p, d') hplen[d'] (d' >= kMinHairpin; FCOX is 0 where the pair cannot form).  One lane per column.
__global__ __launch_bounds__(kSpanThreads) void span_cf_acc_hp(const SpanArgs* __restrict__ items)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    if ((size_t)blockIdx.x * kSpanThreads >= A.ldn) return;
    const size_t col = (size_t)blockIdx.x * kSpanThreads + threadIdx.x;
    if (col >= A.ldn) return;
    const size_t ldn = A.ldn;
    const double* __restrict__ fcox = A.tab + CF_FCOX * A.ts + col;
    double* __restrict__ R = A.tab + CFA_R * A.ts + col;
    double run = 0.0;
    for (int d = A.Le - 1; d >= 0; d--) {
        if (d >= kMinHairpin) run = fma(fcox[(size_t)d * ldn], A.hplen[d], run);
        R[(size_t)d * ldn] = run;
    }
}

namespace {

// One thread's gap sum (cf_acc_gaps of mccaskill_acc.hip in the band): own gap of l letters on `side` (0: 5', x = i; 1: 3', x = j),
// the outer pairs (i, j) by growing span d < Le.  The inner cells of one step are a window over the other side's lengths that slides
// by one cell per step and lives in registers: a step loads the outer cell and the one cell that enters.  The three shapes whose
// weight depends on the letters have weight 0 in the filter and are added per step.
template <int NT> __device__ __forceinline__ double cfa_gap_walk(const SpanArgs& A, const LinModel* __restrict__ M, int side, int l, int x)
{
    const int T = kMaxSingle - l, n = A.n;   // the other side holds 0 .. T letters
    const size_t ldn = A.ldn;
    const double* __restrict__ FCX = A.tab + CF_FCX * A.ts;
    const double* __restrict__ FCOX = A.tab + CF_FCOX * A.ts;
    const uint8_t* __restrict__ s = A.s;
    double wgt[NT], win[NT];
#pragma unroll
    for (int lo = 0; lo < NT; lo++) {
        const int l1 = side ? lo : l, l2 = side ? l : lo, t = l + lo;
        wgt[lo] = (lo <= T && !(l1 <= 1 && l2 <= 1)) ? M->shape_w[t * (t + 1) / 2 + l1] : 0.0;
        win[lo] = 0.0;
    }
    int dmax = side ? x - 1 : n - 1 - x;   // outer pair (i, j): 1 <= i, j <= n-1
    if (dmax > A.Le - 1) dmax = A.Le - 1;
    double acc = 0.0;
    for (int d = l + 2; d <= dmax; d++) {
        const int i = side ? x - d : x, j = i + d;
#pragma unroll
        for (int lo = NT - 1; lo > 0; lo--) win[lo] = win[lo - 1];
        win[0] = FCX[(size_t)(d - 2 - l) * ldn + i + 1 + (side ? 0 : l)];   // the other side empty: cell (i+1, j-1-l) resp. (i+1+l, j-1)
        double inner = 0.0;
#pragma unroll
        for (int lo = 0; lo < NT; lo++) inner = fma(wgt[lo], win[lo], inner);
        if (l == 1) {   // (uniform) 0x1 / 1x0 and 1x1: the other side holds 0 or 1 letters
            const int s_ip1 = s[i + 1], s_j = s[j];
            inner = fma(side ? M->w01 * M->E_b01[s_j] : M->w10 * M->E_b10[s_ip1], win[0], inner);
            inner = fma(M->w11 * M->E_11[s_ip1 * 5 + s_j], win[1], inner);
        }
        acc = fma(FCOX[(size_t)d * ldn + i], inner, acc);
    }
    return acc;
}

}  // namespace

// ---- gap sums into A.gaps[(side * kSpanGapRows + l) * ldn + x], x = 1..n (0 where no loop exists); blockIdx.y = side * 30 + l - 1
__global__ __launch_bounds__(128) void span_cf_acc_gaps(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M)
{
    const SpanArgs A = span_item(items, blockIdx.z);
    if ((int)(blockIdx.x * 128) + 1 > A.n) return;   // no letter of the item in this workgroup
    const int x = blockIdx.x * 128 + threadIdx.x + 1;
    if (x > A.n) return;
    const int side = blockIdx.y / kMaxSingle, l = blockIdx.y % kMaxSingle + 1;   // (uniform)
    const int taps = kMaxSingle - l + 1;
    double acc = 0.0;
    if (x <= A.n - 1) {
        if (taps <= 8) acc = cfa_gap_walk<8>(A, M, side, l, x);
        else if (taps <= 16) acc = cfa_gap_walk<16>(A, M, side, l, x);
        else if (taps <= 24) acc = cfa_gap_walk<24>(A, M, side, l, x);
        else acc = cfa_gap_walk<32>(A, M, side, l, x);
    }
    A.gaps[((size_t)side * kSpanGapRows + l) * A.ldn + x] = acc;
}

// ---- column 0: up[i0 * max_w] = 1 - sum_j P(i0+1, j), the sum of span_finish term for term.  One wavefront per letter.
__global__ __launch_bounds__(kSpanBlock) void span_cf_acc_col0(const SpanArgs* __restrict__ items)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    const int i0 = blockIdx.x, lane = threadIdx.x, n = A.n, Le = A.Le;
    if (i0 >= n) return;
    double acc = 0.0;
    for (int dd = 1 + lane; dd < Le; dd += kSpanBlock) {
        if (i0 + dd < n) acc += A.band[(size_t)i0 * Le + dd];
        if (i0 - dd >= 0) acc += A.band[(size_t)(i0 - dd) * Le + dd];
    }
    acc = wsum(acc);
    if (lane == 0) {
        const double u = 1.0 - acc;
        A.up[(size_t)i0 * A.max_w] = u < 0.0 ? 0.0 : u;
    }
}

// ---- every term but the chain: one THREAD per (letter a, width w = blockIdx.y + 1), lanes over a.  Writes the sum unclamped
// (span_cf_acc_close of the same width adds the chain's term and clamps); a run that passes letter n holds 0.
__global__ __launch_bounds__(256) void span_cf_acc_final(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M)
{
    const SpanArgs A = span_item(items, blockIdx.z);
    if ((int)(blockIdx.x * 256) + 1 > A.n) return;
    const int a = blockIdx.x * 256 + threadIdx.x + 1, w = blockIdx.y + 1, n = A.n, Le = A.Le;
    if (a > n) return;
    const int b = a + w, len = w + 1;
    double* __restrict__ up = A.up + (size_t)(a - 1) * A.max_w + w;
    if (b > n) { *up = 0.0; return; }
    const size_t ldn = A.ldn, ts = A.ts;
    double acc = exp(A.gi[a - 1] + A.go[b] - A.gi[n]);
    if (a >= 2 && b <= n - 1) {
        {   // hairpin: outer 5' letters i < a in the band of b
            const double* __restrict__ R = A.tab + CFA_R * ts;
            double h = 0.0;
            for (int i = a - 1; i >= 1 && i >= b - Le + 1; i--) h += R[(size_t)(b - i) * ldn + i];
            acc += h;
        }
        const double* __restrict__ gl = A.gaps;                                   // suffix sums over the gap length
        const double* __restrict__ gr = A.gaps + (size_t)kSpanGapRows * ldn;
        for (int i = a - 1; i >= 1 && i >= b - kMaxSingle; i--) acc += gl[(size_t)(b - i) * ldn + i];
        for (int j = b; j <= n - 1 && j <= a - 1 + kMaxSingle; j++) acc += gr[(size_t)(j - a + 1) * ldn + j];
        double m = 0.0;
        {   // the run leads a branch: FM1O(a-1, j) x FM1(b, j), rows j - (a-1) < Le
            const double* __restrict__ x = A.tab + CF_FM1O * ts + (a - 1);
            const double* __restrict__ y = A.tab + CF_FM1 * ts + b;
            const int j1 = n - 1 < a - 2 + Le ? n - 1 : a - 2 + Le;
            for (int j = b + 2; j <= j1; j++) m = fma(x[(size_t)(j - a + 1) * ldn], y[(size_t)(j - b) * ldn], m);
        }
        double mu_len = 1.0;
        for (int k = 0; k < len; k++) mu_len *= M->w_mu;
        acc += m * mu_len;
    }
    *up = acc;
}

// ---- S, diagonal d: S(k, k) = 1, S(k, k+1) = 0, S(k, k+d) = FM1(k, k+d) + sum_{e=2}^{d-2} FM1(k, k+e) S(k+e, k+d)
__global__ __launch_bounds__(kSpanThreads) void span_cf_acc_sdiag(const SpanArgs* __restrict__ items, int d)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    if (d >= A.Le || (size_t)blockIdx.x * kSpanThreads >= A.ldn) return;
    const size_t col = (size_t)blockIdx.x * kSpanThreads + threadIdx.x;
    if (col >= A.ldn) return;
    const int k = (int)col;
    const size_t ldn = A.ldn;
    const double* __restrict__ fm1 = A.tab + CF_FM1 * A.ts + k;
    double* __restrict__ S = A.tab + CFA_S * A.ts + k;
    double v = 0.0;
    if (k >= 1 && k <= A.n - 1 - d) {
        if (d == 0) v = 1.0;
        else if (d >= 2) {
            double sum = 0.0;
            for (int e = 2; e <= d - 2; e++) sum = fma(fm1[(size_t)e * ldn], S[(size_t)(d - e) * ldn + e], sum);
            v = fm1[(size_t)d * ldn] + sum;
            if (!(v <= kSpanHuge)) { atomicOr(A.bad, 1); v = 0.0; }
        }
    }
    S[(size_t)d * ldn] = v;
}

// ---- one link of the chain: dst(k', d') = scale sum_{e >= 0} src(k'-e, d'+e) S(k'-e, e), b = k' + d' <= n-1, d' >= 3, d' + e < Le.
// first: src is FMO and scale w_mu^2 (A_0 = w_mu FMO); else scale w_mu.  One lane per cell, blockIdx.y strides the rows.
__global__ __launch_bounds__(kSpanThreads) void span_cf_acc_link(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M, int src_t, int dst_t, int first)
{
    const SpanArgs A = span_item(items, blockIdx.z);
    if ((size_t)blockIdx.x * kSpanThreads >= A.ldn) return;
    const size_t col = (size_t)blockIdx.x * kSpanThreads + threadIdx.x;
    if (col >= A.ldn) return;
    const int kp = (int)col, n = A.n, Le = A.Le;
    const size_t ldn = A.ldn;
    const double* __restrict__ src = A.tab + (size_t)src_t * A.ts + kp;
    const double* __restrict__ S = A.tab + CFA_S * A.ts + kp;
    double* __restrict__ dst = A.tab + (size_t)dst_t * A.ts + kp;
    const double scale = first ? M->w_mu * M->w_mu : M->w_mu;
    for (int dp = blockIdx.y; dp < Le; dp += gridDim.y) {
        double v = 0.0;
        if (kp >= 1 && dp >= 3 && kp + dp <= n - 1) {
            const int e1 = kp - 1 < Le - 1 - dp ? kp - 1 : Le - 1 - dp;
            for (int e = 0; e <= e1; e++) v = fma(src[(size_t)(dp + e) * ldn - e], S[(size_t)e * ldn - e], v);
            v *= scale;
        }
        dst[(size_t)dp * ldn] = v;
    }
}

// ---- the chain's term of width j + 1 and the end of column j: up += sum_{e >= 2} A_j(t-e, e+j+1) FM(t-e, e), t = a - 1, b = a + j;
// flags a value that is not finite, clamps.  One thread per letter a.
__global__ __launch_bounds__(256) void span_cf_acc_close(const SpanArgs* __restrict__ items, int j, int src_t)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    if ((int)(blockIdx.x * 256) + 1 > A.n) return;
    const int a = blockIdx.x * 256 + threadIdx.x + 1, n = A.n, Le = A.Le;
    const int b = a + j, t = a - 1;
    if (a > n || b > n) return;   // (past the end: span_cf_acc_final wrote the 0)
    const size_t ldn = A.ldn;
    double m = 0.0;
    if (b <= n - 1) {
        const double* __restrict__ x = A.tab + (size_t)src_t * A.ts + t;
        const double* __restrict__ y = A.tab + CF_FM * A.ts + t;
        const int e1 = t - 1 < Le - 2 - j ? t - 1 : Le - 2 - j;
        for (int e = 2; e <= e1; e++) m = fma(x[(size_t)(e + j + 1) * ldn - e], y[(size_t)e * ldn - e], m);
    }
    double* __restrict__ up = A.up + (size_t)(a - 1) * A.max_w + j;
    const double acc = *up + m;
    if (!(acc <= 1e300)) atomicOr(A.bad, 1);
    *up = acc > 1.0 ? 1.0 : acc;
}

}  // namespace rh
