// mccaskill_span_cf.hip -- the sweeps of span-limited folding under the CONTRAfold model (rh_set_span_contrafold; definition, tables
// and the exterior representation: span_fold.h; descriptor, launcher and the kernels both models share: span_kernels.h,
// mccaskill_span.hip).
//
// The recurrences are those of mccaskill_lin.hip (FC, FM1, FM, FM2 = sum FM1 x FM, the pull-form outside, posterior = FC~ x FCo^) in
// scaled linear space on band tables of Le rows: every term whose enclosing or enclosed pair would lie in a row d >= Le is dropped.
// The organisation is that of span_inside_diag / span_outside_diag: one launch per diagonal, one lane per cell, 64 consecutive cells
// of a diagonal per wavefront, so every operand is a contiguous row segment; the sums of a cell are plain loops of at most Le terms
// (the single-branch shapes: at most 496 taps over FCX rows, their weights by scalar loads).  Every launch writes its whole row,
// zeros where no cell exists, so nothing is cleared and a read only needs its row below Le and its column inside the tables.
// The outside tables are stored divided by Z and times lam^-d, which the weights of LinModel carry from cell to cell.
#include <hip/hip_runtime.h>

#include "dev_util.h"
#include "span_kernels.h"

namespace rh {

using namespace host;

// ---- inside, diagonal d: cell (i, d) is the pair of letters (i, j+1), j = i + d
__global__ __launch_bounds__(kSpanThreads) void span_cf_inside_diag(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M, int d, double ext_w)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    if (d >= A.Le || (size_t)blockIdx.x * kSpanThreads >= A.ldn) return;   // the item has no such row, or no such columns
    const size_t col = (size_t)blockIdx.x * kSpanThreads + threadIdx.x;
    if (col >= A.ldn) return;
    const int i = (int)col, n = A.n, j = i + d;
    const size_t ldn = A.ldn, ts = A.ts, at = (size_t)d * ldn + i;
    double* __restrict__ tab = A.tab;
    const bool valid = i >= 1 && i <= n - 1 - d;
    double fc = 0.0, e_in = 0.0, e_stem = 0.0, fm1v = 0.0, fmv = 0.0;
    bool bad = false;
    if (valid) {
        const uint8_t* __restrict__ s = A.s;
        const int s_im1 = s[i - 1], s_i = s[i], s_ip1 = s[i + 1], s_j = s[j], s_jp1 = s[j + 1], s_jp2 = s[j + 2];
        const bool pairable = d + 1 < A.L && pairs(s_i, s_jp1);   // the pair (i, j+1) spans d + 1 letters
        double fm2 = 0.0;
        {   // FM2[i,d] = sum_{m=1}^{d-1} FM1[m][i] * FM[d-m][i+m]
            const double* __restrict__ fm1 = tab + CF_FM1 * ts + i;
            const double* __restrict__ fm = tab + CF_FM * ts + i;
            for (int m = 1; m <= d - 1; m++) fm2 = fma(fm1[(size_t)m * ldn], fm[(size_t)(d - m) * ldn + m], fm2);
        }
        if (pairable) {
            const int idx = 25 * (5 * s_i + s_ip1) + 5 * s_jp1 + s_j;           // (i, j+1) as enclosing pair
            const int idd = 25 * (5 * s_jp1 + s_jp2) + 5 * s_i + s_im1;         // ... as enclosed pair
            const double e_bp = M->E_bp[s_i * 5 + s_jp1];
            e_in = e_bp * M->TJB[idd]; e_stem = e_bp * M->TJA[idd];
            // loops with one enclosed pair (p, q) = (i+1+l1, j-l2), cell (p, d-2-t), t = l1 + l2: the generic shapes over FCX (the stacking
            // shape, 0x1, 1x0 and 1x1 have weight 0 there), then those four with their letter-dependent weights
            double g = 0.0;
            const int tmax = d - 2 < kMaxSingle ? d - 2 : kMaxSingle;
            for (int t = 2; t <= tmax; t++) {
                const double* __restrict__ w = M->shape_w + t * (t + 1) / 2;
                const double* __restrict__ x = tab + CF_FCX * ts + (size_t)(d - 2 - t) * ldn + i + 1;
                for (int l1 = 0; l1 <= t; l1++) g = fma(w[l1], x[l1], g);
            }
            double sp = 0.0, st = 0.0;
            if (d >= 3) {
                const double* __restrict__ x = tab + CF_FCX * ts + (size_t)(d - 3) * ldn + i + 1;
                sp = M->w01 * M->E_b01[s_j] * x[0] + M->w10 * M->E_b10[s_ip1] * x[1];
                if (d >= 4) sp += M->w11 * M->E_11[s_ip1 * 5 + s_j] * tab[CF_FCX * ts + (size_t)(d - 4) * ldn + i + 2];
            }
            if (d >= 2) st = tab[CF_FC * ts + (size_t)(d - 2) * ldn + i + 1] * M->lam2 * M->TST[idx];
            const double hp = d >= kMinHairpin ? A.hplen[d] : 0.0;
            fc = M->TJB[idx] * (g + sp + hp) + st + fm2 * M->TJA[idx] * M->e_mpmb;
            if (!(fc == fc) || fc > kSpanHuge || (fc != 0.0 && fc < kSpanTiny)) bad = true;
        }
        if (d >= 2) {
            fm1v = tab[CF_FCM * ts + (size_t)(d - 2) * ldn + i + 1] * M->w_mp2 + tab[CF_FM1 * ts + (size_t)(d - 1) * ldn + i + 1] * M->w_mu;
            fmv = fm2 + tab[CF_FM * ts + (size_t)(d - 1) * ldn + i] * M->w_mu + fm1v;
            if (!(fmv == fmv) || fmv > kSpanHuge) bad = true;
        }
    }
    if (bad) { atomicOr(A.bad, 1); fc = fm1v = fmv = 0.0; }
    const double fcm = fc * e_stem;
    tab[CF_FC * ts + at] = fc;
    tab[CF_FCX * ts + at] = fc * e_in;
    tab[CF_FCM * ts + at] = fcm;
    tab[CF_FCA * ts + at] = fcm * ext_w;
    tab[CF_FM1 * ts + at] = fm1v;
    tab[CF_FM * ts + at] = fmv;
}

// ---- outside (pull form) and posterior, diagonal d
__global__ __launch_bounds__(kSpanThreads) void span_cf_outside_diag(const SpanArgs* __restrict__ items, const LinModel* __restrict__ M, int d, double ext_w)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    if (d >= A.Le || (size_t)blockIdx.x * kSpanThreads >= A.ldn) return;
    const size_t col = (size_t)blockIdx.x * kSpanThreads + threadIdx.x;
    if (col >= A.ldn) return;
    const int i = (int)col, n = A.n, j = i + d, Le = A.Le;
    const size_t ldn = A.ldn, ts = A.ts, at = (size_t)d * ldn + i;
    double* __restrict__ tab = A.tab;
    const bool valid = i >= 1 && i <= n - 1 - d;
    double fco = 0.0, e_out = 0.0, fmo = 0.0, fm1o = 0.0, fm2o = 0.0, p = 0.0;
    bool bad = false;
    if (valid) {
        const uint8_t* __restrict__ s = A.s;
        const int s_im1 = s[i - 1], s_i = s[i], s_ip1 = s[i + 1], s_j = s[j], s_jp1 = s[j + 1], s_jp2 = s[j + 2];
        const bool pairable = d + 1 < A.L && pairs(s_i, s_jp1);
        if (d >= 2) {
            const int emax = Le - 1 - d;
            double sm = 0.0, s1 = 0.0;
            {   // FMo[i,d] = sum_e FM2o[d+e][i-e] * FM1[e][i-e]: the part (i-e .. i] in front of this one
                const int e1 = i - 1 < emax ? i - 1 : emax;
                const double* __restrict__ x = tab + CF_FM2O * ts + (size_t)d * ldn + i;
                const double* __restrict__ y = tab + CF_FM1 * ts + i;
                for (int e = 1; e <= e1; e++) sm = fma(x[(size_t)e * ldn - e], y[(size_t)e * ldn - e], sm);
            }
            {   // FM1o[i,d] += sum_e FM2o[d+e][i] * FM[e][j]: the part (j .. j+e] behind this one
                const int e1 = n - 1 - j < emax ? n - 1 - j : emax;
                const double* __restrict__ x = tab + CF_FM2O * ts + (size_t)d * ldn + i;
                const double* __restrict__ y = tab + CF_FM * ts + j;
                for (int e = 1; e <= e1; e++) s1 = fma(x[(size_t)e * ldn], y[(size_t)e * ldn], s1);
            }
            const bool up = d + 1 < Le;   // (a cell of row d+1 that does not exist holds 0, column 0 included)
            fmo = sm + (up ? tab[CF_FMO * ts + (size_t)(d + 1) * ldn + i] : 0.0) * M->w_mu;
            fm1o = s1 + fmo + (up ? tab[CF_FM1O * ts + (size_t)(d + 1) * ldn + i - 1] : 0.0) * M->w_mu;
        }
        double e_tja = 0.0;
        if (pairable) {
            const int idx = 25 * (5 * s_i + s_ip1) + 5 * s_jp1 + s_j;
            const int idd = 25 * (5 * s_jp1 + s_jp2) + 5 * s_i + s_im1;
            e_out = M->TJB[idx]; e_tja = M->TJA[idx];
            const double e_bp = M->E_bp[s_i * 5 + s_jp1];
            const double ext = span_ext_outer(A.gi[i - 1], A.go[j + 1], A.gi[n], A.sc * (double)d) * ext_w;
            const double multi = d + 2 < Le ? tab[CF_FM1O * ts + (size_t)(d + 2) * ldn + i - 1] * M->w_mp2 : 0.0;
            // enclosing pairs (io, jo+1) = (i-1-l1, j+2+l2), cell (io, d+2+t); a cell that does not exist holds 0, column 0 included
            double g = 0.0;
            for (int t = 2; t <= kMaxSingle && d + 2 + t < Le; t++) {
                const double* __restrict__ w = M->shape_w + t * (t + 1) / 2;
                const double* __restrict__ x = tab + CF_FCOX * ts + (size_t)(d + 2 + t) * ldn + i - 1;
                const int l1e = t < i - 1 ? t : i - 1;
                for (int l1 = 0; l1 <= l1e; l1++) g = fma(w[l1], x[-l1], g);
            }
            double sp = 0.0, st = 0.0;
            if (d + 3 < Le) {
                const double* __restrict__ x = tab + CF_FCOX * ts + (size_t)(d + 3) * ldn + i - 1;
                sp = M->w01 * M->E_b01[s_jp2] * x[0];
                if (i >= 2) sp += M->w10 * M->E_b10[s_im1] * x[-1];
                if (i >= 2 && d + 4 < Le) sp += M->w11 * M->E_11[s_im1 * 5 + s_jp2] * tab[CF_FCOX * ts + (size_t)(d + 4) * ldn + i - 2];
            }
            if (d + 2 < Le) st = tab[CF_FCO * ts + (size_t)(d + 2) * ldn + i - 1] * M->lam2 * M->TST[25 * (5 * s_im1 + s_i) + 5 * s_jp2 + s_jp1];
            fco = e_bp * (M->TJA[idd] * (ext + multi) + M->TJB[idd] * (g + sp)) + st;
            p = fco * tab[CF_FC * ts + at];
            if (!(p == p) || !(fco == fco) || p > 1e300 || fco > 1e300) { bad = true; p = 0.0; fco = 0.0; }
            p = p > 1.0 ? 1.0 : (p < 0.0 ? 0.0 : p);
        }
        fm2o = fmo + fco * e_tja * M->e_mpmb;
        if (!(fm2o == fm2o) || fm2o > 1e300 || !(fm1o == fm1o) || fm1o > 1e300) { bad = true; fm2o = fm1o = fmo = 0.0; }
    }
    if (bad) atomicOr(A.bad, 1);
    tab[CF_FCO * ts + at] = fco;
    tab[CF_FCOX * ts + at] = fco * e_out;
    tab[CF_FMO * ts + at] = fmo;
    tab[CF_FM1O * ts + at] = fm1o;
    tab[CF_FM2O * ts + at] = fm2o;
    // bp_band[(i-1) * Le + d+1] = P(i, i+d+1); the lanes 1..n cover every row of the band, 0 where the pair runs off the end
    if (i >= 1 && i <= n && d + 1 < Le) A.band[(size_t)(i - 1) * Le + d + 1] = p;
}

__global__ void span_cf_logz(const SpanArgs* __restrict__ items, int count, double eu)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const SpanArgs A = items[k];
    span_global(A.logz)[0] = span_global(A.gi)[A.n] + (double)A.n * eu;
}

}  // namespace rh
