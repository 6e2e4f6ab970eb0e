// mccaskill_span.hip -- span-limited folding (rh_span_fold): the McCaskill ensemble of a whole long sequence under the Vienna-BL model,
// restricted to pairs (a, b) with b - a < L.  Definition, table layout and the exterior representation: span_fold.h.
//
// The recurrences are those of mccaskill_vlin.hip for one molecule (hairpins, the interior loops within kMaxSingle, FM2 = sum FM1 x FM,
// FM1 / FMS / FM, the pull-form outside and the posterior) on band tables of Le rows: every term whose enclosing or enclosed pair
// would lie in a row d >= Le is dropped, and the exterior sums are logarithms (span_ext_pass).  One launch per diagonal, one lane per
// cell, 64 consecutive cells of a diagonal per wavefront: every operand is a contiguous row segment.  The sums of a cell are plain
// loops of at most Le terms.  Every launch writes its whole row, zeros where no cell exists, so nothing is cleared and a read only
// needs its row and column inside the tables.
// rh_span_fold_acc adds the region accessibilities up[i][w] of the same ensemble: the span_acc_* kernels behind the outside sweep.
// rh_span_fold_batch runs many sequences through the same launches: every kernel takes per-item descriptors and the item as a grid
// dimension (span_item), the exponent ladder runs per item, and the single calls are batches of one.
// rh_span_fold_constrained / rh_span_fold_batch_constrained restrict the pairs further by a structure constraint: an item's descriptor
// points to the packed per-letter records of its constraint (ConsRec, constraint_prepass.h), and the two sweeps -- the only kernels
// that decide whether a pair exists -- test a pair on the records of its two letters.
// rh_set_span_contrafold turns the same calls on for a CONTRAfold context: the launcher runs the sweeps of mccaskill_span_cf.hip between
// the exterior passes and the finish of this file, over the context's own exponent ladder (lin0, then kRungS); with
// rh_set_region_accessibility on as well it answers max_w > 1 through the stage of mccaskill_span_cf_acc.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ctx.h"
#include "constraint_prepass.h"
#include "dev_util.h"
#include "span_kernels.h"
#include "vienna_model.h"

using namespace rh;
using namespace rh::host;

namespace {

enum SpanTable { SP_FC = 0, SP_FCX, SP_FCB, SP_FCA, SP_FM1, SP_FMS, SP_FM, SP_FCO, SP_FCOX, SP_FCOB, SP_FMSO, SP_FM1O, SP_FM2O, SP_COUNT };
static_assert(SP_COUNT == kSpanTables && SP_FCA == kSpanExtTable);

// (SpanArgs, the per-item descriptor of every kernel, and span_item, which fetches it: span_kernels.h)

// The pair type of cell (i, d), the pair of letters (i, j1 = i + d + 1): 0 where the span limit or the item's constraint excludes the
// pair.  Every other kernel reaches a pair through an FC / FCo^ cell, which is 0 where the type is: the tabulated shapes skip v == 0
// and fo == 0, FCX / FCB / FCA and their outside copies are FC / FCo^ times a weight, the exterior passes read FCA, span_acc_hp skips
// FCo^ == 0, the gap sums are products of an inside and an outside cell, and the multiloop tables are sums over FCA and FCo^.
// The null test is uniform over the workgroup (the descriptor sits in scalar registers); the two 8-byte loads are contiguous along
// the diagonal.  kCons = false, the sweeps of a launch none of whose items has a constraint, compiles the test away: those sweeps
// are the code they were before constraints existed.
template <bool kCons> __device__ __forceinline__ int span_pair_type(const SpanArgs& A, int i, int j1, int d, int s_i, int s_j1)
{
    int type = d + 1 < A.L ? vienna_ptype(s_i, s_j1) : 0;   // the pair (i, j1) spans d + 1 letters
    if (kCons && A.cons && type && !allow_pair_rec(i, j1, A.n, A.cons[i], A.cons[j1])) type = 0;
    return type;
}

// the seven tabulated loop shapes (as mccaskill_vlin.hip): outer pair type t1, inner pair type t2, letters si1/sj1 next to the outer
// pair inside the loop, sp1/sq1 next to the inner pair
__device__ __forceinline__ double span_small_w(const VLinModel* L, int l1, int l2, int t1, int t2, int si1, int sj1, int sp1, int sq1)
{
    const int r2 = vienna_rtype(t2);
    const int tt = t1 * 8 + r2;
    if (l1 == 0 && l2 == 0) return L->E_stack[tt];
    if (l1 + l2 == 1) return L->E_bulge1[tt];
    if (l1 == 1 && l2 == 1) return L->E_int11[tt * 25 + si1 * 5 + sj1];
    if (l1 == 1 && l2 == 2) return L->E_int21[tt * 125 + (si1 * 5 + sq1) * 5 + sj1];
    if (l1 == 2 && l2 == 1) return L->E_int21[(r2 * 8 + t1) * 125 + (sq1 * 5 + si1) * 5 + sp1];
    return L->E_int22[tt * 625 + ((si1 * 5 + sp1) * 5 + sq1) * 5 + sj1];
}
__device__ __forceinline__ int small_l1(int k) { return (k == 2 || k == 3 || k == 4) ? 1 : (k >= 5 ? 2 : 0); }
__device__ __forceinline__ int small_l2(int k) { return (k == 1 || k == 3 || k == 5) ? 1 : ((k == 4 || k == 6) ? 2 : 0); }

// ---- inside, diagonal d: grid over the ldn columns of the row
template <bool kCons> __global__ __launch_bounds__(kSpanThreads) void span_inside_diag(const SpanArgs* __restrict__ items, const VLinModel* __restrict__ M, int d)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    if (d >= A.Le || (size_t)blockIdx.x * kSpanThreads >= A.ldn) return;   // the item has no such row, or no such columns
    const size_t col = (size_t)blockIdx.x * kSpanThreads + threadIdx.x;
    if (col >= A.ldn) return;
    const int i = (int)col, n = A.n, j = i + d;
    const size_t ldn = A.ldn, ts = A.ts, at = (size_t)d * ldn + i;
    double* __restrict__ tab = A.tab;
    const bool valid = i >= 1 && i <= n - 1 - d;
    double fc = 0.0, e_txi = 0.0, e_tau = 1.0, e_tsa = 0.0, fm1v = 0.0, fmsv = 0.0, fmv = 0.0;
    bool bad = false;
    if (valid) {
        const uint8_t* __restrict__ s = A.s;
        const int s_im1 = s[i - 1], s_i = s[i], s_ip1 = s[i + 1], s_j = s[j], s_jp1 = s[j + 1], s_jp2 = s[j + 2];
        const int type = span_pair_type<kCons>(A, i, j + 1, d, s_i, s_jp1);
        double fm2 = 0.0;
        {   // FM2[i,d] = sum_{m=1}^{d-1} FM1[m][i] * FM[d-m][i+m]
            const double* __restrict__ fm1 = tab + SP_FM1 * ts + i;
            const double* __restrict__ fm = tab + SP_FM * ts + i;
            for (int m = 1; m <= d - 1; m++) fm2 = fma(fm1[(size_t)m * ldn], fm[(size_t)(d - m) * ldn + m], fm2);
        }
        if (type) {
            const int idx = 25 * (5 * s_i + s_ip1) + 5 * s_jp1 + s_j;           // (i, j+1) seen from inside
            const int idx_raw = 25 * (5 * s_jp1 + s_jp2) + 5 * s_i + s_im1;     // seen from outside
            const double e_txo = M->TXO[idx], e_tmc = M->TMC[idx];
            e_tau = M->E_tau[type]; e_txi = M->TXI[idx_raw]; e_tsa = M->TSA[idx_raw];
            const int b_ip2 = s[i + 2 <= n + 1 ? i + 2 : n + 1], b_ip3 = s[i + 3 <= n + 1 ? i + 3 : n + 1];
            const int b_jm1 = s[j - 1 >= 0 ? j - 1 : 0], b_jm2 = s[j - 2 >= 0 ? j - 2 : 0];
            double hp = 0.0;
            if (d == 3) hp = A.hplen[d] * e_tau;
            else if (d > 3) {
                double tet = 1.0;
                if (d == 4 && s_i != 0 && s_ip1 != 0 && b_ip2 != 0 && b_ip3 != 0 && s_j != 0 && s_jp1 != 0)
                    tet = M->E_tetra[(((((s_i - 1) * 4 + (s_ip1 - 1)) * 4 + (b_ip2 - 1)) * 4 + (b_ip3 - 1)) * 4 + (s_j - 1)) * 4 + (s_jp1 - 1)];
                hp = A.hplen[d] * M->TMH[idx] * tet;
            }
            // loops with one enclosed pair (p, q) = (i+1+l1, j-l2), cell (p, d-2-t), t = l1 + l2: generic interior loops over FCX, bulges
            // of two letters and more over FCB, the seven tabulated shapes over FC
            double g = 0.0, gb = 0.0, sm = 0.0;
            const int tmax = d - 2 < kMaxSingle ? d - 2 : kMaxSingle;
            for (int t = 2; t <= tmax; t++) {
                const size_t row = (size_t)(d - 2 - t) * ldn + i + 1;
                if (t >= 4) {
                    const double* __restrict__ w = M->shape_w + t * (t + 1) / 2;
                    const double* __restrict__ x = tab + SP_FCX * ts + row;
                    for (int l1 = 1; l1 < t; l1++) g = fma(w[l1], x[l1], g);
                }
                const double* __restrict__ xb = tab + SP_FCB * ts + row;
                gb = fma(M->WB[t], xb[0] + xb[t], gb);
            }
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const int l1 = small_l1(k), l2 = small_l2(k), t = l1 + l2;
                if (d - 2 - t < 0) continue;
                const double v = tab[SP_FC * ts + (size_t)(d - 2 - t) * ldn + i + 1 + l1];
                if (v == 0.0) continue;
                const int sp = l1 == 0 ? s_ip1 : (l1 == 1 ? b_ip2 : b_ip3), spm = l1 == 0 ? s_i : (l1 == 1 ? s_ip1 : b_ip2);
                const int sq = l2 == 0 ? s_j : (l2 == 1 ? b_jm1 : b_jm2), sqp = l2 == 0 ? s_jp1 : (l2 == 1 ? s_j : b_jm1);
                sm = fma(v, span_small_w(M, l1, l2, type, vienna_ptype(sp, sq), s_ip1, s_j, spm, sqp), sm);
            }
            fc = e_txo * g + e_tau * gb + sm + hp + fm2 * e_tmc;
            if (!(fc == fc) || fc > kSpanHuge || (fc != 0.0 && fc < kSpanTiny)) bad = true;
        }
        if (d >= 2) {
            fm1v = tab[SP_FCA * ts + (size_t)(d - 2) * ldn + i + 1] * M->w_mp2 + tab[SP_FM1 * ts + (size_t)(d - 1) * ldn + i + 1] * M->w_mu;
            fmsv = fm1v + tab[SP_FMS * ts + (size_t)(d - 1) * ldn + i] * M->w_mu;
            fmv = fm2 + fmsv;
            if (!(fmv == fmv) || fmv > kSpanHuge) bad = true;
        }
    }
    if (bad) { atomicOr(A.bad, 1); fc = fm1v = fmsv = fmv = 0.0; }
    tab[SP_FC * ts + at] = fc;
    tab[SP_FCX * ts + at] = fc * e_txi;
    tab[SP_FCB * ts + at] = fc * e_tau;
    tab[SP_FCA * ts + at] = fc * e_tsa;
    tab[SP_FM1 * ts + at] = fm1v;
    tab[SP_FMS * ts + at] = fmsv;
    tab[SP_FM * ts + at] = fmv;
}

// ---- the exterior logarithms, one workgroup of kSpanWaves wavefronts: dir 0 writes gi[0..n] ascending, dir 1 go[n..0] descending
// (span_fold.h).  Phase A of a block is spread over the wavefronts -- wavefront w takes the rows d = w, w + kSpanWaves, .. of every
// entry, four loads in flight per lane -- as is the fill of T; phase B runs on wavefront 0.  An entry is read by the blocks behind
// the one that wrote it: the barriers of a block order them.
__global__ __launch_bounds__(kSpanBlock * kSpanWaves) void span_ext_pass(const SpanArgs* __restrict__ items, int dir)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    __shared__ double T[kSpanBlock][kSpanBlock];      // T[l][m]: the term of entry l whose other end is entry m of the block
    __shared__ double part[kSpanWaves][kSpanBlock];   // phase-A sums per wavefront
    __shared__ double esd[kSpanBlock];                // exp(s d)
    __shared__ double ref_s;
    const int w = threadIdx.x / kSpanBlock, lane = threadIdx.x % kSpanBlock, n = A.n, Le = A.Le;
    const size_t ldn = A.ldn;
    const double* __restrict__ fca = A.tab + SP_FCA * A.ts;
    double* g = dir == 0 ? A.gi : A.go;
    const double s = A.sc;
    double g_ref = 0.0;
    if (w == 0) esd[lane] = exp(s * (double)lane);
    if (threadIdx.x == 0) g[dir == 0 ? 0 : n] = 0.0;
    __syncthreads();
    const int nb = span_ext_blocks(n);
    for (int b = 0; b < nb; b++) {
        const int at = span_ext_entry(dir, n, b, lane);
        const bool on = at >= 0 && at <= n;
        // A: the terms whose other end lies in front of the block, ascending d within a wavefront
        double a = 0.0;
        if (on) {
            const int dmax = span_ext_dmax(dir, n, Le, at);
            for (int d = span_ext_first(lane, w); d <= dmax; d += 4 * kSpanWaves) {
                double gk[4], f[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int du = d + u * kSpanWaves <= dmax ? d + u * kSpanWaves : d;
                    gk[u] = g[span_ext_other(dir, at, du)];
                    f[u] = fca[(size_t)du * ldn + span_ext_col(dir, at, du)];
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (d + u * kSpanWaves <= dmax) a += span_ext_term(gk[u], g_ref, s * (double)(d + u * kSpanWaves), f[u]);
            }
        }
        part[w][lane] = a;
        // the terms inside the block: lane m fills its column, rows l = m+2 .. 63; for a row d the lanes read neighbouring cells
        for (int d = w; d < kSpanBlock; d += kSpanWaves) {
            const int l = lane + 2 + d;
            if (l >= kSpanBlock) continue;
            const int atl = span_ext_entry(dir, n, b, l);
            const bool cell = d < Le && atl >= 0 && atl <= n;
            T[l][lane] = cell ? fca[(size_t)d * ldn + span_ext_col(dir, atl, d)] * esd[d] : 0.0;
        }
        __syncthreads();
        if (w == 0) {
            a = part[0][lane];
            for (int k = 1; k < kSpanWaves; k++) a += part[k][lane];
            // B: the entries one after the other; every lane carries the running ratio, lane l keeps its own
            double r = 1.0, mine = 0.0;
            const int count = min(kSpanBlock, n - b * kSpanBlock);   // entries of this block
            for (int l = 0; l < count; l++) {
                const double inner = wsum(lane <= l - 2 ? mine * T[l][lane] : 0.0);
                r = span_ext_ratio(r, __shfl(a, l, kSpanBlock), inner);
                if (lane == l) mine = r;
            }
            if (on) g[at] = span_ext_log(g_ref, mine);
            if (lane == 0) ref_s = span_ext_log(g_ref, r);
        }
        __syncthreads();   // the entries are read by the blocks behind this one; T and part are refilled
        g_ref = ref_s;
    }
    if (threadIdx.x == 0 && !(g_ref == g_ref && g_ref < 1e300 && g_ref > -1e300)) atomicOr(A.bad, 1);
}

// ---- outside (pull form) and posterior, diagonal d
template <bool kCons> __global__ __launch_bounds__(kSpanThreads) void span_outside_diag(const SpanArgs* __restrict__ items, const VLinModel* __restrict__ M, int d)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    if (d >= A.Le || (size_t)blockIdx.x * kSpanThreads >= A.ldn) return;
    const size_t col = (size_t)blockIdx.x * kSpanThreads + threadIdx.x;
    if (col >= A.ldn) return;
    const int i = (int)col, n = A.n, j = i + d, Le = A.Le;
    const size_t ldn = A.ldn, ts = A.ts, at = (size_t)d * ldn + i;
    double* __restrict__ tab = A.tab;
    const bool valid = i >= 1 && i <= n - 1 - d;
    double fco = 0.0, e_txo = 0.0, e_tau = 1.0, fmso = 0.0, fm1o = 0.0, fm2o = 0.0, p = 0.0;
    bool bad = false;
    if (valid) {
        const uint8_t* __restrict__ s = A.s;
        const int s_im1 = s[i - 1], s_i = s[i], s_ip1 = s[i + 1], s_j = s[j], s_jp1 = s[j + 1], s_jp2 = s[j + 2];
        const int type = span_pair_type<kCons>(A, i, j + 1, d, s_i, s_jp1);
        double fmo = 0.0;
        if (d >= 2) {
            const int emax = Le - 1 - d;
            double s1 = 0.0;
            {   // FMo[i,d] = sum_e FM2o[d+e][i-e] * FM1[e][i-e]: the part (i-e .. i] in front of this one
                const int e1 = i - 1 < emax ? i - 1 : emax;
                const double* __restrict__ x = tab + SP_FM2O * ts + (size_t)d * ldn + i;
                const double* __restrict__ y = tab + SP_FM1 * ts + i;
                for (int e = 1; e <= e1; e++) fmo = fma(x[(size_t)e * ldn - e], y[(size_t)e * ldn - e], fmo);
            }
            {   // FM1o[i,d] += sum_e FM2o[d+e][i] * FM[e][j]: the part (j .. j+e] behind this one
                const int e1 = n - 1 - j < emax ? n - 1 - j : emax;
                const double* __restrict__ x = tab + SP_FM2O * ts + (size_t)d * ldn + i;
                const double* __restrict__ y = tab + SP_FM * ts + j;
                for (int e = 1; e <= e1; e++) s1 = fma(x[(size_t)e * ldn], y[(size_t)e * ldn], s1);
            }
            const bool up = d + 1 < Le;
            fmso = fmo + (up ? tab[SP_FMSO * ts + (size_t)(d + 1) * ldn + i] : 0.0) * M->w_mu;
            fm1o = s1 + fmso + (up ? tab[SP_FM1O * ts + (size_t)(d + 1) * ldn + i - 1] : 0.0) * M->w_mu;
        }
        double e_tmc = 0.0;
        if (type) {
            const int idx = 25 * (5 * s_i + s_ip1) + 5 * s_jp1 + s_j;
            const int idx_raw = 25 * (5 * s_jp1 + s_jp2) + 5 * s_i + s_im1;
            e_txo = M->TXO[idx]; e_tmc = M->TMC[idx]; e_tau = M->E_tau[type];
            const double e_txi = M->TXI[idx_raw], e_tsa = M->TSA[idx_raw];
            const double ext = span_ext_outer(A.gi[i - 1], A.go[j + 1], A.gi[n], A.sc * (double)d);
            const double multi = d + 2 < Le ? tab[SP_FM1O * ts + (size_t)(d + 2) * ldn + i - 1] * M->w_mp2 : 0.0;
            // enclosing pairs (io, jo+1) = (i-1-l1, j+2+l2), cell (io, d+2+t); a cell that does not exist holds 0, column 0 included
            double g = 0.0, gb = 0.0, sm = 0.0;
            for (int t = 2; t <= kMaxSingle && d + 2 + t < Le; t++) {
                const size_t base = (size_t)(d + 2 + t) * ldn + i - 1;
                if (t >= 4) {
                    const double* __restrict__ w = M->shape_w + t * (t + 1) / 2;
                    const double* __restrict__ x = tab + SP_FCOX * ts + base;
                    const int l1e = t - 1 < i - 1 ? t - 1 : i - 1;
                    for (int l1 = 1; l1 <= l1e; l1++) g = fma(w[l1], x[-l1], g);
                }
                const double* __restrict__ xb = tab + SP_FCOB * ts + base;
                gb = fma(M->WB[t], xb[0] + (t <= i - 1 ? xb[-t] : 0.0), gb);
            }
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const int l1 = small_l1(k), l2 = small_l2(k), io = i - 1 - l1, jo = j + 1 + l2;
                if (d + 2 + l1 + l2 >= Le || io < 1 || jo > n - 1) continue;
                const double v = tab[SP_FCO * ts + (size_t)(jo - io) * ldn + io];
                if (v == 0.0) continue;
                const int to = vienna_ptype(s[io], s[jo + 1]);
                sm = fma(v, span_small_w(M, l1, l2, to, type, s[io + 1], s[jo], s_im1, s_jp2), sm);
            }
            fco = e_tsa * (ext + multi) + e_txi * g + e_tau * gb + sm;
            p = d >= kMinHairpin ? fco * tab[SP_FC * ts + at] : 0.0;
            if (!(p == p) || !(fco == fco) || p > 1e300 || fco > 1e300) { bad = true; p = 0.0; fco = 0.0; }
            p = p > 1.0 ? 1.0 : (p < 0.0 ? 0.0 : p);
        }
        fm2o = fmo + fco * e_tmc;
        if (!(fm2o == fm2o) || fm2o > 1e300 || !(fm1o == fm1o) || fm1o > 1e300) { bad = true; fm2o = fm1o = fmso = 0.0; }
    }
    if (bad) atomicOr(A.bad, 1);
    tab[SP_FCO * ts + at] = fco;
    tab[SP_FCOX * ts + at] = fco * e_txo;
    tab[SP_FCOB * ts + at] = fco * e_tau;
    tab[SP_FMSO * ts + at] = fmso;
    tab[SP_FM1O * ts + at] = fm1o;
    tab[SP_FM2O * ts + at] = fm2o;
    // bp_band[(i-1) * Le + d+1] = P(i, i+d+1); the lanes 1..n cover every row of the band, 0 where the pair runs off the end
    if (i >= 1 && i <= n && d + 1 < Le) A.band[(size_t)(i - 1) * Le + d + 1] = p;
}

// ---- finish: up[i] = 1 - sum_j P(i, j), column 0 of the band, log Z.  grid (n), one wavefront per letter
__global__ __launch_bounds__(kSpanBlock) void span_finish(const SpanArgs* __restrict__ items)
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
        if (A.max_w == 1) A.up[i0] = u < 0.0 ? 0.0 : u;   // (wider: span_acc_final writes every column)
        A.band[(size_t)i0 * Le] = 0.0;
        if (i0 == 0) A.logz[0] = A.gi[n];
    }
}

// =================================================================================
// Region accessibility up[i][w] = P(letters i+1 .. i+1+w unpaired) on the band tables behind the outside sweep (rh_span_fold_acc, max_w > 1):
// the decomposition of the vlin_acc_* family in mccaskill_vlin.hip -- a run a..b lies in the exterior (E), in a hairpin loop (H), in a
// gap of a loop with one enclosed pair (I) or in a run of a multiloop (M).  The outside tables are stored divided by Z and times
// lam^-len, the inside tables times lam^len, so every outside x inside product is a probability up to the weights of the run's own
// unpaired letters (w_mu^len in M; the loop weights carry them in H and I), and E is a difference of logarithms.  A cell that does
// not exist holds 0 in every table and every row is ldn wide, so a read needs only its row below Le and its column inside 0..ldn-1.
constexpr int SP_ACC_R = SP_FM;   // FM is dead behind the outside sweep: the hairpin suffix sums R take its place

// R[d][p] = sum_{d' >= d} Hp(p, p+d'+1), Hp(p, q) = P(letters p, q close a hairpin loop) = FCo^(p, d) x the hairpin weight of
// span_inside_diag.  One lane per column p, rows in descending order.
__global__ __launch_bounds__(kSpanThreads) void span_acc_hp(const SpanArgs* __restrict__ items, const VLinModel* __restrict__ M)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    if ((size_t)blockIdx.x * kSpanThreads >= A.ldn) return;
    const size_t col = (size_t)blockIdx.x * kSpanThreads + threadIdx.x;
    if (col >= A.ldn) return;
    const int p = (int)col, n = A.n;
    const size_t ldn = A.ldn;
    const uint8_t* __restrict__ s = A.s;
    const double* __restrict__ fco = A.tab + SP_FCO * A.ts + p;
    double* __restrict__ R = A.tab + SP_ACC_R * A.ts + p;
    int lt[6];   // letters p .. p+5 (the tetraloop's), code 0 past the end
#pragma unroll
    for (int k = 0; k < 6; k++) lt[k] = s[p + k <= n + 1 ? p + k : n + 1];
    double run = 0.0;
    for (int d = A.Le - 1; d >= 0; d--) {
        const int q = p + d + 1;
        if (d >= kMinHairpin && p >= 1 && q <= n) {
            const double o = fco[(size_t)d * ldn];
            if (o != 0.0) {   // (a pair that cannot form has FCo^ = 0)
                const int sq = s[q], sqm = s[q - 1];
                double e = A.hplen[d];
                if (d == 3) e *= M->E_tau[vienna_ptype(lt[0], sq)];
                else {
                    e *= M->TMH[25 * (5 * lt[0] + lt[1]) + 5 * sq + sqm];
                    if (d == 4 && lt[0] != 0 && lt[1] != 0 && lt[2] != 0 && lt[3] != 0 && lt[4] != 0 && lt[5] != 0)
                        e *= M->E_tetra[(((((lt[0] - 1) * 4 + (lt[1] - 1)) * 4 + (lt[2] - 1)) * 4 + (lt[3] - 1)) * 4 + (lt[4] - 1)) * 4 + (lt[5] - 1)];
                }
                run = fma(o, e, run);
            }
        }
        R[(size_t)d * ldn] = run;
    }
}

// the H part: up[(a-1)*max_w + w] = H(a, b) = sum_{p < a} R[b-p][p], b = a + w <= n.  One wavefront per b: the widths share the terms
// p <= b - max_w (at most Le of them, lane-strided and added by wsum), then lane 0 adds one term per narrower width.
__global__ __launch_bounds__(256) void span_acc_hsum(const SpanArgs* __restrict__ items)
{
    const SpanArgs A = span_item(items, blockIdx.y);
    if ((int)blockIdx.x * 4 + 1 > A.n) return;
    const int b = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) + 1, lane = threadIdx.x & 63;
    const int n = A.n, Le = A.Le, mw = A.max_w;
    if (b > n) return;                                        // wave-uniform
    const size_t ldn = A.ldn;
    const double* __restrict__ R = A.tab + SP_ACC_R * A.ts;
    double tail = 0.0;
    for (int p = (b - Le + 1 > 1 ? b - Le + 1 : 1) + lane; p <= b - mw; p += 64) tail += R[(size_t)(b - p) * ldn + p];
    tail = wsum(tail);
    if (lane == 0) {
        double run = tail;
        for (int w = mw - 1; w >= 0; w--) {
            const int a = b - w;
            if (a < 1) continue;
            A.up[(size_t)(a - 1) * mw + w] = run;
            if (w >= 1 && w < Le) run += R[(size_t)w * ldn + a];   // width w-1 also counts p = a
        }
    }
}

// Gap sums of the loops with one enclosed pair, one THREAD per (letter, own gap length g = 1..30), lanes over the letter (as
// vlin_acc_gaps; blockIdx.y = side * 30 + g - 1):
//   GL[p][g] = sum over the loops with outer 5' letter p whose 5' gap is the g letters p+1..p+g
//   GR[q][g] = the same for the 3' gap q-g..q-1 of the outer 3' letter q
// A thread's inner 5' letter k = p+1+g (left) resp. inner 3' letter l = q-1-g (right) is fixed; its loops are (inner span r, other gap
// o): inner cell (k, r) resp. (l-1-r, r), outer span D = r+2+g+o, outer cell (p, D) resp. (q-1-D, D), only rows D < Le.  The outer
// values of inner span r+1 are those of r shifted by one o: a register window of 31 + UR - 1 entries that slides by UR per batch of
// UR inner spans, one new load per span; the generic weights w(g, o) are uniform over the workgroup.  Bulges and the tabulated shapes
// are a handful of (g, o) and are added with direct loads.  Every load of a lane's neighbours is a contiguous row segment.
__global__ __launch_bounds__(256) void span_acc_gaps(const SpanArgs* __restrict__ items, const VLinModel* __restrict__ M)
{
    constexpr int NW = kMaxSingle + 1, UR = 2;
    const SpanArgs A = span_item(items, blockIdx.z);
    if ((int)(blockIdx.x * blockDim.x) + 1 > A.n) return;   // no letter of the item in this workgroup
    const int g = (int)blockIdx.y % kMaxSingle + 1;
    const bool right = (int)blockIdx.y >= kMaxSingle;
    const int pos = blockIdx.x * blockDim.x + threadIdx.x + 1;   // p (left) or q (right)
    const int n = A.n, Le = A.Le;
    const bool live = pos <= n;
    const size_t ldn = A.ldn, ts = A.ts;
    const uint8_t* __restrict__ s = A.s;
    const double* __restrict__ FCO = A.tab + SP_FCO * ts;
    const double* __restrict__ FCOX = A.tab + SP_FCOX * ts;
    const double* __restrict__ FCOB = A.tab + SP_FCOB * ts;
    const double* __restrict__ FC = A.tab + SP_FC * ts;
    const double* __restrict__ FCX = A.tab + SP_FCX * ts;
    const double* __restrict__ FCB = A.tab + SP_FCB * ts;
    // generic weights of (own gap g, other gap o); 0 for bulges, tabulated shapes and o beyond the loop budget
    double wt[NW];
#pragma unroll
    for (int o = 0; o < NW; o++) {
        const int t = g + o;
        wt[o] = t <= kMaxSingle ? M->shape_w[t * (t + 1) / 2 + (right ? o : g)] : 0.0;
    }
    const double wb = g >= 2 ? M->WB[g] : 0.0;
    // outer cell of span D: column p (left) resp. q-1-D (right); 0 beyond the band and in front of letter 1
    const auto outer_at = [&](const double* __restrict__ T, int D) -> double {
        const int pc = right ? pos - 1 - D : pos;
        return (live && D < Le && pc >= 1) ? T[(size_t)D * ldn + pc] : 0.0;
    };
    const int kl = right ? pos - 1 - g : pos + 1 + g;   // inner 3' letter l (right) resp. inner 5' letter k (left)
    const int rmax = right ? kl - 2 : n - 1 - kl;       // inner spans 0..rmax exist
    const int r_end = Le - 3 - g;                       // the last inner span whose outer pair (other gap 0) lies in the band
    double win[NW + UR - 1];
#pragma unroll
    for (int o = 0; o < NW + UR - 1; o++) win[o] = outer_at(FCOX, 2 + g + o);
    double acc = 0.0;
    for (int r0 = 0; r0 <= r_end; r0 += UR) {
        double xs[UR], wn[UR], bo[UR], bi[UR];
        bool ok[UR];
        size_t ics[UR];
#pragma unroll
        for (int u = 0; u < UR; u++) {
            const int r = r0 + u;                             // (r <= r_end + 1 < Le)
            ok[u] = live && kl >= 1 && r <= rmax;
            ics[u] = (size_t)r * ldn + (ok[u] ? (right ? kl - 1 - r : kl) : 1);
            xs[u] = ok[u] ? FCX[ics[u]] : 0.0;
            wn[u] = outer_at(FCOX, r0 + UR + 2 + g + (NW - 1) + u);   // enters the window of the next batch at index NW-1+u
            bo[u] = ok[u] ? outer_at(FCOB, r + 2 + g) : 0.0;          // bulge: own gap g >= 2, other gap 0
            bi[u] = ok[u] ? FCB[ics[u]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < UR; u++) {
            const int r = r0 + u;
            double sum = 0.0;
#pragma unroll
            for (int o = 0; o < NW; o++) sum = fma(wt[o], win[u + o], sum);
            acc = fma(xs[u], sum, acc);
            acc = fma(bo[u] * wb, bi[u], acc);
            if (g <= 2 && ok[u]) {   // the tabulated shapes with this gap length (four of the sixty slices)
                const int k = right ? kl - 1 - r : kl, l = k + r + 1;   // inner pair (k, l)
                const double fc = FC[ics[u]];
                if (fc != 0.0) {
                    const int ti = vienna_ptype(s[k], s[l]);
                    for (int o = 0; o <= 2; o++) {
                        const int l1 = right ? o : g, l2 = right ? g : o;
                        if (l1 + l2 == 2 && (l1 == 0 || l2 == 0)) continue;   // 0x2 / 2x0 are bulges
                        const int D = r + 2 + g + o, p = k - 1 - l1, q = l + 1 + l2;
                        if (D >= Le || p < 1 || q > n) continue;
                        const double fo = FCO[(size_t)D * ldn + p];
                        if (fo == 0.0) continue;
                        acc = fma(fo * span_small_w(M, l1, l2, vienna_ptype(s[p], s[q]), ti, s[p + 1], s[q - 1], s[k - 1], s[l + 1]), fc, acc);
                    }
                }
            }
        }
        // slide the window by the batch
#pragma unroll
        for (int o = 0; o + 1 < NW; o++) win[o] = win[o + UR];
#pragma unroll
        for (int u = 0; u < UR; u++) win[NW - 1 + u] = wn[u];
    }
    if (live) A.gaps[((size_t)(right ? 1 : 0) * kSpanGapRows + g) * ldn + pos] = acc;
}

// gap sums -> suffix sums over the gap length: S[g][pos] = sum_{l >= g} G[l][pos]; one thread per (letter, side = blockIdx.y)
__global__ __launch_bounds__(256) void span_acc_gsuf(const SpanArgs* __restrict__ items)
{
    const SpanArgs A = span_item(items, blockIdx.z);
    if ((int)(blockIdx.x * blockDim.x) + 1 > A.n) return;
    const int pos = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (pos > A.n) return;
    double* __restrict__ G = A.gaps + (size_t)blockIdx.y * kSpanGapRows * A.ldn + pos;
    double run = 0.0;
    for (int g = kMaxSingle; g >= 1; g--) { run += G[(size_t)g * A.ldn]; G[(size_t)g * A.ldn] = run; }
}

// adds E, I and M to the H part and clamps; one THREAD per (letter a, width w = blockIdx.y), lanes over a.  A run that passes letter n
// holds 0; a value that is not finite raises the flag.
__global__ __launch_bounds__(256) void span_acc_final(const SpanArgs* __restrict__ items, const VLinModel* __restrict__ M)
{
    const SpanArgs A = span_item(items, blockIdx.z);
    if ((int)(blockIdx.x * blockDim.x) + 1 > A.n) return;
    const int a = blockIdx.x * blockDim.x + threadIdx.x + 1, w = blockIdx.y;
    const int n = A.n, Le = A.Le;
    if (a > n) return;
    const int b = a + w, len = w + 1;
    double* __restrict__ up = A.up + (size_t)(a - 1) * A.max_w + w;
    if (b > n) { *up = 0.0; return; }
    const size_t ldn = A.ldn, ts = A.ts;
    const double* __restrict__ gl = A.gaps;                                   // suffix sums over the gap length, [g][pos]
    const double* __restrict__ gr = A.gaps + (size_t)kSpanGapRows * ldn;
    double mu_len = 1.0;
    for (int k = 0; k < len; k++) mu_len *= M->w_mu;
    double acc = exp(A.gi[a - 1] + A.go[b] - A.gi[n]);                        // E, in logarithms
    // I: the run lies in the 5' gap of the loop whose outer 5' letter is p < a when that gap reaches b: length >= b-p
    for (int p = a - 1; p >= 1 && p >= b - kMaxSingle; p--) acc += gl[(size_t)(b - p) * ldn + p];
    for (int q = b + 1; q <= n && q <= a + kMaxSingle; q++) acc += gr[(size_t)(q - a) * ldn + q];   // ... 3' gaps
    double m = 0.0;
    if (a >= 2 && b <= n - 3) {     // M, run before a branch: FM1o(a-1, e+1) x FM1(b, e-w), the part ends at letter a+e; rows e+1 < Le
        const double* __restrict__ x = A.tab + SP_FM1O * ts + (a - 1);
        const double* __restrict__ y = A.tab + SP_FM1 * ts + b;
        const int e1 = n - 1 - a < Le - 2 ? n - 1 - a : Le - 2;
        for (int e = w + 2; e <= e1; e++) m = fma(x[(size_t)(e + 1) * ldn], y[(size_t)(e - w) * ldn], m);
    }
    if (a >= 4 && b <= n - 1) {     // M, run after the last branch: FMSo(i, e+len) x FMS(i, e), i = a-1-e; rows e+len < Le
        const double* __restrict__ x = A.tab + SP_FMSO * ts;
        const double* __restrict__ y = A.tab + SP_FMS * ts;
        const int e1 = a - 2 < Le - 1 - len ? a - 2 : Le - 1 - len;
        for (int e = 2; e <= e1; e++) {
            const int i = a - 1 - e;
            m = fma(x[(size_t)(e + len) * ldn + i], y[(size_t)e * ldn + i], m);
        }
    }
    acc += m * mu_len;
    acc += *up;                                                               // H (span_acc_hsum)
    if (!(acc <= 1e300)) atomicOr(A.bad, 1);
    *up = acc > 1.0 ? 1.0 : acc;
}

// the events of one call, gone with their scope
struct SpanEvents {
    hipEvent_t e[9] = {};
    hipError_t create()
    {
        for (auto& x : e) { hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; }
        return hipSuccess;
    }
    ~SpanEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

// device times (ms) of the attempts of one ladder: the sweeps; the exterior passes and the finish; the three steps of the accessibility stage
struct SpanTimes {
    double sweeps = 0, ext = 0, acc[3] = {0, 0, 0};
};

// One attempt on the model selected now over the items `run` (a single call: one): inside sweeps, exterior passes, outside sweeps,
// finish and, for the items that came back unflagged where widths above one are asked for, the accessibility stage on the same model
// and hairpin weights.  One launch per diagonal below the largest Le, over the widest ldn; the exterior passes have a workgroup per
// item.  The items share one hplen (it depends on the exponent only and item k reads the rows below its own Le); item k of `run`
// gets the flag bad[k], and (*flags)[k] is that flag behind everything that ran for it.  `sum`: the times are added to *T.
// A CONTRAfold context (`cf`: the model of this attempt, lin0 or a rung) runs the sweeps of mccaskill_span_cf.hip between the same
// exterior passes and finish, and the accessibility stage of mccaskill_span_cf_acc.hip.
int span_attempt(rh_ctx* c, const LinSet* cf, std::vector<SpanArgs>& run, int* bad, const SpanEvents& ev, std::vector<int>* flags, SpanTimes* T, bool sum)
{
    const VLinModel* M = c->d_vlin;
    hipStream_t st = c->s_mc;
    const unsigned K = (unsigned)run.size();
    const int max_w = run[0].max_w;
    int Le = 0, n = 0;
    size_t ldn = 0;
    bool cons = false;   // an item of the launches has a constraint: the sweeps that test pairs on the records
    for (unsigned k = 0; k < K; k++) {
        SpanArgs& A = run[k];
        Le = std::max(Le, A.Le); n = std::max(n, A.n); ldn = std::max(ldn, A.ldn);
        cons = cons || A.cons != nullptr;
        A.sc = cf ? cf->h.s : c->h_vlin->s;
        A.bad = bad + k;
    }
    std::vector<double> hplen((size_t)Le);
    if (cf) for (int d = 0; d < Le; d++) hplen[(size_t)d] = cf->h.E_hairpin[d < 30 ? d : 30] * std::exp(-cf->h.s * (double)d);
    else hairpin_length_weights(*c->h_vlin, Le, hplen.data());
    // CONTRAfold: the exterior's factor of row d, exp(external_paired - external_unpaired (d + 2)) (span_fold.h)
    const double eu = cf ? c->h_score->external_unpaired : 0.0, ep = cf ? c->h_score->external_paired : 0.0;
    const auto ext_w = [&](int d) { return std::exp(ep - eu * (double)(d + 2)); };
    int rc;
    if ((rc = ensure(c, c->d_span_desc, sizeof(SpanArgs) * K, false))) return rc;
    const SpanArgs* items = c->d_span_desc.as<const SpanArgs>();
    HIP_TRY(c, hipMemcpyAsync(const_cast<double*>(run[0].hplen), hplen.data(), sizeof(double) * hplen.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_span_desc.p, run.data(), sizeof(SpanArgs) * K, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(bad, 0, sizeof(int) * K, st));
    const dim3 grid((unsigned)((ldn + kSpanThreads - 1) / kSpanThreads), K), block(kSpanThreads);
    HIP_TRY(c, hipEventRecord(ev.e[0], st));
    const auto inside = cons ? span_inside_diag<true> : span_inside_diag<false>;
    const auto outside = cons ? span_outside_diag<true> : span_outside_diag<false>;
    if (cf) for (int d = 0; d < Le; d++) hipLaunchKernelGGL(span_cf_inside_diag, grid, block, 0, st, items, cf->d.as<const LinModel>(), d, ext_w(d));
    else for (int d = 0; d < Le; d++) hipLaunchKernelGGL(inside, grid, block, 0, st, items, M, d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e[1], st));
    hipLaunchKernelGGL(span_ext_pass, dim3(1, K), dim3(kSpanBlock * kSpanWaves), 0, st, items, 0);
    hipLaunchKernelGGL(span_ext_pass, dim3(1, K), dim3(kSpanBlock * kSpanWaves), 0, st, items, 1);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e[2], st));
    if (cf) for (int d = Le - 1; d >= 0; d--) hipLaunchKernelGGL(span_cf_outside_diag, grid, block, 0, st, items, cf->d.as<const LinModel>(), d, ext_w(d));
    else for (int d = Le - 1; d >= 0; d--) hipLaunchKernelGGL(outside, grid, block, 0, st, items, M, d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e[3], st));
    hipLaunchKernelGGL(span_finish, dim3((unsigned)n, K), dim3(kSpanBlock), 0, st, items);
    if (cf) hipLaunchKernelGGL(span_cf_logz, dim3((K + 63) / 64), dim3(64), 0, st, items, (int)K, eu);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e[4], st));
    flags->assign(K, 1);
    HIP_TRY(c, hipMemcpyAsync(flags->data(), bad, sizeof(int) * K, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float t[4] = {};
    for (int k = 0; k < 4; k++) HIP_TRY(c, hipEventElapsedTime(&t[k], ev.e[k], ev.e[k + 1]));
    T->sweeps = (sum ? T->sweeps : 0.0) + (double)t[0] + t[2];
    T->ext = (sum ? T->ext : 0.0) + (double)t[1] + t[3];
    if (max_w == 1) return RH_OK;
    // the accessibility stage for the unflagged items: the hairpin part, the gap sums, the final kernel
    std::vector<SpanArgs> acc;
    for (unsigned k = 0; k < K; k++) if (!(*flags)[k]) acc.push_back(run[k]);
    if (acc.empty()) return RH_OK;
    const unsigned Ka = (unsigned)acc.size();
    n = 0; ldn = 0; Le = 0;
    for (const SpanArgs& A : acc) { n = std::max(n, A.n); ldn = std::max(ldn, A.ldn); Le = std::max(Le, A.Le); }
    HIP_TRY(c, hipMemcpyAsync(c->d_span_desc.p, acc.data(), sizeof(SpanArgs) * Ka, hipMemcpyHostToDevice, st));   // (the sweeps are done with it)
    const unsigned letters = (unsigned)((n + 255) / 256);
    if (cf) {
        // CONTRAfold (mccaskill_span_cf_acc.hip).  The three times: everything but the chain (hairpin sums, gap sums, column 0, the
        // final kernel); the S build; the links with their closes.
        const LinModel* Mc = cf->d.as<const LinModel>();
        const unsigned cols = (unsigned)((ldn + kSpanThreads - 1) / kSpanThreads);
        HIP_TRY(c, hipEventRecord(ev.e[5], st));
        hipLaunchKernelGGL(span_cf_acc_hp, dim3(cols, Ka), block, 0, st, items);
        hipLaunchKernelGGL(span_cf_acc_gaps, dim3((unsigned)((n + 127) / 128), 2 * kMaxSingle, Ka), dim3(128), 0, st, items, Mc);
        hipLaunchKernelGGL(span_acc_gsuf, dim3(letters, 2, Ka), dim3(256), 0, st, items);
        hipLaunchKernelGGL(span_cf_acc_col0, dim3((unsigned)n, Ka), dim3(kSpanBlock), 0, st, items);
        hipLaunchKernelGGL(span_cf_acc_final, dim3(letters, (unsigned)(max_w - 1), Ka), dim3(256), 0, st, items, Mc);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(ev.e[6], st));
        for (int d = 0; d < Le; d++) hipLaunchKernelGGL(span_cf_acc_sdiag, dim3(cols, Ka), block, 0, st, items, d);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(ev.e[7], st));
        const unsigned rows = (unsigned)std::min(Le, 65535);
        for (int j = 1; j < max_w; j++) {   // A_j into the table A_{j-1} did not come from
            const int src = j == 1 ? (int)CF_FMO : (j % 2 ? (int)CFA_A1 : (int)CFA_A0), dst = j % 2 ? (int)CFA_A0 : (int)CFA_A1;
            hipLaunchKernelGGL(span_cf_acc_link, dim3(cols, rows, Ka), block, 0, st, items, Mc, src, dst, j == 1 ? 1 : 0);
            hipLaunchKernelGGL(span_cf_acc_close, dim3(letters, Ka), dim3(256), 0, st, items, j, dst);
        }
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(ev.e[8], st));
        HIP_TRY(c, hipMemcpyAsync(flags->data(), bad, sizeof(int) * K, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        for (int k = 0; k < 3; k++) {
            float ta = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&ta, ev.e[5 + k], ev.e[6 + k]));
            T->acc[k] = (sum ? T->acc[k] : 0.0) + (double)ta;
        }
        return RH_OK;
    }
    HIP_TRY(c, hipEventRecord(ev.e[5], st));
    hipLaunchKernelGGL(span_acc_hp, dim3((unsigned)((ldn + kSpanThreads - 1) / kSpanThreads), Ka), block, 0, st, items, M);
    hipLaunchKernelGGL(span_acc_hsum, dim3((unsigned)((n + 3) / 4), Ka), dim3(256), 0, st, items);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e[6], st));
    hipLaunchKernelGGL(span_acc_gaps, dim3(letters, 2 * kMaxSingle, Ka), dim3(256), 0, st, items, M);
    hipLaunchKernelGGL(span_acc_gsuf, dim3(letters, 2, Ka), dim3(256), 0, st, items);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e[7], st));
    hipLaunchKernelGGL(span_acc_final, dim3(letters, (unsigned)max_w, Ka), dim3(256), 0, st, items, M);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e[8], st));
    HIP_TRY(c, hipMemcpyAsync(flags->data(), bad, sizeof(int) * K, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int k = 0; k < 3; k++) {
        float ta = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ta, ev.e[5 + k], ev.e[6 + k]));
        T->acc[k] = (sum ? T->acc[k] : 0.0) + (double)ta;
    }
    return RH_OK;
}

// The exponent ladder over the items of one set of launches: the context's exponent first, then its ladder in exponent_order's order,
// while a band cell of an item leaves the double range.  The flagged items of an attempt are the next attempt's items, on their own
// tables, so every item ends on the exponent its single call ends on.  (*status)[k]: RH_OK, or RH_ERR_UNSUPPORTED where no exponent
// holds for item k.
// A CONTRAfold context starts on lin0 (s = 0.12) whatever the batch path remembers (lin_primary: a span fold's bits depend on its
// letters only) and goes on over kRungS; the rung models are the batch path's, built on first use, and nothing is selected.
int span_ladder(rh_ctx* c, const std::vector<SpanArgs>& items, int* bad, std::vector<int>* status, SpanTimes* T, bool sum)
{
    SpanEvents ev;
    HIP_TRY(c, ev.create());
    const bool cf = c->model == RH_MODEL_CONTRAFOLD;
    const int first = cf ? -1 : c->vlin_primary;
    std::vector<int> order = {first};
    for (int model : cf ? exponent_order(first, c->lin0.h.s, kRungS, rh_ctx::kRungs) : exponent_order(first, c->vlin_m[0].h->s, kVRungS, rh_ctx::kVRungs))
        order.push_back(model);
    std::vector<int> left(items.size()), flags;
    for (size_t k = 0; k < left.size(); k++) left[k] = (int)k;
    int rc = RH_OK;
    for (size_t a = 0; a < order.size() && !left.empty(); a++) {
        if ((rc = cf ? (order[a] >= 0 ? ensure_rungs(c) : RH_OK) : select_vlin(c, order[a]))) break;
        const LinSet* lin = !cf ? nullptr : order[a] < 0 ? &c->lin0 : &c->lin_r[order[a]];
        std::vector<SpanArgs> run;
        for (int k : left) run.push_back(items[(size_t)k]);
        if ((rc = span_attempt(c, lin, run, bad, ev, &flags, T, sum))) break;
        std::vector<int> next;
        for (size_t k = 0; k < left.size(); k++) if (flags[k]) next.push_back(left[k]);
        left.swap(next);
    }
    const int back = cf ? RH_OK : select_vlin(c, c->vlin_primary);
    if (rc) return rc;
    if (back) return back;
    status->assign(items.size(), RH_OK);
    for (int k : left) (*status)[(size_t)k] = RH_ERR_UNSUPPORTED;
    return RH_OK;
}

// has_cons: the call came with a constraint (an entry of a batch's is not NULL)
int span_refusals(rh_ctx* c, int max_w, bool has_cons)
{
    if (c->model == RH_MODEL_CONTRAFOLD && c->span_cf) {   // rh_set_span_contrafold: what the CONTRAfold sweeps do not cover
        if (c->mode == RH_MODE_LOG) return fail(c, RH_ERR_UNSUPPORTED, "span fold: there is no log-space version (the context is in RH_MODE_LOG)");
        if (max_w > 1 && !c->region_acc)
            return fail(c, RH_ERR_UNSUPPORTED,
                        "span fold: the CONTRAfold model has no span region accessibility (max_w %d: width 1 only) unless rh_set_region_accessibility is on", max_w);
        if (has_cons) return fail(c, RH_ERR_UNSUPPORTED, "span fold: the CONTRAfold model takes no structure constraint (pass NULL)");
        return RH_OK;
    }
    if (c->model != RH_MODEL_VIENNA_BL) return fail(c, RH_ERR_UNSUPPORTED, "span fold: the CONTRAfold model has no span-limited kernels (Vienna-BL contexts only)");
    if (c->vienna_sem == kViennaSem20) return fail(c, RH_ERR_UNSUPPORTED, "span fold: ViennaRNA-2.x semantics have no span-limited kernels (1.8 semantics only)");
    if (c->mode == RH_MODE_LOG) return fail(c, RH_ERR_UNSUPPORTED, "span fold: there is no log-space version (the context is in RH_MODE_LOG)");
    return RH_OK;
}

// the letter codes of one item as the model's batch path encodes them; the model's "no nucleotide" code (span_no_letter) stays at 0
// and behind the last letter
void span_codes(const rh_ctx* c, const char* seq, int n, uint8_t* codes)
{
    const bool cf = c->model == RH_MODEL_CONTRAFOLD;
    for (int i = 0; i < n; i++) codes[(size_t)i + 1] = cf ? nuc_code(seq[i]) : vienna_code(seq[i]);
}
uint8_t span_no_letter(const rh_ctx* c) { return c->model == RH_MODEL_CONTRAFOLD ? 4 : 0; }
// the band tables of an item: the sweeps' and, under the CONTRAfold model at widths above one, the accessibility stage's own
int span_tables(const rh_ctx* c, int max_w)
{
    return c->model == RH_MODEL_CONTRAFOLD ? span_cf_tables(max_w) : kSpanTables;
}

// rh_span_fold (max_w = 1), rh_span_fold_acc and rh_span_fold_constrained (cons, which may be NULL): a batch of one whose result is
// the context's local result
int span_run(rh_ctx* c, const char* seq, int n, const char* cons, int max_span, int max_w)
{
    if (!c) return RH_ERR_ARG;
    SpanPlan P;
    SpanAccPlan Q;
    std::string why;
    std::vector<ConsRec> rec;   // empty: nothing restricts the band
    bool restricts = false;
    if (int rc = span_check(seq, n, max_span, &P, &why, span_tables(c, max_w))) return fail(c, rc, "%s", why.c_str());
    if (int rc = span_acc_check(P, max_w, &Q, &why)) return fail(c, rc, "%s", why.c_str());
    if (int rc = span_cons_records(seq, n, cons, max_span, &rec, &restricts, &why)) return fail(c, rc, "%s", why.c_str());
    if (int rc = span_refusals(c, max_w, cons != nullptr)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->loc_valid = c->loc_hp.valid = false;   // (the hp result of rh_local_duplex goes with the band it came with)
    int rc;
    const size_t seq_bytes = ((size_t)n + 2 + 15) & ~(size_t)15;
    if ((rc = ensure(c, c->d_span_tab, sizeof(double) * P.tables, false))) return rc;
    if ((rc = ensure(c, c->d_span_ext, sizeof(double) * (P.ext + (size_t)P.Le), false))) return rc;
    if ((rc = ensure(c, c->d_span_seq, seq_bytes, false))) return rc;
    if ((rc = ensure(c, c->d_span_bad, sizeof(int), false))) return rc;
    if ((rc = ensure(c, c->d_loc_bp, sizeof(double) * P.band, false))) return rc;
    if ((rc = ensure(c, c->d_loc_up, sizeof(double) * Q.up, false))) return rc;
    if (Q.gaps && (rc = ensure(c, c->d_span_gaps, sizeof(double) * Q.gaps, false))) return rc;
    if ((rc = ensure(c, c->d_loc_logz, sizeof(double), false))) return rc;
    if (restricts && (rc = ensure(c, c->d_span_cons, sizeof(ConsRec) * rec.size(), false))) return rc;
    std::vector<uint8_t> codes(seq_bytes, span_no_letter(c));
    span_codes(c, seq, n, codes.data());
    HIP_TRY(c, hipMemcpyAsync(c->d_span_seq.p, codes.data(), seq_bytes, hipMemcpyHostToDevice, c->s_mc));
    if (restricts) HIP_TRY(c, hipMemcpyAsync(c->d_span_cons.p, rec.data(), sizeof(ConsRec) * rec.size(), hipMemcpyHostToDevice, c->s_mc));
    SpanArgs A{};
    A.tab = c->d_span_tab.as<double>(); A.ldn = P.ldn; A.ts = P.table;
    A.s = c->d_span_seq.as<const uint8_t>();
    A.n = n; A.Le = P.Le; A.L = max_span;
    A.gi = c->d_span_ext.as<double>(); A.go = A.gi + (n + 1); A.hplen = A.go + (n + 1);
    A.band = c->d_loc_bp.as<double>(); A.up = c->d_loc_up.as<double>(); A.logz = c->d_loc_logz.as<double>();
    A.gaps = Q.gaps ? c->d_span_gaps.as<double>() : nullptr; A.max_w = max_w;
    A.cons = restricts ? c->d_span_cons.as<const ConsRec>() : nullptr;
    std::vector<int> status;
    SpanTimes T;
    if ((rc = span_ladder(c, {A}, c->d_span_bad.as<int>(), &status, &T, false))) return rc;   // (the times of the last attempt)
    if (status[0]) return fail(c, RH_ERR_UNSUPPORTED, "span fold: no scale exponent of the ladder keeps the band tables of max_span %d in the double range", max_span);
    c->span_ms[0] = T.sweeps; c->span_ms[1] = T.ext;
    for (int k = 0; k < 3; k++) c->span_acc_ms[k] = T.acc[k];
    LocalPlan R;
    R.n = n; R.W = max_span; R.S = 1; R.We = n; R.nw = 1; R.ld = P.Le;   // one window at 0 with the band pitch Le
    c->loc = R; c->loc_max_w = max_w; c->loc_valid = true;
    c->span_acc_timed = max_w > 1;
    c->loc_ms[0] = c->span_ms[0]; c->loc_ms[1] = c->span_ms[1];
    if (c->span_acc_timed) c->loc_ms[1] += c->span_acc_ms[0] + c->span_acc_ms[1] + c->span_acc_ms[2];
    c->span_timed = true;
    return RH_OK;
}

// rh_span_fold_batch and rh_span_fold_batch_constrained (cons, or any entry of it, may be NULL): chunk after chunk on the grow-only
// scratch of the single calls; the results go to the batch's own buffers.  The records of a chunk lie item after item like its letter
// codes, a record per code, and are not part of the chunk budget, as the letters are not: the chunks do not depend on the constraints.
int span_batch_run(rh_ctx* c, const char* const* seqs, const int* n, int count, const char* const* cons, int max_span, int max_w)
{
    if (!c) return RH_ERR_ARG;
    SpanBatchPlan B;
    std::string why;
    std::vector<std::vector<ConsRec>> recs;   // per item; empty: nothing restricts its band
    if (int rc = span_batch_plan(seqs, n, count, max_span, max_w, c->sb_bytes, &B, &why, span_tables(c, max_w))) return fail(c, rc, "%s", why.c_str());
    if (int rc = span_cons_batch(seqs, n, count, cons, max_span, &recs, &why)) return fail(c, rc, "%s", why.c_str());
    bool has_cons = false;
    for (int k = 0; cons && k < count; k++) has_cons = has_cons || cons[k] != nullptr;
    if (int rc = span_refusals(c, max_w, has_cons)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->sb_valid = false;
    size_t tables = 0, gaps = 0, ext = 0, letters = 0, records = 0;
    int items = 0;
    for (const SpanChunk& C : B.chunks) {
        tables = std::max(tables, C.tables); gaps = std::max(gaps, C.gaps); ext = std::max(ext, C.ext + (size_t)C.max_Le);
        letters = std::max(letters, C.letters); items = std::max(items, C.count);
        for (int j = 0; j < C.count; j++)
            if (!recs[(size_t)(C.first + j)].empty()) records = std::max(records, C.letters);
    }
    int rc;
    if ((rc = ensure(c, c->d_span_tab, sizeof(double) * tables, false))) return rc;
    if ((rc = ensure(c, c->d_span_ext, sizeof(double) * ext, false))) return rc;
    if ((rc = ensure(c, c->d_span_seq, letters, false))) return rc;
    if ((rc = ensure(c, c->d_span_bad, sizeof(int) * (size_t)items, false))) return rc;
    if (gaps && (rc = ensure(c, c->d_span_gaps, sizeof(double) * gaps, false))) return rc;
    if ((rc = ensure(c, c->d_sb_bp, sizeof(double) * B.band, false))) return rc;
    if ((rc = ensure(c, c->d_sb_up, sizeof(double) * B.up, false))) return rc;
    if ((rc = ensure(c, c->d_sb_logz, sizeof(double) * (size_t)count, false))) return rc;
    if (records && (rc = ensure(c, c->d_span_cons, sizeof(ConsRec) * records, false))) return rc;
    std::vector<int> status((size_t)count, RH_OK), part;
    SpanTimes T;
    for (const SpanChunk& C : B.chunks) {
        std::vector<uint8_t> codes(C.letters, span_no_letter(c));
        std::vector<ConsRec> crec;   // the chunk's records, as many as letter codes, where an item of the chunk has some
        std::vector<SpanArgs> args((size_t)C.count);
        size_t tab_at = 0, gaps_at = 0, ext_at = 0, seq_at = 0;
        double* hplen = c->d_span_ext.as<double>() + C.ext;   // behind the chunk's gi and go
        for (int j = 0; j < C.count; j++) {
            const int k = C.first + j;
            const SpanBatchItem& I = B.items[(size_t)k];
            span_codes(c, seqs[k], I.P.n, codes.data() + seq_at);
            SpanArgs& A = args[(size_t)j];
            A = SpanArgs{};
            A.tab = c->d_span_tab.as<double>() + tab_at; A.ldn = I.P.ldn; A.ts = I.P.table;
            A.s = c->d_span_seq.as<const uint8_t>() + seq_at;
            A.n = I.P.n; A.Le = I.P.Le; A.L = max_span;
            A.gi = c->d_span_ext.as<double>() + ext_at; A.go = A.gi + (I.P.n + 1); A.hplen = hplen;
            A.band = c->d_sb_bp.as<double>() + I.band_at; A.up = c->d_sb_up.as<double>() + I.up_at; A.logz = c->d_sb_logz.as<double>() + k;
            A.gaps = I.Q.gaps ? c->d_span_gaps.as<double>() + gaps_at : nullptr; A.max_w = max_w;
            const std::vector<ConsRec>& R = recs[(size_t)k];
            if (!R.empty()) {   // (n + 2 records behind seq_at, inside the C.letters the chunk's codes take)
                if (crec.empty()) crec.assign(C.letters, ConsRec{0, 0});
                std::copy(R.begin(), R.end(), crec.begin() + (ptrdiff_t)seq_at);
                A.cons = c->d_span_cons.as<const ConsRec>() + seq_at;
            }
            tab_at += I.P.tables; gaps_at += I.Q.gaps; ext_at += I.P.ext; seq_at += ((size_t)I.P.n + 2 + 15) & ~(size_t)15;
        }
        HIP_TRY(c, hipMemcpyAsync(c->d_span_seq.p, codes.data(), C.letters, hipMemcpyHostToDevice, c->s_mc));
        if (!crec.empty()) HIP_TRY(c, hipMemcpyAsync(c->d_span_cons.p, crec.data(), sizeof(ConsRec) * crec.size(), hipMemcpyHostToDevice, c->s_mc));
        if ((rc = span_ladder(c, args, c->d_span_bad.as<int>(), &part, &T, true))) return rc;   // (synchronised: the next chunk reuses the scratch)
        for (int j = 0; j < C.count; j++) status[(size_t)(C.first + j)] = part[(size_t)j];
    }
    c->sb = std::move(B);
    c->sb_status.swap(status);
    c->sb_ms[0] = T.sweeps; c->sb_ms[1] = T.ext; c->sb_ms[2] = T.acc[0] + T.acc[1] + T.acc[2];
    c->sb_scan_ms = 0;
    c->sb_valid = true;
    return RH_OK;
}

// a fetch of item `item` of the batch result: RH_OK, or the failure recorded in the context
int span_batch_ready(rh_ctx* c, int item, const char* who, bool served)
{
    if (!c->sb_valid) return fail(c, RH_ERR_ARG, "%s: no span batch result", who);
    if (item < 0 || item >= c->sb.count) return fail(c, RH_ERR_ARG, "%s: item %d outside the batch of %d", who, item, c->sb.count);
    if (served && c->sb_status[(size_t)item])
        return fail(c, c->sb_status[(size_t)item], "%s: item %d: no scale exponent of the ladder keeps the band tables of max_span %d in the double range", who, item,
                    c->sb.L);
    return RH_OK;
}

}  // namespace

extern "C" {

int rh_set_span_contrafold(rh_ctx* c, int on)
{
    if (!c) return RH_ERR_ARG;
    if (c->model == RH_MODEL_CONTRAFOLD) c->span_cf = on != 0;   // (a Vienna-BL context has its span folds anyway: accepted, changes nothing)
    return RH_OK;
}
int rh_get_span_contrafold(const rh_ctx* c) { return c ? c->span_cf : RH_ERR_ARG; }

int rh_span_fold(rh_ctx* c, const char* seq, int n, int max_span) { return span_run(c, seq, n, nullptr, max_span, 1); }

int rh_span_fold_acc(rh_ctx* c, const char* seq, int n, int max_span, int max_w) { return span_run(c, seq, n, nullptr, max_span, max_w); }

int rh_span_fold_constrained(rh_ctx* c, const char* seq, int n, const char* constraint, int max_span, int max_w)
{
    return span_run(c, seq, n, constraint, max_span, max_w);
}

int rh_span_acc_times(rh_ctx* c, double ms[3])
{
    if (!c || !ms) return RH_ERR_ARG;
    if (!c->span_timed || !c->span_acc_timed) return fail(c, RH_ERR_ARG, "no span fold result with widths above one");
    for (int k = 0; k < 3; k++) ms[k] = c->span_acc_ms[k];
    return RH_OK;
}

int rh_span_times(rh_ctx* c, double ms[2])
{
    if (!c || !ms) return RH_ERR_ARG;
    if (!c->span_timed) return fail(c, RH_ERR_ARG, "no span fold result");
    ms[0] = c->span_ms[0]; ms[1] = c->span_ms[1];
    return RH_OK;
}

int rh_span_fold_batch(rh_ctx* c, const char* const* seqs, const int* n, int count, int max_span, int max_w)
{
    return span_batch_run(c, seqs, n, count, nullptr, max_span, max_w);
}

int rh_span_fold_batch_constrained(rh_ctx* c, const char* const* seqs, const int* n, int count, const char* const* constraints, int max_span, int max_w)
{
    return span_batch_run(c, seqs, n, count, constraints, max_span, max_w);
}

int rh_span_batch_layout(rh_ctx* c, int* count, int* max_span, int* max_w)
{
    if (!c) return RH_ERR_ARG;
    if (!c->sb_valid) return fail(c, RH_ERR_ARG, "rh_span_batch_layout: no span batch result");
    if (count) *count = c->sb.count;
    if (max_span) *max_span = c->sb.L;
    if (max_w) *max_w = c->sb.max_w;
    return RH_OK;
}

int rh_span_batch_item(rh_ctx* c, int item, int* n, int* ld, int* status)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = span_batch_ready(c, item, "rh_span_batch_item", false)) return rc;
    if (n) *n = c->sb.items[(size_t)item].P.n;
    if (ld) *ld = c->sb.items[(size_t)item].P.Le;
    if (status) *status = c->sb_status[(size_t)item];
    return RH_OK;
}

int rh_span_batch_results(rh_ctx* c, int item, double* bp_band, double* up, double* logz)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = span_batch_ready(c, item, "rh_span_batch_results", true)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const SpanBatchItem& I = c->sb.items[(size_t)item];
    if (bp_band) HIP_TRY(c, hipMemcpyAsync(bp_band, c->d_sb_bp.as<const double>() + I.band_at, sizeof(double) * I.P.band, hipMemcpyDeviceToHost, c->s_mc));
    if (up) HIP_TRY(c, hipMemcpyAsync(up, c->d_sb_up.as<const double>() + I.up_at, sizeof(double) * I.Q.up, hipMemcpyDeviceToHost, c->s_mc));
    if (logz) HIP_TRY(c, hipMemcpyAsync(logz, c->d_sb_logz.as<const double>() + item, sizeof(double), hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    return RH_OK;
}

int rh_span_batch_candidates(rh_ctx* c, int item, int what, float threshold, rh_cand* out, int cap)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = span_batch_ready(c, item, "rh_span_batch_candidates", true)) return rc;
    if (what < 0 || what > 1 || cap < 0 || (cap > 0 && !out)) return fail(c, RH_ERR_ARG, "rh_span_batch_candidates: bad what/cap");
    HIP_TRY(c, hipSetDevice(c->device));
    const SpanBatchItem& I = c->sb.items[(size_t)item];
    const double* table = what == 0 ? c->d_sb_bp.as<const double>() + I.band_at : c->d_sb_up.as<const double>() + I.up_at;
    return local_scan_table(c, table, I.P.n, what == 0 ? I.P.Le : c->sb.max_w, what, threshold, out, cap, &c->sb_scan_ms, "rh_span_batch_candidates");
}

int rh_set_span_batch_bytes(rh_ctx* c, size_t bytes)
{
    if (!c) return RH_ERR_ARG;
    c->sb_bytes = bytes;
    return RH_OK;
}

int rh_span_batch_times(rh_ctx* c, double ms[3])
{
    if (!c || !ms) return RH_ERR_ARG;
    if (!c->sb_valid) return fail(c, RH_ERR_ARG, "rh_span_batch_times: no span batch result");
    for (int k = 0; k < 3; k++) ms[k] = c->sb_ms[k];
    return RH_OK;
}

}  // extern "C"
