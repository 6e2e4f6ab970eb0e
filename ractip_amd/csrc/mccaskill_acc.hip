// mccaskill_acc.hip -- CONTRAfold model: region accessibility up[i][w] = P(letters i..i+w unpaired), widths 2..max_w, from
// the finished inside / outside tables (rh_set_region_accessibility; width 1 stays mc_unpaired's 1 - sum bp).
//
// up = Z(no letter of the region pairs) / Z, with Z the sum over the DERIVATIONS the inside recurrences count
// (InferenceEngine.ipp:3376-3717).  A region is unpaired when each of its letters is emitted by an "unpaired" step of the
// grammar, and adjacent unpaired letters lie in one loop, so a region a..b (letters, 1-based; len = b-a+1) has five sources:
//   exterior   F5i[a-1] * eu^len * F5o[b]
//   hairpin    sum_{i <= a-1, j >= b} FCo(i,j) * hairpin(i,j)                          (2-D suffix sums, O(n^2))
//   interior   sum over the one-sided gaps (i+1..p) or (q+1..j) of single-branch loops that contain the region; both sides
//              of a loop hold at most 30 letters, so a region gets at most 2 * 465 gap weights
//   multi, leading letters of a branch (FM1(i,j) -> FM1(i+1,j) + mu):  sum_j FM1o(a-1,j) * mu^len * FM1(b,j)
//   multi, trailing letters (FM(i,j) -> FM(i,j-1) + mu): FM = FM2 | FM(i,j-1)+mu | FM1 with FM2(i,j) = sum_k FM1(i,k) FM(k,j)
//              lets a trailing letter be shed at EVERY level of the right recursion, so one structure has several derivations
//              and Z counts them all.  Between shedding letter t+1 and letter t a derivation may descend through any run of
//              branches:  S(k,k') = delta + FM1(k,k') + sum_m FM1(k,m) FM1(m,k') + ...  (independent of the right end), and
//                  sum FMo(k_b,b) mu S(k_b,k_{b-1}) mu ... S(k_{a+1},k_a) mu FM(k_a,a-1)
//              is a chain of products with S: A_0[b][k] = mu FMo(k,b), A_j = mu A_{j-1} S, term(len = j+1) = A_j[b][.] . FM(., b-1-j).
// Every term is (outside) x (weights) x (inside) of total span n, so on the scaled linear tables the lambda^span factors
// cancel against Z~ = F5i~[n] term by term, whatever the scale exponent of the attempt.
//
// One text serves both table sets: the kernels are written over a semiring (PATH 0: the scaled linear tables, diagonal-major,
// (+, x); PATH 1: the log-space tables, square, (log-sum-exp, +)).
#include <hip/hip_runtime.h>

#include "batch.h"
#include "dev_util.h"
#include "lin_model.h"
#include "lse.h"
#include "score_model.h"
#include "kernels.h"

namespace rh {

namespace {

struct LinPath {   // values as the scaled linear sweeps leave them
    static constexpr int kFCX = L_FCX, kFM1 = L_FM1, kFM = L_FM, kFCOX = L_FCOX, kFMO = L_FMO, kFM1O = L_FM1O;
    static __device__ __forceinline__ double zero() { return 0.0; }
    static __device__ __forceinline__ double one() { return 1.0; }
    static __device__ __forceinline__ double mul(double a, double b) { return a * b; }
    static __device__ __forceinline__ double add(double a, double b) { return a + b; }
    static __device__ __forceinline__ double mad(double a, double b, double c) { return fma(a, b, c); }
    static __device__ __forceinline__ double prob(double x, double z) { return x / z; }
    static __device__ __forceinline__ size_t cell(int ld, int i, int j) { return (size_t)(j - i) * ld + i; }
    static __device__ __forceinline__ double eu(const AccArgs& A) { return A.lin->w_eu; }
    static __device__ __forceinline__ double mu(const AccArgs& A) { return A.lin->w_mu; }
    // ScoreHairpin without the junction (FCoX carries it), d unpaired letters
    static __device__ __forceinline__ double hairpin(const AccArgs& A, int d) { return exp(-A.lin->s * d) * A.lin->E_hairpin[d < 30 ? d : 30]; }
    // single-branch loop (l1, l2) without the junctions and the inner pair (FCoX and FCX carry them); letters i+1 and j of the loop
    static __device__ __forceinline__ double single(const AccArgs& A, int l1, int l2, int s_ip1, int s_j)
    {
        const LinModel* L = A.lin;
        if (l1 == 0 && l2 == 1) return L->w01 * L->E_b01[s_j];
        if (l1 == 1 && l2 == 0) return L->w10 * L->E_b10[s_ip1];
        if (l1 == 1 && l2 == 1) return L->w11 * L->E_11[s_ip1 * 5 + s_j];
        const int t = l1 + l2;
        return L->shape_w[t * (t + 1) / 2 + l1];
    }
};

struct LogPath {   // the log-space tables (sentinel kNeg = "zero")
    static constexpr int kFCX = T_FCX, kFM1 = T_FM1, kFM = T_FM, kFCOX = T_FCOX, kFMO = T_FMO, kFM1O = T_FM1O;
    static __device__ __forceinline__ double zero() { return kNeg; }
    static __device__ __forceinline__ double one() { return 0.0; }
    static __device__ __forceinline__ double mul(double a, double b) { return a + b; }
    static __device__ __forceinline__ double add(double a, double b)
    {
        const double m = fmax(a, b), lo = fmin(a, b);
        if (lo <= kNeg / 2) return m <= kNeg / 2 ? kNeg : m;   // (sums of sentinels stay the sentinel)
        return m + log1p(exp(lo - m));
    }
    static __device__ __forceinline__ double mad(double a, double b, double c) { return add(c, a + b); }
    static __device__ __forceinline__ double prob(double x, double z) { return x <= kNeg / 2 ? 0.0 : exp(x - z); }
    static __device__ __forceinline__ size_t cell(int ld, int i, int j) { return (size_t)i * ld + j; }
    static __device__ __forceinline__ double eu(const AccArgs& A) { return A.score->external_unpaired; }
    static __device__ __forceinline__ double mu(const AccArgs& A) { return A.score->multi_unpaired; }
    static __device__ __forceinline__ double hairpin(const AccArgs& A, int d) { return A.score->hairpin_len[d < 30 ? d : 30]; }
    static __device__ __forceinline__ double single(const AccArgs& A, int l1, int l2, int s_ip1, int s_j)
    {
        const ScoreModel* M = A.score;
        double v = M->mc_shape[l1 * 31 - l1 * (l1 - 1) / 2 + l2].score;   // row-major in (l1, l2), l1 + l2 <= 30 (param_loader.cpp)
        if (l1 == 0 && l2 == 1) v += M->bulge_0x1[s_j];
        if (l1 == 1 && l2 == 0) v += M->bulge_1x0[s_ip1];
        if (l1 == 1 && l2 == 1) v += M->internal_1x1[s_ip1 * 5 + s_j];
        return v;
    }
};

template <int PATH> struct PathOf { using type = LinPath; };
template <> struct PathOf<1> { using type = LogPath; };

// one sequence's tables and scratch: X0 (hairpin suffix sums, then chain vectors), X1 (S diagonal-major while it is built, then
// chain vectors), X2 (S, square), G (gap weights [2][31][ld]: left gaps by (l1, i), right gaps by (l2, j))
template <class P>
struct SeqView {
    const double* tab;
    double *x0, *x1, *x2, *g;
    const double *f5i, *f5o;
    const uint8_t* s;
    size_t ts;
    int ld, n;
    __device__ __forceinline__ SeqView(const McBatch& B, const AccArgs& A, int sq)
    {
        ld = B.ld; n = B.n[sq]; ts = B.tab_stride;
        tab = B.tab + (size_t)sq * B.seq_stride;
        double* sc = A.scratch + (size_t)sq * acc_scratch_doubles(B.ld);
        x0 = sc; x1 = sc + ts; x2 = sc + 2 * ts; g = sc + 3 * ts;
        f5i = B.f5i + (size_t)sq * ld; f5o = B.f5o + (size_t)sq * ld;
        s = B.seq + (size_t)sq * B.lds;
    }
    __device__ __forceinline__ double at(int table, int i, int j) const { return tab[table * ts + P::cell(ld, i, j)]; }
};

template <class P>
__device__ __forceinline__ double ring_pow(double x, int k)
{
    double p = P::one();
    for (int q = 0; q < k; q++) p = P::mul(p, x);
    return p;
}

}  // namespace

// ---- hairpin part, pass 1: x0[i][j] = sum_{i' <= i} FCoX(i',j) * hairpin(j-i'), 1 <= i <= j <= n-1; one thread per column j
template <int PATH>
__global__ __launch_bounds__(256) void cf_acc_hrows(McBatch B, AccArgs A)
{
    using P = typename PathOf<PATH>::type;
    const SeqView<P> V(B, A, blockIdx.y);
    const int j = blockIdx.x * 256 + threadIdx.x + 1;
    if (j > V.n - 1) return;
    double run = P::zero();
    for (int i = 1; i <= j; i++) {
        const int d = j - i;
        if (d >= kMinHairpin) run = P::add(run, P::mul(V.at(P::kFCOX, i, j), P::hairpin(A, d)));
        V.x0[(size_t)i * V.ld + j] = run;
    }
}

// ---- pass 2: x0[i][j] = sum_{j' >= j} of pass 1; one thread per row i
template <int PATH>
__global__ __launch_bounds__(256) void cf_acc_hcols(McBatch B, AccArgs A)
{
    using P = typename PathOf<PATH>::type;
    const SeqView<P> V(B, A, blockIdx.y);
    const int i = blockIdx.x * 256 + threadIdx.x + 1;
    if (i > V.n - 1) return;
    double run = P::zero();
    for (int j = V.n - 1; j >= i; j--) {
        run = P::add(run, V.x0[(size_t)i * V.ld + j]);
        V.x0[(size_t)i * V.ld + j] = run;
    }
}

// ---- gap weights of the single-branch loops.  blockIdx.y < 30: left gaps, l1 = blockIdx.y + 1, one thread per i:
//   g[l1][i] = sum_j FCoX(i,j) sum_{l2 <= 30-l1} w(l1,l2) FCX(i+1+l1, j-1-l2)       (letters i+1 .. i+l1 unpaired)
// blockIdx.y >= 30: right gaps, l2 = blockIdx.y - 29, one thread per j:
//   g[31+l2][j] = sum_i FCoX(i,j) sum_{l1 <= 30-l2} w(l1,l2) FCX(i+1+l1, j-1-l2)     (letters j-l2+1 .. j unpaired)
// A thread walks the outer pairs of its row (column) by growing span d.  The inner sum is a filter over a window that slides by
// one cell per step -- left gaps: the cells (i+1+l1, .) of one column, right gaps: the cells (., j-1-l2) of one row -- so a step
// loads the outer cell and the ONE cell that enters the window, which lives in registers (NT taps: the other side's lengths,
// rounded up to a multiple of eight; the weights beyond are the ring's zero).  On the diagonal-major tables both loads are row
// segments read at consecutive columns by consecutive threads.  The three shapes whose weight depends on the letters (0x1, 1x0,
// 1x1) have weight zero in the filter and are added per step.
template <class P, int NT>
__device__ __forceinline__ double gap_walk(const SeqView<P>& V, const AccArgs& A, int side, int l, int x)
{
    const int T = kMaxSingle - l, n = V.n;   // the other side holds 0 .. T letters
    double wgt[NT], win[NT];
#pragma unroll
    for (int lo = 0; lo < NT; lo++) {
        const int l1 = side ? lo : l, l2 = side ? l : lo;
        wgt[lo] = (lo <= T && !(l1 <= 1 && l2 <= 1)) ? P::single(A, l1, l2, 4, 4) : P::zero();
        win[lo] = P::zero();
    }
    const int dmax = side ? x - 1 : n - 1 - x;   // outer pair (i, j+1): 1 <= i, j <= n-1
    double acc = P::zero();
    for (int d = l + 2; d <= dmax; d++) {
        const int i = side ? x - d : x, j = i + d;
#pragma unroll
        for (int lo = NT - 1; lo > 0; lo--) win[lo] = win[lo - 1];
        win[0] = side ? V.at(P::kFCX, i + 1, j - 1 - l) : V.at(P::kFCX, i + 1 + l, j - 1);   // the other side empty
        double inner = P::zero();
#pragma unroll
        for (int lo = 0; lo < NT; lo++) inner = P::mad(wgt[lo], win[lo], inner);
        if (l <= 1) {   // (uniform) shapes with a letter term: the other side holds 0 or 1 letters
            const int s_ip1 = V.s[i + 1], s_j = V.s[j];
            if (l == 1) inner = P::mad(side ? P::single(A, 0, 1, s_ip1, s_j) : P::single(A, 1, 0, s_ip1, s_j), win[0], inner);
            inner = P::mad(P::single(A, 1, 1, s_ip1, s_j), win[1], inner);
        }
        acc = P::mad(V.at(P::kFCOX, i, j), inner, acc);
    }
    return acc;
}

template <int PATH>
__global__ __launch_bounds__(128) void cf_acc_gaps(McBatch B, AccArgs A)
{
    using P = typename PathOf<PATH>::type;
    const SeqView<P> V(B, A, blockIdx.z);
    const int x = blockIdx.x * 128 + threadIdx.x + 1;
    if (x > V.n - 1) return;
    const int side = blockIdx.y / kMaxSingle, l = blockIdx.y % kMaxSingle + 1;   // (uniform)
    const int taps = kMaxSingle - l + 1;
    double acc;
    if (taps <= 8) acc = gap_walk<P, 8>(V, A, side, l, x);
    else if (taps <= 16) acc = gap_walk<P, 16>(V, A, side, l, x);
    else if (taps <= 24) acc = gap_walk<P, 24>(V, A, side, l, x);
    else acc = gap_walk<P, 32>(V, A, side, l, x);
    V.g[(size_t)(side * 31 + l) * V.ld + x] = acc;
}

// ---- every term but the chain, one thread per region: a = letter, w = blockIdx.y + 1 (width w + 1).  Writes up[(a-1)*max_w + w].
template <int PATH>
__global__ __launch_bounds__(128) void cf_acc_final(McBatch B, AccArgs A)
{
    using P = typename PathOf<PATH>::type;
    const SeqView<P> V(B, A, blockIdx.z);
    const int a = blockIdx.x * 128 + threadIdx.x + 1, w = blockIdx.y + 1, n = V.n, ld = V.ld;
    if (a > n) return;
    const int b = a + w, len = w + 1;
    double* __restrict__ up = B.up + ((size_t)blockIdx.z * ld + (a - 1)) * A.max_w + w;
    if (b > n) { *up = 0.0; return; }
    double acc = P::mul(P::mul(V.f5i[a - 1], ring_pow<P>(P::eu(A), len)), V.f5o[b]);
    if (a - 1 >= 1 && b <= n - 1) {
        acc = P::add(acc, V.x0[(size_t)(a - 1) * ld + b]);
        // left gaps (i+1 .. p) with i <= a-1, p >= b, p - i <= 30; right gaps (q+1 .. j) with q <= a-1, j >= b, j - q <= 30
        for (int i = b - kMaxSingle > 1 ? b - kMaxSingle : 1; i <= a - 1; i++)
            for (int p = b; p <= i + kMaxSingle && p <= n - 1; p++) acc = P::add(acc, V.g[(size_t)(p - i) * ld + i]);
        for (int j = b; j <= a - 1 + kMaxSingle && j <= n - 1; j++)
            for (int q = j - kMaxSingle > 1 ? j - kMaxSingle : 1; q <= a - 1; q++) acc = P::add(acc, V.g[(size_t)(31 + j - q) * ld + j]);
        double m = P::zero();
        for (int j = b + 2; j <= n - 1; j++) m = P::mad(V.at(P::kFM1O, a - 1, j), V.at(P::kFM1, b, j), m);
        acc = P::add(acc, P::mul(m, ring_pow<P>(P::mu(A), len)));
    }
    const double p = P::prob(acc, V.f5i[n]);
    *up = !(p == p) ? 0.0 : (p > 1.0 ? 1.0 : p);
}

// ---- S = delta + G, G(k,k') = FM1(k,k') + sum_{k+2 <= m <= k'-2} FM1(k,m) G(m,k'): one workgroup per sequence walks the
// diagonals d = k'-k (a cell needs the shorter diagonals only).  The 1024 threads are cw cells x 1024/cw parts of the sum (cw =
// 64 .. 1024, the smallest that holds the diagonal), the parts meet in LDS in a fixed order.  x1 holds S diagonal-major, which
// the sum reads at consecutive columns; x2 holds it square for the products.
template <int PATH>
__global__ __launch_bounds__(1024) void cf_acc_sbuild(McBatch B, AccArgs A)
{
    using P = typename PathOf<PATH>::type;
    __shared__ double part[1024];
    const SeqView<P> V(B, A, blockIdx.x);
    const int n = V.n, ld = V.ld, tid = threadIdx.x;
    for (int d = 0; d <= n - 2; d++) {
        const int nc = n - 1 - d;   // cells k = 1 .. nc
        if (d < 4) {                // no sum: S(k,k) = 1, S(k,k+1) = 0, then FM1 alone
            for (int k = 1 + tid; k <= nc; k += 1024) {
                const double v = d == 0 ? P::one() : (d >= 2 ? V.at(P::kFM1, k, k + d) : P::zero());
                V.x1[(size_t)d * ld + k] = v;
                V.x2[(size_t)k * ld + k + d] = v;
            }
        } else {
            const int cw = nc <= 64 ? 64 : nc <= 128 ? 128 : nc <= 256 ? 256 : nc <= 512 ? 512 : 1024, parts = 1024 / cw;
            const int c = tid % cw, p = tid / cw;
            for (int k0 = 1; k0 <= nc; k0 += cw) {
                const int k = k0 + c;
                double acc = P::zero(), acc1 = P::zero();
                if (k <= nc) {
                    const double* sd = V.x1;
                    int e = 2 + p;
                    for (; e + 7 * parts <= d - 2; e += 8 * parts) {   // sixteen loads in flight
                        double f[8], g[8];
#pragma unroll
                        for (int u = 0; u < 8; u++) { f[u] = V.at(P::kFM1, k, k + e + u * parts); g[u] = sd[(size_t)(d - e - u * parts) * ld + k + e + u * parts]; }
#pragma unroll
                        for (int u = 0; u < 8; u += 2) { acc = P::mad(f[u], g[u], acc); acc1 = P::mad(f[u + 1], g[u + 1], acc1); }
                    }
                    for (; e <= d - 2; e += parts) acc = P::mad(V.at(P::kFM1, k, k + e), sd[(size_t)(d - e) * ld + k + e], acc);
                }
                part[tid] = P::add(acc, acc1);
                __syncthreads();
                if (p == 0 && k <= nc) {
                    double v = V.at(P::kFM1, k, k + d);
                    for (int q = 0; q < parts; q++) v = P::add(v, part[q * cw + c]);
                    V.x1[(size_t)d * ld + k] = v;
                    V.x2[(size_t)k * ld + k + d] = v;
                }
                __syncthreads();
            }
        }
        __syncthreads();   // (the next diagonal reads this one through global memory: same workgroup)
    }
}

// ---- A_0[b][k] = mu * FMo(k,b), 1 <= k <= b-3 (k = b-2 would end at FM(k,b-1) of span 1, which does not exist)
template <int PATH>
__global__ __launch_bounds__(256) void cf_acc_seed(McBatch B, AccArgs A)
{
    using P = typename PathOf<PATH>::type;
    const SeqView<P> V(B, A, blockIdx.z);
    const int k = blockIdx.x * 256 + threadIdx.x + 1, b = blockIdx.y + 1;
    if (b > V.n - 1 || k > b - 3) return;
    V.x0[(size_t)b * V.ld + k] = P::mul(P::mu(A), V.at(P::kFMO, k, b));
}

// ---- one link of the chain: dst[b][k'] = mu * sum_{k <= k'} src[b][k] S(k,k'), 1 <= k' <= b-3.  64 x 64 output tiles, K tiles of
// 16 staged in LDS, 4 x 4 outputs per thread; entries outside the triangles are never stored and read as the ring's zero, so
// neither matrix needs clearing.  flip: src = x1, dst = x0 (else x0 -> x1).
template <int PATH>
__global__ __launch_bounds__(256) void cf_acc_link(McBatch B, AccArgs A, int flip)
{
    using P = typename PathOf<PATH>::type;
    __shared__ __attribute__((aligned(16))) double As[kAccK][kAccTile + 2];   // [k][row b]     (pitch 66: 16-byte rows, read as double2)
    __shared__ __attribute__((aligned(16))) double Ss[kAccK][kAccTile + 2];   // [k][column k']
    const SeqView<P> V(B, A, blockIdx.z);
    const int n = V.n, ld = V.ld;
    const int b0 = blockIdx.y * kAccTile, c0 = blockIdx.x * kAccTile;
    if (c0 > b0 || b0 > n - 1) return;   // (no k' <= b-3 in the tile; uniform: before any barrier)
    const double* __restrict__ src = flip ? V.x1 : V.x0;
    double* __restrict__ dst = flip ? V.x0 : V.x1;
    const double* __restrict__ S = V.x2;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = P::zero();
    int kend = c0 + kAccTile - 1;                      // k <= k' and k <= b-3
    if (kend > b0 + kAccTile - 4) kend = b0 + kAccTile - 4;
    if (kend > n - 4) kend = n - 4;
    // the thread's four cells of each staged tile; the next K tile is fetched into registers while this one is multiplied
    double ra[4], rs[4];
    const auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int idx = threadIdx.x + q * 256;
            const int r = idx >> 4, kk = idx & 15, gb = b0 + r, gk = k0 + kk;
            ra[q] = (gb <= n - 1 && gk >= 1 && gk <= gb - 3) ? src[(size_t)gb * ld + gk] : P::zero();
            const int k2 = idx >> 6, cc = idx & 63, gk2 = k0 + k2, gc = c0 + cc;
            rs[q] = (gk2 >= 1 && gc <= n - 1 && gk2 <= gc) ? S[(size_t)gk2 * ld + gc] : P::zero();
        }
    };
    fetch(0);
    for (int k0 = 0; k0 <= kend; k0 += kAccK) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int idx = threadIdx.x + q * 256;
            As[idx & 15][idx >> 4] = ra[q];
            Ss[idx >> 6][idx & 63] = rs[q];
        }
        __syncthreads();
        if (k0 + kAccK <= kend) fetch(k0 + kAccK);
#pragma unroll
        for (int kk = 0; kk < kAccK; kk++) {
            const double2 a01 = *(const double2*)&As[kk][ty * 4], a23 = *(const double2*)&As[kk][ty * 4 + 2];
            const double2 s01 = *(const double2*)&Ss[kk][tx * 4], s23 = *(const double2*)&Ss[kk][tx * 4 + 2];
            const double av[4] = {a01.x, a01.y, a23.x, a23.y}, sv[4] = {s01.x, s01.y, s23.x, s23.y};
#pragma unroll
            for (int x = 0; x < 4; x++)
#pragma unroll
                for (int y = 0; y < 4; y++) acc[x][y] = P::mad(av[x], sv[y], acc[x][y]);
        }
        __syncthreads();
    }
    const double mu = P::mu(A);
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const int gb = b0 + ty * 4 + x, gc = c0 + tx * 4 + y;
            if (gb <= n - 1 && gc >= 1 && gc <= gb - 3) dst[(size_t)gb * ld + gc] = P::mul(mu, acc[x][y]);
        }
}

// ---- the chain's term of width j + 1: up[(a-1)*max_w + j] += sum_{k' <= t-2} A_j[b][k'] FM(k',t) / Z, a = b - j, t = b-1-j;
// one wavefront per b.  flip: A_j is in x1.
template <int PATH>
__global__ __launch_bounds__(256) void cf_acc_close(McBatch B, AccArgs A, int j, int flip)
{
    using P = typename PathOf<PATH>::type;
    const SeqView<P> V(B, A, blockIdx.y);
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6) + 1, lane = threadIdx.x & 63, n = V.n;
    const int a = b - j, t = b - 1 - j;
    if (b > n - 1 || a < 1) return;
    const double* __restrict__ row = (flip ? V.x1 : V.x0) + (size_t)b * V.ld;
    double acc = P::zero();
    for (int k = 1 + lane; k <= t - 2; k += 64) acc = P::mad(row[k], V.at(P::kFM, k, t), acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = P::add(acc, __shfl_xor(acc, o, 64));
    if (lane == 0) {
        double* __restrict__ up = B.up + ((size_t)blockIdx.y * V.ld + (a - 1)) * A.max_w + j;
        double p = P::prob(acc, V.f5i[n]);
        p = !(p == p) ? 0.0 : p;
        p += *up;
        *up = p > 1.0 ? 1.0 : p;
    }
}

#define RH_ACC_INSTANTIATE(PATH)                                          \
    template __global__ void cf_acc_hrows<PATH>(McBatch, AccArgs);        \
    template __global__ void cf_acc_hcols<PATH>(McBatch, AccArgs);        \
    template __global__ void cf_acc_gaps<PATH>(McBatch, AccArgs);         \
    template __global__ void cf_acc_final<PATH>(McBatch, AccArgs);        \
    template __global__ void cf_acc_sbuild<PATH>(McBatch, AccArgs);       \
    template __global__ void cf_acc_seed<PATH>(McBatch, AccArgs);         \
    template __global__ void cf_acc_link<PATH>(McBatch, AccArgs, int);    \
    template __global__ void cf_acc_close<PATH>(McBatch, AccArgs, int, int);
RH_ACC_INSTANTIATE(0)
RH_ACC_INSTANTIATE(1)
#undef RH_ACC_INSTANTIATE

}  // namespace rh
