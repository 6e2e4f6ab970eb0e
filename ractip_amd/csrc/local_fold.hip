// local_fold.hip -- local folding of a long sequence (rh_local_fold and the rh_local_* fetches): the windows of local_windows.h go
// through stage() and compute() chunk by chunk as fold-only batches, and the kernels here add each chunk's bp and up tables into
// band accumulators that stay on the device, divide by the window counts behind the last chunk, and scan the band for candidates.
//
// The mean of an entry is a plain double sum over the windows that contain it, in increasing window order, and one division by their
// number.  The accumulate kernel is a gather: a workgroup owns a row of the band, a lane an entry, and the lane adds its windows in
// order, carrying the partial sum from chunk to chunk in the accumulator -- so the result does not depend on the chunking, and no
// atomics are needed.  Row i - start(k) of window k's triangular table is contiguous in j, hence in d = j - i: reads and writes are
// coalesced, and every table entry of every window is read once.  A row starts from 0 in the first chunk that holds one of its
// windows (every letter lies in some window), so the accumulators are never cleared as a whole.
//
// Local hybridization (rh_local_duplex) runs the same chunks with a query in front of the windows: sequence 0 of every chunk is the
// query, pair k the query with window k, and local_hp_accumulate / local_hp_finish average the chunk's hp blocks into hp_loc by the
// same rule, next to the band of the windowed molecule, which the kernels above accumulate from sequences 1..c.
//
// Local hybridization of two windowed molecules (rh_local_duplex2) walks the grid of window pairs in rectangular tiles, each an
// indexed batch of windows of s1 followed by windows of s2 with all their pairs, and local_hp2_rows / local_hp2_add_rows /
// local_hp2_finish average the tiles' hp blocks into hp_loc2 in two levels -- per window of s1 the sum over the windows of s2 in a
// row buffer, then the sum of the finished rows -- so that the bits do not depend on the tiling.  Its result has buffers of its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ctx.h"
#include "kernels.h"

using namespace rh;
using namespace rh::host;

namespace {

constexpr int kLocalThreads = 256;
constexpr int kLocalGridRows = 65535;   // second grid dimension of the hp kernels: rows beyond it are walked

struct LocalAcc {
    LocalPlan P;
    const double* bp;    // the chunk's posteriors [k1 - k0][tri_stride], each the triangular table of We letters
    const double* up;    // [k1 - k0][up_stride], We * max_w entries used
    double* acc_bp;      // [n][ld]
    double* acc_up;      // [n][max_w]
    size_t tri_stride, up_stride;
    int k0, k1;          // the chunk: windows k0 .. k1 - 1
    int row0;            // first letter of window k0: workgroup b owns row row0 + b
    int max_w;
};

// the windows of the chunk that contain letters i .. i+len-1
__device__ __forceinline__ void chunk_range(const LocalAcc& A, int i, int len, int* lo, int* hi)
{
    local_window_range(A.P, i, len, lo, hi);
    if (*lo < A.k0) *lo = A.k0;
    if (*hi > A.k1 - 1) *hi = A.k1 - 1;
}

// grid: the rows row0 .. start(k1 - 1) + We - 1, which the windows of the chunk cover without a gap (S <= W)
__global__ __launch_bounds__(kLocalThreads) void local_accumulate(LocalAcc A)
{
    const int i = A.row0 + blockIdx.x;
    if (i >= A.P.n) return;
    int lo1, hi1;
    local_window_range(A.P, i, 1, &lo1, &hi1);
    const bool fresh = lo1 >= A.k0;   // the first chunk that touches this row: the sums start from 0
    const int We = A.P.We;
    for (int d = threadIdx.x; d < A.P.ld; d += kLocalThreads) {
        double* out = A.acc_bp + (size_t)i * A.P.ld + d;
        double s = fresh ? 0.0 : *out;
        int lo = 1, hi = 0;
        if (d >= 1) chunk_range(A, i, d + 1, &lo, &hi);
#pragma unroll 4
        for (int k = lo; k <= hi; k++) {
            const int ia = i - local_start(A.P, k) + 1;   // 1-based letter of the window; the pair is (ia, ia + d), ia + d <= We
            s += A.bp[(size_t)(k - A.k0) * A.tri_stride + (size_t)ia * (size_t)(2 * (We + 1) - ia - 1) / 2 + ia + d];
        }
        *out = s;
    }
    for (int w = threadIdx.x; w < A.max_w; w += kLocalThreads) {
        double* out = A.acc_up + (size_t)i * A.max_w + w;
        double s = fresh ? 0.0 : *out;
        int lo, hi;
        chunk_range(A, i, w + 1, &lo, &hi);
#pragma unroll 4
        for (int k = lo; k <= hi; k++)
            s += A.up[(size_t)(k - A.k0) * A.up_stride + (size_t)(i - local_start(A.P, k)) * A.max_w + w];
        *out = s;
    }
}

// sum -> mean, in place: grid (n), one division by the number of windows that contain the run; 0 where none does
__global__ __launch_bounds__(kLocalThreads) void local_finish(LocalPlan P, int max_w, double* __restrict__ bp, double* __restrict__ up)
{
    const int i = blockIdx.x;
    for (int d = threadIdx.x; d < P.ld + max_w; d += kLocalThreads) {
        const bool is_up = d >= P.ld;
        const int len = (is_up ? d - P.ld : d) + 1;
        double* v = is_up ? up + (size_t)i * max_w + (d - P.ld) : bp + (size_t)i * P.ld + d;
        int lo, hi;
        local_window_range(P, i, len, &lo, &hi);
        *v = hi >= lo ? *v / (double)(hi - lo + 1) : 0.0;
    }
}

// ---- hp_loc [(n1+1)][(n2+1)], row-major, 1-based, from the hp blocks of the chunk's pairs [k1 - k0][hp_stride] (row pitch ldd, 1-based:
// DxBatch::hp).  A lane owns one entry (i, j), lanes consecutive in j.  windowed = 2: pair k is (query, window k) and the lane reads
// block k at (i, j - start(k)); windowed = 1: (window k, query), read at (i - start(k), j).  Either way the reads of a wavefront are
// contiguous in j, like its writes.
struct LocalHpAcc {
    LocalPlan P;         // of the windowed molecule
    const double* hp;
    double* acc;
    size_t hp_stride;
    int ldd, n1, n2, windowed;
    int k0, k1;          // the chunk: windows k0 .. k1 - 1
    int t0, nt;          // the letters (0-based) of the windowed molecule its windows cover: t0 .. t0 + nt - 1, without a gap
};

// grid (column blocks, rows): only the columns (windowed = 2) or rows (windowed = 1) of the chunk's letters; rows beyond the grid's
// second dimension are walked
__global__ __launch_bounds__(kLocalThreads) void local_hp_accumulate(LocalHpAcc A)
{
    const bool w2 = A.windowed == 2;
    const int cols = w2 ? A.nt : A.n2, rows = w2 ? A.n1 : A.nt;
    const int col = blockIdx.x * kLocalThreads + threadIdx.x;
    if (col >= cols) return;
    const int j = (w2 ? A.t0 : 0) + 1 + col;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const int i = (w2 ? 0 : A.t0) + 1 + r;
        int lo, hi;
        local_window_range(A.P, (w2 ? j : i) - 1, 1, &lo, &hi);
        const bool fresh = lo >= A.k0;   // the first chunk that holds one of the letter's windows: the sum starts from 0
        if (lo < A.k0) lo = A.k0;
        if (hi > A.k1 - 1) hi = A.k1 - 1;
        double* out = A.acc + (size_t)i * ((size_t)A.n2 + 1) + j;
        double s = fresh ? 0.0 : *out;
#pragma unroll 4
        for (int k = lo; k <= hi; k++) {
            const int st = local_start(A.P, k);
            const double* blk = A.hp + (size_t)(k - A.k0) * A.hp_stride;
            s += w2 ? blk[(size_t)i * A.ldd + (j - st)] : blk[(size_t)(i - st) * A.ldd + j];
        }
        *out = s;
    }
}

// sum -> mean, in place, over all of (0..n1) x (0..n2): one division by the number of windows that contain the letter (at least one);
// row 0 and column 0 are written as 0
__global__ __launch_bounds__(kLocalThreads) void local_hp_finish(LocalPlan P, int n1, int n2, int windowed, double* __restrict__ hp)
{
    const int j = blockIdx.x * kLocalThreads + threadIdx.x;
    if (j > n2) return;
    for (int i = blockIdx.y; i <= n1; i += gridDim.y) {
        double* v = hp + (size_t)i * ((size_t)n2 + 1) + j;
        if (i == 0 || j == 0) { *v = 0.0; continue; }
        int lo, hi;
        local_window_range(P, (windowed == 2 ? j : i) - 1, 1, &lo, &hi);
        *v = *v / (double)(hi - lo + 1);
    }
}

// ---- hp_loc2 of two windowed molecules (rh_local_duplex2): the two-level form of the kernels above.  A tile holds the pairs of the
// windows kA .. kB-1 of s1 with the windows lA .. lB-1 of s2, pair (k - kA) * (lB - lA) + (l - lA), in the hp blocks of its batch.
// The sum over l goes into the row buffer R[a][ia][j] (a = k - kA, ia = 1..We1 the letter of window k, j = 0..n2, pitch n2 + 1) and
// is carried there across the column tiles of a row block; behind the last column tile the rows of the block are added into hp_loc2
// in increasing k, which carries the sum over k from row block to row block.  Both are gathers with lanes consecutive in j.
struct LocalHp2 {
    LocalPlan P1, P2;    // of s1 and of s2
    const double* hp;    // the tile's hp blocks [(kB - kA) * (lB - lA)][hp_stride], row pitch ldd, 1-based
    double* R;           // [kB - kA][We1 + 1][n2 + 1]
    double* acc;         // hp_loc2 [(n1+1)][(n2+1)]
    size_t hp_stride;
    int ldd;
    int kA, kB, lA, lB;
};

// grid (column blocks, lines): only the columns the tile's windows of s2 cover, which they do without a gap; a line is one (a, ia),
// lines beyond the grid's second dimension are walked.  A column starts from 0 in the first column tile that holds one of its windows.
__global__ __launch_bounds__(kLocalThreads) void local_hp2_rows(LocalHp2 A)
{
    const int t0 = local_start(A.P2, A.lA), nt = local_start(A.P2, A.lB - 1) + A.P2.We - t0;
    const int col = blockIdx.x * kLocalThreads + threadIdx.x;
    if (col >= nt) return;
    const int j = t0 + 1 + col;
    int lo, hi;
    local_window_range(A.P2, j - 1, 1, &lo, &hi);
    const bool fresh = lo >= A.lA;
    if (lo < A.lA) lo = A.lA;
    if (hi > A.lB - 1) hi = A.lB - 1;
    const int nc = A.lB - A.lA, We1 = A.P1.We, lines = (A.kB - A.kA) * We1;
    const size_t pitch = (size_t)A.P2.n + 1;
    for (int r = blockIdx.y; r < lines; r += gridDim.y) {
        const int a = r / We1, ia = r - a * We1 + 1;
        double* out = A.R + ((size_t)a * (size_t)(We1 + 1) + ia) * pitch + j;
        double s = fresh ? 0.0 : *out;
#pragma unroll 4
        for (int l = lo; l <= hi; l++)
            s += A.hp[((size_t)a * nc + (l - A.lA)) * A.hp_stride + (size_t)ia * A.ldd + (j - local_start(A.P2, l))];
        *out = s;
    }
}

// grid (column blocks over 1..n2, rows): the rows of s1 the block's windows cover, without a gap; rows beyond the grid's second
// dimension are walked.  A row starts from 0 in the first row block that holds one of its windows.
__global__ __launch_bounds__(kLocalThreads) void local_hp2_add_rows(LocalHp2 A)
{
    const int j = 1 + blockIdx.x * kLocalThreads + threadIdx.x;
    if (j > A.P2.n) return;
    const int i0 = local_start(A.P1, A.kA), ni = local_start(A.P1, A.kB - 1) + A.P1.We - i0, We1 = A.P1.We;
    const size_t pitch = (size_t)A.P2.n + 1;
    for (int r = blockIdx.y; r < ni; r += gridDim.y) {
        const int i = i0 + 1 + r;
        int lo, hi;
        local_window_range(A.P1, i - 1, 1, &lo, &hi);
        const bool fresh = lo >= A.kA;
        if (lo < A.kA) lo = A.kA;
        if (hi > A.kB - 1) hi = A.kB - 1;
        double* out = A.acc + (size_t)i * pitch + j;
        double s = fresh ? 0.0 : *out;
#pragma unroll 4
        for (int k = lo; k <= hi; k++)
            s += A.R[((size_t)(k - A.kA) * (size_t)(We1 + 1) + (i - local_start(A.P1, k))) * pitch + j];
        *out = s;
    }
}

// sum -> mean, in place, over all of (0..n1) x (0..n2): one division by the product of the two window counts (each at least one, the
// product exact in double); row 0 and column 0 are written as 0
__global__ __launch_bounds__(kLocalThreads) void local_hp2_finish(LocalPlan P1, LocalPlan P2, double* __restrict__ hp)
{
    const int j = blockIdx.x * kLocalThreads + threadIdx.x;
    if (j > P2.n) return;
    int lo, hi;
    local_window_range(P2, j - 1, 1, &lo, &hi);
    const double c2 = (double)(hi - lo + 1);
    for (int i = blockIdx.y; i <= P1.n; i += gridDim.y) {
        double* v = hp + (size_t)i * ((size_t)P2.n + 1) + j;
        if (i == 0 || j == 0) { *v = 0.0; continue; }
        local_window_range(P1, i - 1, 1, &lo, &hi);
        *v = *v / ((double)(hi - lo + 1) * c2);
    }
}

// ---- ordered threshold compaction over the band or over up, as candidates.hip does it for a batch: one wavefront per row, the
// probability narrowed to float before the comparison.  Row i holds the entries e0 .. min(width - 1, last - i) at base[i*pitch + e];
// bp: e = d, e0 = 1, last = n - 1, record (i + 1, i + 1 + d); up: e = w, e0 = 0, last = any, record (i, w); hp: the rows 1..n1 of
// hp_loc (base = its row 1), e = j, e0 = 1, last = any, record (i + 1, j).
enum LocalScanKind { kScanBp = 0, kScanUp, kScanHp };
struct LocalScan {
    const double* base;
    int n, pitch, width, e0, last, kind;
    float th;
};
__device__ __forceinline__ int scan_end(const LocalScan& V, int i) { return min(V.width - 1, V.last - i); }

__global__ __launch_bounds__(256) void local_cand_count(LocalScan V, int* __restrict__ counts)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= V.n) return;
    const double* p = V.base + (size_t)i * V.pitch;
    const int e1 = scan_end(V, i);
    int c = 0;
    for (int e = V.e0 + lane; e <= e1; e += 64) c += ((float)p[e] > V.th) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) counts[i] = c;
}
__global__ __launch_bounds__(256) void local_cand_write(LocalScan V, const int* __restrict__ counts, const int* __restrict__ offsets,
                                                        rh_cand* __restrict__ out, int cap)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= V.n) return;
    if (counts[i] == 0) return;
    const double* p = V.base + (size_t)i * V.pitch;
    const int e1 = scan_end(V, i);
    int pos = offsets[i];
    for (int eb = V.e0; eb <= e1; eb += 64) {
        const int e = eb + lane;
        const float pf = e <= e1 ? (float)p[e] : 0.0f;
        const bool hit = e <= e1 && pf > V.th;
        const unsigned long long m = __ballot(hit);
        if (hit) {
            const int k = pos + __popcll(m & ((1ull << lane) - 1ull));
            if (k < cap) {
                rh_cand r;
                r.i = V.kind == kScanUp ? i : i + 1;
                r.j = V.kind == kScanBp ? i + 1 + e : e;
                r.p = pf;
                out[k] = r;
            }
        }
        pos += __popcll(m);
    }
}

// an event pair that goes with its scope
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t create() { hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// the table counts the context's model sizes a chunk by (staging.hip)
LocalTables local_tables(const rh_ctx* c)
{
    const bool vienna = c->model == RH_MODEL_VIENNA_BL;
    LocalTables T;
    T.fold = vienna ? (int)VM_COUNT : (int)T_COUNT;
    T.dx = std::max((int)D_COUNT, (int)V_COUNT);
    T.dxl = !vienna ? (int)DL_COUNT : c->vienna_sem == kViennaSem20 ? (int)VD_COUNT20 : (int)VD_COUNT;
    T.cofold = vienna && c->hybrid == RH_HYBRID_COFOLD;
    return T;
}

// windows per chunk: what rh_set_local_chunk asked for, or the largest count whose tables stay under kLocalChunkBytes; D: the chunks
// of rh_local_duplex, which hold the query as well
int chunk_windows(const rh_ctx* c, const LocalPlan& P, const LocalDuplexPlan* D)
{
    int chunk = c->loc_chunk;
    if (chunk <= 0) chunk = D ? local_duplex_chunk_auto(*D, local_tables(c)) : local_chunk_auto(P, local_tables(c));
    if (D) chunk = std::min(chunk, kLocalChunkMax - 1);
    return std::min(chunk, P.nw);
}

int local_ready(rh_ctx* c)
{
    if (!c->loc_valid) return fail(c, RH_ERR_ARG, "no local fold result");
    return RH_OK;
}

int local_hp_ready(rh_ctx* c)
{
    if (!c->loc_valid || !c->loc_hp_valid) return fail(c, RH_ERR_ARG, "no local hybridization result");
    return RH_OK;
}

// The scheduler of rh_local_fold (D == nullptr) and rh_local_duplex over checked arguments: chunks of consecutive windows of `seq`,
// each one batch through stage() and compute() -- fold-only, or indexed with the query as sequence 0 and the pairs (0, k) / (k, 0) --
// and behind each compute the accumulate kernels, behind the last one the finish kernels.
int local_run(rh_ctx* c, const LocalPlan& P, const char* seq, const LocalDuplexPlan* D, const char* query)
{
    int rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->loc_valid = c->loc_hp_valid = false;
    const int max_w = c->max_w;
    const int q = D ? 1 : 0;   // sequences in front of the windows
    if ((rc = ensure(c, c->d_loc_bp, sizeof(double) * local_band_size(P), false))) return rc;
    if ((rc = ensure(c, c->d_loc_up, sizeof(double) * local_up_size(P, max_w), false))) return rc;
    if ((rc = ensure(c, c->d_loc_logz, sizeof(double) * P.nw, false))) return rc;
    if (D && (rc = ensure(c, c->d_loc_hp, sizeof(double) * local_hp_size(*D), false))) return rc;
    if (D && (rc = ensure(c, c->d_loc_logzp, sizeof(double) * P.nw, false))) return rc;
    EventPair ev;
    HIP_TRY(c, ev.create());
    const int chunk = chunk_windows(c, P, D);
    std::vector<const char*> seqs((size_t)chunk + q);
    std::vector<int> lens((size_t)chunk + q, P.We), first, second;
    if (D) {
        seqs[0] = query; lens[0] = D->nq;
        first.assign((size_t)chunk, 0); second.assign((size_t)chunk, 0);
        std::vector<int>& win = D->windowed == 2 ? second : first;
        for (int k = 0; k < chunk; k++) win[k] = 1 + k;
    }
    double ms_fold = 0.0, ms_acc = 0.0;
    float t = 0.f;
    for (int k0 = 0; k0 < P.nw; k0 += chunk) {
        const int k1 = std::min(P.nw, k0 + chunk);
        for (int k = k0; k < k1; k++) seqs[q + k - k0] = seq + local_start(P, k);
        BatchRequest r;
        r.ns = q + k1 - k0; r.seqs = seqs.data(); r.lens = lens.data();
        r.with_mc = true;
        if (D) { r.with_dx = true; r.npairs = k1 - k0; r.first = first.data(); r.second = second.data(); }
        if ((rc = stage(c, r))) return rc;
        // One window (W >= n) is the pair itself, and the call answers with the bits of rh_duplex: under RH_HYBRID_COFOLD that call
        // has no folds to seed its two-molecule sweeps from, and seeded sweeps differ from it in the last bits on the scaled linear
        // kernels -- so this one compute runs them unseeded too.  With two windows or more every chunk is seeded, like any batch.
        const int seed = c->co_seed;
        if (D && P.nw == 1) c->co_seed = 0;
        rc = compute(c);
        c->co_seed = seed;
        if (rc) return rc;
        ms_fold += c->ms[3];
        LocalAcc A{};
        A.P = P;
        A.tri_stride = c->mc.tri_stride; A.up_stride = (size_t)c->mc.ld * max_w;
        A.bp = c->d_bp.as<const double>() + q * A.tri_stride; A.up = c->d_up.as<const double>() + q * A.up_stride;
        A.acc_bp = c->d_loc_bp.as<double>(); A.acc_up = c->d_loc_up.as<double>();
        A.k0 = k0; A.k1 = k1; A.row0 = local_start(P, k0); A.max_w = max_w;
        const int rows = local_start(P, k1 - 1) + P.We - A.row0;
        HIP_TRY(c, hipEventRecord(ev.a, c->s_mc));
        hipLaunchKernelGGL(local_accumulate, dim3(rows), dim3(kLocalThreads), 0, c->s_mc, A);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(c->d_loc_logz.as<double>() + k0, c->d_mclogz.as<const double>() + q, sizeof(double) * (k1 - k0), hipMemcpyDeviceToDevice, c->s_mc));
        if (D) {
            LocalHpAcc H{};
            H.P = P;
            H.hp = c->d_hp.as<const double>(); H.acc = c->d_loc_hp.as<double>();
            H.hp_stride = c->dx.tab_stride; H.ldd = c->dx.ldd;
            H.n1 = D->n1; H.n2 = D->n2; H.windowed = D->windowed;
            H.k0 = k0; H.k1 = k1; H.t0 = A.row0; H.nt = rows;
            const int cols = D->windowed == 2 ? rows : D->n2, lines = D->windowed == 2 ? D->n1 : rows;
            hipLaunchKernelGGL(local_hp_accumulate, dim3((cols + kLocalThreads - 1) / kLocalThreads, std::min(lines, kLocalGridRows)), dim3(kLocalThreads), 0, c->s_mc, H);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(c->d_loc_logzp.as<double>() + k0, c->d_logz.p, sizeof(double) * (k1 - k0), hipMemcpyDeviceToDevice, c->s_mc));
        }
        if (k1 == P.nw) {
            hipLaunchKernelGGL(local_finish, dim3(P.n), dim3(kLocalThreads), 0, c->s_mc, P, max_w, A.acc_bp, A.acc_up);
            HIP_TRY(c, hipGetLastError());
            if (D) {
                hipLaunchKernelGGL(local_hp_finish, dim3((D->n2 + 1 + kLocalThreads - 1) / kLocalThreads, std::min(D->n1 + 1, kLocalGridRows)), dim3(kLocalThreads), 0,
                                   c->s_mc, P, D->n1, D->n2, D->windowed, c->d_loc_hp.as<double>());
                HIP_TRY(c, hipGetLastError());
            }
        }
        HIP_TRY(c, hipEventRecord(ev.b, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));   // (the next chunk's stage() reuses the tables this one read)
        HIP_TRY(c, hipEventElapsedTime(&t, ev.a, ev.b));
        ms_acc += t;
    }
    c->loc = P; c->loc_max_w = max_w;
    c->loc_ms[0] = ms_fold; c->loc_ms[1] = ms_acc;
    c->loc_valid = true;
    if (D) { c->loc_hp = *D; c->loc_hp_valid = true; }
    return RH_OK;
}

int local_hp2_ready(rh_ctx* c)
{
    if (!c->loc2_valid) return fail(c, RH_ERR_ARG, "no local hybridization result of two windowed molecules");
    return RH_OK;
}

// The scheduler of rh_local_duplex2 over checked arguments: the tiles of local_windows.h, row blocks in increasing k and inside a row
// block column tiles in increasing l, each one indexed batch with folds through stage() and compute() -- sequences 0..nr-1 the
// windows of s1, nr..nr+nc-1 those of s2, pair a * nc + b = (a, nr + b).  Behind every compute the row kernel and the copy of the
// tile's log Z, behind the last column tile of a row block the add kernel, behind the last row block the finish kernel.
int local2_run(rh_ctx* c, const LocalDuplex2Plan& D, const char* s1, const char* s2)
{
    int rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->loc2_valid = false;
    const LocalPlan &P1 = D.P1, &P2 = D.P2;
    int rows = c->loc2_tile[0], cols = c->loc2_tile[1];
    if (rows <= 0 || cols <= 0) local_tile_auto(D, local_tables(c), &rows, &cols);
    rows = std::min(rows, P1.nw); cols = std::min(cols, P2.nw);
    if ((rc = ensure(c, c->d_loc2_hp, sizeof(double) * local_hp2_size(D), false))) return rc;
    if ((rc = ensure(c, c->d_loc2_rows, sizeof(double) * local_hp2_rowbuf_size(D, rows), false))) return rc;
    if ((rc = ensure(c, c->d_loc2_logz, sizeof(double) * local_hp2_logz_size(D), false))) return rc;
    EventPair ev;
    HIP_TRY(c, ev.create());
    std::vector<const char*> seqs((size_t)rows + cols);
    std::vector<int> lens((size_t)rows + cols), first((size_t)rows * cols), second((size_t)rows * cols);
    LocalHp2 A{};
    A.P1 = P1; A.P2 = P2;
    A.R = c->d_loc2_rows.as<double>(); A.acc = c->d_loc2_hp.as<double>();
    const int col_blocks = (P2.n + kLocalThreads - 1) / kLocalThreads;
    double ms_compute = 0.0, ms_acc = 0.0;
    float t = 0.f;
    LocalTile tile;
    for (size_t ti = 0; local_tile_at(D, rows, cols, ti, &tile); ti++) {
        const int kA = tile.kA, kB = tile.kB, lA = tile.lA, lB = tile.lB, nr = kB - kA, nc = lB - lA;
        for (int a = 0; a < nr; a++) { seqs[a] = s1 + local_start(P1, kA + a); lens[a] = P1.We; }
        for (int b = 0; b < nc; b++) { seqs[nr + b] = s2 + local_start(P2, lA + b); lens[nr + b] = P2.We; }
        for (int a = 0; a < nr; a++)
            for (int b = 0; b < nc; b++) { first[(size_t)a * nc + b] = a; second[(size_t)a * nc + b] = nr + b; }
        BatchRequest r;
        r.ns = nr + nc; r.seqs = seqs.data(); r.lens = lens.data();
        r.with_mc = true; r.with_dx = true;
        r.npairs = nr * nc; r.first = first.data(); r.second = second.data();
        if ((rc = stage(c, r))) return rc;
        // one window pair is the pair itself and answers with the bits of rh_duplex: its one compute runs unseeded, as in local_run
        const int seed = c->co_seed;
        if (P1.nw == 1 && P2.nw == 1) c->co_seed = 0;
        rc = compute(c);
        c->co_seed = seed;
        if (rc) return rc;
        ms_compute += c->ms[3];
        A.hp = c->d_hp.as<const double>(); A.hp_stride = c->dx.tab_stride; A.ldd = c->dx.ldd;
        A.kA = kA; A.kB = kB; A.lA = lA; A.lB = lB;
        const int nt = local_start(P2, lB - 1) + P2.We - local_start(P2, lA);
        HIP_TRY(c, hipEventRecord(ev.a, c->s_mc));
        hipLaunchKernelGGL(local_hp2_rows, dim3((nt + kLocalThreads - 1) / kLocalThreads, std::min(nr * P1.We, kLocalGridRows)), dim3(kLocalThreads), 0,
                           c->s_mc, A);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpy2DAsync(c->d_loc2_logz.as<double>() + (size_t)kA * P2.nw + lA, sizeof(double) * P2.nw, c->d_logz.p, sizeof(double) * nc,
                                    sizeof(double) * nc, nr, hipMemcpyDeviceToDevice, c->s_mc));
        if (lB == P2.nw) {
            const int ni = local_start(P1, kB - 1) + P1.We - local_start(P1, kA);
            hipLaunchKernelGGL(local_hp2_add_rows, dim3(col_blocks, std::min(ni, kLocalGridRows)), dim3(kLocalThreads), 0, c->s_mc, A);
            HIP_TRY(c, hipGetLastError());
            if (kB == P1.nw) {
                hipLaunchKernelGGL(local_hp2_finish, dim3((P2.n + 1 + kLocalThreads - 1) / kLocalThreads, std::min(P1.n + 1, kLocalGridRows)),
                                   dim3(kLocalThreads), 0, c->s_mc, P1, P2, A.acc);
                HIP_TRY(c, hipGetLastError());
            }
        }
        HIP_TRY(c, hipEventRecord(ev.b, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));   // (the next tile's stage() reuses the tables this one read)
        HIP_TRY(c, hipEventElapsedTime(&t, ev.a, ev.b));
        ms_acc += t;
    }
    c->loc2 = D;
    c->loc2_used[0] = rows; c->loc2_used[1] = cols;
    c->loc2_ms[0] = ms_compute; c->loc2_ms[1] = ms_acc;
    c->loc2_valid = true;
    return RH_OK;
}

// count, prefix on the host, ordered write: the scan V into out[0 .. cap), the kernel time added to *ms; returns the total found
int scan_candidates(rh_ctx* c, const LocalScan& V, rh_cand* out, int cap, double* ms, const char* who)
{
    const int n = V.n;
    int rc;
    if ((rc = ensure(c, c->d_cnt, sizeof(int) * 2 * ((size_t)n + 1), false))) return rc;
    int* d_counts = c->d_cnt.as<int>();
    int* d_offsets = d_counts + (n + 1);
    EventPair ev;
    HIP_TRY(c, ev.create());
    float t = 0.f;
    HIP_TRY(c, hipEventRecord(ev.a, c->s_mc));
    hipLaunchKernelGGL(local_cand_count, dim3((n + 3) / 4), dim3(256), 0, c->s_mc, V, d_counts);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.b, c->s_mc));
    std::vector<int> counts(n), offsets(n);
    HIP_TRY(c, hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * n, hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    HIP_TRY(c, hipEventElapsedTime(&t, ev.a, ev.b));
    *ms += t;
    long long found = 0;
    for (int i = 0; i < n; i++) { offsets[i] = (int)std::min<long long>(found, cap); found += counts[i]; }
    if (found > 0x7fffffffLL) return fail(c, RH_ERR_UNSUPPORTED, "%s: %lld entries above the threshold", who, found);
    const int take = (int)std::min<long long>(found, cap);
    if (take > 0) {
        if ((rc = ensure(c, c->d_cand, sizeof(rh_cand) * (size_t)take, false))) return rc;
        HIP_TRY(c, hipMemcpyAsync(d_offsets, offsets.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->s_mc));
        HIP_TRY(c, hipEventRecord(ev.a, c->s_mc));
        hipLaunchKernelGGL(local_cand_write, dim3((n + 3) / 4), dim3(256), 0, c->s_mc, V, d_counts, d_offsets, c->d_cand.as<rh_cand>(), take);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(ev.b, c->s_mc));
        HIP_TRY(c, hipMemcpyAsync(out, c->d_cand.p, sizeof(rh_cand) * (size_t)take, hipMemcpyDeviceToHost, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));
        HIP_TRY(c, hipEventElapsedTime(&t, ev.a, ev.b));
        *ms += t;
    }
    return (int)found;
}

}  // namespace

extern "C" {

int rh_set_local_chunk(rh_ctx* c, int windows)
{
    if (!c) return RH_ERR_ARG;
    if (windows < 0 || windows > kLocalChunkMax) return fail(c, RH_ERR_ARG, "rh_set_local_chunk: %d windows outside [0, %d]", windows, kLocalChunkMax);
    c->loc_chunk = windows;
    return RH_OK;
}

int rh_local_fold(rh_ctx* c, const char* seq, int n, int window, int step)
{
    if (!c) return RH_ERR_ARG;
    LocalPlan P;
    std::string why;
    if (int rc = local_check(seq, n, window, step, &P, &why)) return fail(c, rc, "%s", why.c_str());
    return local_run(c, P, seq, nullptr, nullptr);
}

int rh_local_duplex(rh_ctx* c, const char* s1, int n1, const char* s2, int n2, int windowed, int window, int step)
{
    if (!c) return RH_ERR_ARG;
    LocalDuplexPlan D;
    std::string why;
    if (int rc = local_duplex_check(s1, n1, s2, n2, windowed, window, step, &D, &why)) return fail(c, rc, "%s", why.c_str());
    return local_run(c, D.P, windowed == 1 ? s1 : s2, &D, windowed == 1 ? s2 : s1);
}

int rh_local_hp_layout(rh_ctx* c, int* n1, int* n2, int* windowed, int* nw)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp_ready(c)) return rc;
    if (n1) *n1 = c->loc_hp.n1;
    if (n2) *n2 = c->loc_hp.n2;
    if (windowed) *windowed = c->loc_hp.windowed;
    if (nw) *nw = c->loc_hp.P.nw;
    return RH_OK;
}

int rh_local_hp_results(rh_ctx* c, double* hp, double* logz_pair)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp_ready(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (hp) HIP_TRY(c, hipMemcpyAsync(hp, c->d_loc_hp.p, sizeof(double) * local_hp_size(c->loc_hp), hipMemcpyDeviceToHost, c->s_mc));
    if (logz_pair) HIP_TRY(c, hipMemcpyAsync(logz_pair, c->d_loc_logzp.p, sizeof(double) * c->loc_hp.P.nw, hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    return RH_OK;
}

int rh_local_layout(rh_ctx* c, int* n, int* ld, int* nw, int* max_w, int* starts)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_ready(c)) return rc;
    if (n) *n = c->loc.n;
    if (ld) *ld = c->loc.ld;
    if (nw) *nw = c->loc.nw;
    if (max_w) *max_w = c->loc_max_w;
    for (int k = 0; starts && k < c->loc.nw; k++) starts[k] = local_start(c->loc, k);
    return RH_OK;
}

int rh_local_results(rh_ctx* c, double* bp_band, double* up, double* logz_win)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_ready(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (bp_band) HIP_TRY(c, hipMemcpyAsync(bp_band, c->d_loc_bp.p, sizeof(double) * local_band_size(c->loc), hipMemcpyDeviceToHost, c->s_mc));
    if (up) HIP_TRY(c, hipMemcpyAsync(up, c->d_loc_up.p, sizeof(double) * local_up_size(c->loc, c->loc_max_w), hipMemcpyDeviceToHost, c->s_mc));
    if (logz_win) HIP_TRY(c, hipMemcpyAsync(logz_win, c->d_loc_logz.p, sizeof(double) * c->loc.nw, hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    return RH_OK;
}

int rh_local_candidates(rh_ctx* c, int what, float threshold, rh_cand* out, int cap)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = what == 2 ? local_hp_ready(c) : local_ready(c)) return rc;
    if (what < 0 || what > 2 || cap < 0 || (cap > 0 && !out)) return fail(c, RH_ERR_ARG, "rh_local_candidates: bad what/cap");
    HIP_TRY(c, hipSetDevice(c->device));
    const LocalPlan& P = c->loc;
    const int hp_ld = c->loc_hp.n2 + 1;
    const int n = what == 2 ? c->loc_hp.n1 : P.n;   // rows of the scan
    const LocalScan V = what == 0   ? LocalScan{c->d_loc_bp.as<const double>(), n, P.ld, P.ld, 1, n - 1, kScanBp, threshold}
                        : what == 1 ? LocalScan{c->d_loc_up.as<const double>(), n, c->loc_max_w, c->loc_max_w, 0, n - 1 + c->loc_max_w, kScanUp, threshold}
                                    : LocalScan{c->d_loc_hp.as<const double>() + hp_ld, n, hp_ld, hp_ld, 1, 0x3fffffff, kScanHp, threshold};
    return scan_candidates(c, V, out, cap, &c->loc_ms[1], "rh_local_candidates");
}

int rh_local_times(rh_ctx* c, double ms[2])
{
    if (!c || !ms) return RH_ERR_ARG;
    if (int rc = local_ready(c)) return rc;
    ms[0] = c->loc_ms[0]; ms[1] = c->loc_ms[1];
    return RH_OK;
}

int rh_set_local_tile(rh_ctx* c, int rows, int cols)
{
    if (!c) return RH_ERR_ARG;
    const bool automatic = rows == 0 && cols == 0;
    if (!automatic && (rows < 1 || cols < 1 || (long long)rows + cols > kLocalChunkMax || (long long)rows * cols > kLocalChunkMax - 1))
        return fail(c, RH_ERR_ARG, "rh_set_local_tile: %d x %d windows (0, 0, or rows + cols <= %d and rows * cols <= %d)", rows, cols, kLocalChunkMax,
                    kLocalChunkMax - 1);
    c->loc2_tile[0] = rows; c->loc2_tile[1] = cols;
    return RH_OK;
}

int rh_local_duplex2(rh_ctx* c, const char* s1, int n1, const char* s2, int n2, int window1, int step1, int window2, int step2)
{
    if (!c) return RH_ERR_ARG;
    LocalDuplex2Plan D;
    std::string why;
    if (int rc = local_duplex2_check(s1, n1, s2, n2, window1, step1, window2, step2, &D, &why)) return fail(c, rc, "%s", why.c_str());
    return local2_run(c, D, s1, s2);
}

int rh_local_hp2_layout(rh_ctx* c, int* n1, int* n2, int* nw1, int* nw2, int* starts1, int* starts2)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp2_ready(c)) return rc;
    const LocalPlan &P1 = c->loc2.P1, &P2 = c->loc2.P2;
    if (n1) *n1 = P1.n;
    if (n2) *n2 = P2.n;
    if (nw1) *nw1 = P1.nw;
    if (nw2) *nw2 = P2.nw;
    for (int k = 0; starts1 && k < P1.nw; k++) starts1[k] = local_start(P1, k);
    for (int l = 0; starts2 && l < P2.nw; l++) starts2[l] = local_start(P2, l);
    return RH_OK;
}

int rh_local_hp2_results(rh_ctx* c, double* hp, double* logz_pair)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp2_ready(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (hp) HIP_TRY(c, hipMemcpyAsync(hp, c->d_loc2_hp.p, sizeof(double) * local_hp2_size(c->loc2), hipMemcpyDeviceToHost, c->s_mc));
    if (logz_pair) HIP_TRY(c, hipMemcpyAsync(logz_pair, c->d_loc2_logz.p, sizeof(double) * local_hp2_logz_size(c->loc2), hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    return RH_OK;
}

int rh_local_hp2_candidates(rh_ctx* c, float threshold, rh_cand* out, int cap)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp2_ready(c)) return rc;
    if (cap < 0 || (cap > 0 && !out)) return fail(c, RH_ERR_ARG, "rh_local_hp2_candidates: bad cap");
    HIP_TRY(c, hipSetDevice(c->device));
    const int n1 = c->loc2.P1.n, hp_ld = c->loc2.P2.n + 1;
    const LocalScan V{c->d_loc2_hp.as<const double>() + hp_ld, n1, hp_ld, hp_ld, 1, 0x3fffffff, kScanHp, threshold};
    return scan_candidates(c, V, out, cap, &c->loc2_ms[1], "rh_local_hp2_candidates");
}

int rh_local_hp2_tile(rh_ctx* c, int* rows, int* cols)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp2_ready(c)) return rc;
    if (rows) *rows = c->loc2_used[0];
    if (cols) *cols = c->loc2_used[1];
    return RH_OK;
}

int rh_local_hp2_times(rh_ctx* c, double ms[2])
{
    if (!c || !ms) return RH_ERR_ARG;
    if (int rc = local_hp2_ready(c)) return rc;
    ms[0] = c->loc2_ms[0]; ms[1] = c->loc2_ms[1];
    return RH_OK;
}

}  // extern "C"
