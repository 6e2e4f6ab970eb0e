// local_fold.hip -- the local calls (rh_local_fold, rh_local_duplex, rh_local_duplex2 and the rh_local_* fetches): one walk over tiles of
// windows, the kernels that average what each tile computed into results that stay on the device, and the candidate scans of those.
//
// The walk (local_walk) covers the grid of (window k of s1, window l of s2) in tiles of `rows` x `cols` windows (local_windows.h), each
// tile one batch through stage() and compute(): its windows as sequences, all their pairs.  rh_local_duplex2 is that walk as it
// stands.  rh_local_duplex is the walk with the query as the one window of its molecule, in tiles of 1 x chunk or chunk x 1 windows;
// rh_local_fold is the walk without a second molecule, in fold-only chunks of windows of s1.
//
// Band.  The mean of an entry of bp_band / up is a plain double sum over the windows that contain it, in increasing window order, and
// one division by their number.  The accumulate kernel is a gather: a workgroup owns a row of the band, a lane an entry, and the lane
// adds its windows in order, carrying the partial sum from chunk to chunk in the accumulator -- so the result does not depend on the
// chunking, and no atomics are needed.  Row i - start(k) of window k's triangular table is contiguous in j, hence in d = j - i: reads
// and writes are coalesced, and every table entry of every window is read once.  A row starts from 0 in the first chunk that holds one
// of its windows (every letter lies in some window), so the accumulators are never cleared as a whole.  rh_local_fold accumulates the
// band of its molecule, rh_local_duplex that of the molecule it cuts, next to hp.
//
// hp.  hp_loc(i, j) is a sum in two levels -- per window of s1 the sum over the windows of s2 that contain j, then the sum of those
// rows over the windows of s1 that contain i, each in increasing window order -- and one division by the product of the two counts, so
// that the bits do not depend on the tiling.  Two gathers by the rule of the band (column gather, row gather) and a finish kernel do
// it; where a molecule has one window its level adds one term to 0.0 and is skipped (the three routes: local_walk).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
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

// ---- hp_loc [(n1+1)][(n2+1)], row-major, 1-based, pitch n2 + 1.  A tile holds the pairs of the windows kA .. kB-1 of s1 with the
// windows lA .. lB-1 of s2, pair (k - kA) * (lB - lA) + (l - lA), in the hp blocks of its batch (row pitch ldd, 1-based: DxBatch::hp).
// The sum over l makes rows[a][ia][j] (a = k - kA, ia = 1..We1 the letter of window k, j = 0..n2, pitch n2 + 1), carried across the
// column tiles of a row block; behind the last column tile the rows of the block are added into hp_loc in increasing k, which
// carries the sum over k from row block to row block.  Both are gathers: a lane owns one entry, lanes consecutive in j, so the reads
// of a wavefront are contiguous like its writes.
struct LocalHpGather {
    LocalPlan P1, P2;    // of s1 and of s2
    const double* src;   // blocks of src_stride doubles, row pitch src_pitch, 1-based: the column gather reads the tile's hp blocks
    size_t src_stride;   // [(kB - kA) * (lB - lA)], the row gather the finished rows of the row block [kB - kA]
    int src_pitch;
    double* dst;         // column gather: the rows, a-th block at dst + a * dst_stride; row gather: hp_loc
    size_t dst_stride;
    int kA, kB, lA, lB;
};

// grid (column blocks, lines): only the columns the tile's windows of s2 cover, which they do without a gap; a line is one (a, ia),
// lines beyond the grid's second dimension are walked.  A column starts from 0 in the first column tile that holds one of its windows.
__global__ __launch_bounds__(kLocalThreads) void local_hp_col_gather(LocalHpGather A)
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
        double* out = A.dst + (size_t)a * A.dst_stride + (size_t)ia * pitch + j;
        double s = fresh ? 0.0 : *out;
#pragma unroll 4
        for (int l = lo; l <= hi; l++)
            s += A.src[((size_t)a * nc + (l - A.lA)) * A.src_stride + (size_t)ia * A.src_pitch + (j - local_start(A.P2, l))];
        *out = s;
    }
}

// grid (column blocks over 1..n2, rows): the rows of s1 the block's windows cover, without a gap; rows beyond the grid's second
// dimension are walked.  A row starts from 0 in the first row block that holds one of its windows.
__global__ __launch_bounds__(kLocalThreads) void local_hp_row_gather(LocalHpGather A)
{
    const int j = 1 + blockIdx.x * kLocalThreads + threadIdx.x;
    if (j > A.P2.n) return;
    const int i0 = local_start(A.P1, A.kA), ni = local_start(A.P1, A.kB - 1) + A.P1.We - i0;
    const size_t pitch = (size_t)A.P2.n + 1;
    for (int r = blockIdx.y; r < ni; r += gridDim.y) {
        const int i = i0 + 1 + r;
        int lo, hi;
        local_window_range(A.P1, i - 1, 1, &lo, &hi);
        const bool fresh = lo >= A.kA;
        if (lo < A.kA) lo = A.kA;
        if (hi > A.kB - 1) hi = A.kB - 1;
        double* out = A.dst + (size_t)i * pitch + j;
        double s = fresh ? 0.0 : *out;
#pragma unroll 4
        for (int k = lo; k <= hi; k++)
            s += A.src[(size_t)(k - A.kA) * A.src_stride + (size_t)(i - local_start(A.P1, k)) * A.src_pitch + j];
        *out = s;
    }
}

// sum -> mean, in place, over all of (0..n1) x (0..n2): one division by the product of the two window counts (each at least one, the
// product exact in double, and the other count itself where one of them is 1); row 0 and column 0 are written as 0
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
    if (!c->loc_valid || !c->loc_hp.valid) return fail(c, RH_ERR_ARG, "no local hybridization result");
    return RH_OK;
}

int local_hp2_ready(rh_ctx* c)
{
    if (!c->loc_hp2.valid) return fail(c, RH_ERR_ARG, "no local hybridization result of two windowed molecules");
    return RH_OK;
}

// What a local call asks of the walk, over checked arguments.
struct LocalWalk {
    LocalDuplex2Plan D;          // of s1 and of s2; P2.nw = 0: no second molecule, fold-only batches without pairs
    const char* s1 = nullptr;
    const char* s2 = nullptr;
    int rows = 0, cols = 0;      // windows of s1 x windows of s2 in a tile, clipped to nw1 / nw2
    int band = 0;                // the side (1 or 2; 0: none) whose windows also go into the band accumulators, as rh_local_fold's do
    int front = 1;               // the side whose windows stand first in a tile's batch
    LocalHp* out = nullptr;      // the hp result it writes (none without a second molecule) ...
    double* ms = nullptr;        // ... and its time pair: the tiles' computes, the kernels here
};

// The scheduler of the three local calls: row blocks in increasing k and inside a row block column tiles in increasing l
// (local_tile_at), each tile one batch with folds through stage() and compute().  Pair a * nc + b is (window kA + a of s1, window
// lA + b of s2); the windows of the front side are sequences 0.., those of the other side follow.  Behind every compute the
// gathers and the copies of log Z, behind the last one the finish kernels.  hp takes one of three routes:
//   nw1 = 1           the column gather writes hp_loc itself, which has the layout of the rows of the one window of s1 (We1 = n1);
//   nw2 = 1, nw1 > 1  the finished rows are the tile's hp blocks (0.0 + x is x): the row gather reads them in place;
//   both above 1      the column gather into the row buffer, behind the last column tile of a row block the row gather from it.
// A band side needs each of its windows in one tile only, in increasing order: the other side has at most one window.
int local_walk(rh_ctx* c, const LocalWalk& w)
{
    int rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const LocalPlan &P1 = w.D.P1, &P2 = w.D.P2;
    const LocalPlan& PB = w.band == 2 ? P2 : P1;   // of the band side
    assert(w.band == 0 || (w.band == 1 ? P2.nw : P1.nw) <= 1);
    LocalHp* out = w.out;
    if (w.band) c->loc_valid = c->loc_hp.valid = false;   // (the hp result of rh_local_duplex goes with the band it came with)
    if (out) out->valid = false;
    const int max_w = c->max_w;
    const bool two_level = P1.nw > 1 && P2.nw > 1;
    const size_t pitch = (size_t)P2.n + 1, rows_stride = ((size_t)P1.We + 1) * pitch;   // of hp_loc; of the row buffer of one k
    if (w.band && (rc = ensure(c, c->d_loc_bp, sizeof(double) * local_band_size(PB), false))) return rc;
    if (w.band && (rc = ensure(c, c->d_loc_up, sizeof(double) * local_up_size(PB, max_w), false))) return rc;
    if (w.band && (rc = ensure(c, c->d_loc_logz, sizeof(double) * PB.nw, false))) return rc;
    if (out && (rc = ensure(c, out->hp, sizeof(double) * local_hp2_size(w.D), false))) return rc;
    if (two_level && (rc = ensure(c, c->d_loc_rows, sizeof(double) * local_hp2_rowbuf_size(w.D, w.rows), false))) return rc;
    if (out && (rc = ensure(c, out->logz, sizeof(double) * local_hp2_logz_size(w.D), false))) return rc;
    EventPair ev;
    HIP_TRY(c, ev.create());
    std::vector<const char*> seqs((size_t)w.rows + w.cols);
    std::vector<int> lens((size_t)w.rows + w.cols), first((size_t)w.rows * w.cols), second((size_t)w.rows * w.cols);
    double ms_compute = 0.0, ms_acc = 0.0;
    float t = 0.f;
    LocalTile tile;
    for (size_t ti = 0; local_tile_at(w.D, w.rows, w.cols, ti, &tile); ti++) {
        const int kA = tile.kA, kB = tile.kB, lA = tile.lA, lB = tile.lB, nr = kB - kA, nc = lB - lA;
        const int q1 = w.front == 1 ? 0 : nc, q2 = w.front == 1 ? nr : 0;   // the first sequence of either side
        for (int a = 0; a < nr; a++) { seqs[q1 + a] = w.s1 + local_start(P1, kA + a); lens[q1 + a] = P1.We; }
        for (int b = 0; b < nc; b++) { seqs[q2 + b] = w.s2 + local_start(P2, lA + b); lens[q2 + b] = P2.We; }
        for (int a = 0; a < nr; a++)
            for (int b = 0; b < nc; b++) { first[(size_t)a * nc + b] = q1 + a; second[(size_t)a * nc + b] = q2 + b; }
        BatchRequest r;
        r.ns = nr + nc; r.seqs = seqs.data(); r.lens = lens.data();
        r.with_mc = true;
        if (out) { r.with_dx = true; r.npairs = nr * nc; r.first = first.data(); r.second = second.data(); }
        if ((rc = stage(c, r))) return rc;
        // One window pair (W >= n on both sides) is the pair itself, and the call answers with the bits of rh_duplex: under
        // RH_HYBRID_COFOLD that call has no folds to seed its two-molecule sweeps from, and seeded sweeps differ from it in the last
        // bits on the scaled linear kernels -- so this one compute runs them unseeded too.  Every other tile is seeded, like any batch.
        const int seed = c->co_seed;
        if (P1.nw == 1 && P2.nw == 1) c->co_seed = 0;
        rc = compute(c);
        c->co_seed = seed;
        if (rc) return rc;
        ms_compute += c->ms[3];
        const bool last = kB == P1.nw && lB == P2.nw;
        HIP_TRY(c, hipEventRecord(ev.a, c->s_mc));
        if (w.band) {
            const int q = w.band == 1 ? q1 : q2;
            LocalAcc A{};
            A.P = PB;
            A.tri_stride = c->mc.tri_stride; A.up_stride = (size_t)c->mc.ld * max_w;
            A.bp = c->d_bp.as<const double>() + q * A.tri_stride; A.up = c->d_up.as<const double>() + q * A.up_stride;
            A.acc_bp = c->d_loc_bp.as<double>(); A.acc_up = c->d_loc_up.as<double>();
            A.k0 = w.band == 1 ? kA : lA; A.k1 = w.band == 1 ? kB : lB; A.row0 = local_start(PB, A.k0); A.max_w = max_w;
            const int rows = local_start(PB, A.k1 - 1) + PB.We - A.row0;
            hipLaunchKernelGGL(local_accumulate, dim3(rows), dim3(kLocalThreads), 0, c->s_mc, A);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(c->d_loc_logz.as<double>() + A.k0, c->d_mclogz.as<const double>() + q, sizeof(double) * (A.k1 - A.k0), hipMemcpyDeviceToDevice, c->s_mc));
            if (last) {
                hipLaunchKernelGGL(local_finish, dim3(PB.n), dim3(kLocalThreads), 0, c->s_mc, PB, max_w, A.acc_bp, A.acc_up);
                HIP_TRY(c, hipGetLastError());
            }
        }
        if (out) {
            LocalHpGather G{};
            G.P1 = P1; G.P2 = P2;
            G.kA = kA; G.kB = kB; G.lA = lA; G.lB = lB;
            if (P1.nw == 1 || two_level) {
                G.src = c->d_hp.as<const double>(); G.src_stride = c->dx.tab_stride; G.src_pitch = c->dx.ldd;
                G.dst = two_level ? c->d_loc_rows.as<double>() : out->hp.as<double>(); G.dst_stride = rows_stride;
                const int nt = local_start(P2, lB - 1) + P2.We - local_start(P2, lA);
                hipLaunchKernelGGL(local_hp_col_gather, dim3((nt + kLocalThreads - 1) / kLocalThreads, std::min(nr * P1.We, kLocalGridRows)), dim3(kLocalThreads),
                                   0, c->s_mc, G);
                HIP_TRY(c, hipGetLastError());
            }
            HIP_TRY(c, hipMemcpy2DAsync(out->logz.as<double>() + (size_t)kA * P2.nw + lA, sizeof(double) * P2.nw, c->d_logz.p, sizeof(double) * nc,
                                        sizeof(double) * nc, nr, hipMemcpyDeviceToDevice, c->s_mc));
            if (P1.nw > 1 && lB == P2.nw) {
                G.src = two_level ? c->d_loc_rows.as<const double>() : c->d_hp.as<const double>();
                G.src_stride = two_level ? rows_stride : c->dx.tab_stride; G.src_pitch = two_level ? (int)pitch : c->dx.ldd;
                G.dst = out->hp.as<double>();
                const int ni = local_start(P1, kB - 1) + P1.We - local_start(P1, kA);
                hipLaunchKernelGGL(local_hp_row_gather, dim3((P2.n + kLocalThreads - 1) / kLocalThreads, std::min(ni, kLocalGridRows)), dim3(kLocalThreads), 0,
                                   c->s_mc, G);
                HIP_TRY(c, hipGetLastError());
            }
            if (last) {
                hipLaunchKernelGGL(local_hp2_finish, dim3((P2.n + 1 + kLocalThreads - 1) / kLocalThreads, std::min(P1.n + 1, kLocalGridRows)),
                                   dim3(kLocalThreads), 0, c->s_mc, P1, P2, out->hp.as<double>());
                HIP_TRY(c, hipGetLastError());
            }
        }
        HIP_TRY(c, hipEventRecord(ev.b, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));   // (the next tile's stage() reuses the tables this one read)
        HIP_TRY(c, hipEventElapsedTime(&t, ev.a, ev.b));
        ms_acc += t;
    }
    w.ms[0] = ms_compute; w.ms[1] = ms_acc;
    if (w.band) { c->loc = PB; c->loc_max_w = max_w; c->loc_valid = true; }
    if (out) { out->D = w.D; out->tile[0] = w.rows; out->tile[1] = w.cols; out->valid = true; }
    return RH_OK;
}

// the fetch of an hp result
int fetch_hp(rh_ctx* c, const LocalHp& R, double* hp, double* logz_pair)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (hp) HIP_TRY(c, hipMemcpyAsync(hp, R.hp.p, sizeof(double) * local_hp2_size(R.D), hipMemcpyDeviceToHost, c->s_mc));
    if (logz_pair) HIP_TRY(c, hipMemcpyAsync(logz_pair, R.logz.p, sizeof(double) * local_hp2_logz_size(R.D), hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
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

// the rows 1..n1 of an hp result as a scan
LocalScan hp_scan(const LocalHp& R, float threshold)
{
    const int hp_ld = R.D.P2.n + 1;
    return LocalScan{R.hp.as<const double>() + hp_ld, R.D.P1.n, hp_ld, hp_ld, 1, 0x3fffffff, kScanHp, threshold};
}

}  // namespace

int rh::host::local_scan_table(rh_ctx* c, const double* table, int n, int pitch, int what, float threshold, rh_cand* out, int cap, double* ms, const char* who)
{
    const LocalScan V = what == 0 ? LocalScan{table, n, pitch, pitch, 1, n - 1, kScanBp, threshold}
                                  : LocalScan{table, n, pitch, pitch, 0, n - 1 + pitch, kScanUp, threshold};
    return scan_candidates(c, V, out, cap, ms, who);
}

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
    LocalWalk w;
    std::string why;
    if (int rc = local_check(seq, n, window, step, &w.D.P1, &why)) return fail(c, rc, "%s", why.c_str());
    w.s1 = seq;
    w.rows = chunk_windows(c, w.D.P1, nullptr);
    w.band = 1;
    w.ms = c->loc_ms;
    return local_walk(c, w);
}

int rh_local_duplex(rh_ctx* c, const char* s1, int n1, const char* s2, int n2, int windowed, int window, int step)
{
    if (!c) return RH_ERR_ARG;
    LocalDuplexPlan D;
    std::string why;
    if (int rc = local_duplex_check(s1, n1, s2, n2, windowed, window, step, &D, &why)) return fail(c, rc, "%s", why.c_str());
    const int chunk = chunk_windows(c, D.P, &D);
    LocalWalk w;
    w.D = local_duplex_grid(D);
    w.s1 = s1; w.s2 = s2;
    w.rows = windowed == 1 ? chunk : 1; w.cols = windowed == 1 ? 1 : chunk;
    w.band = windowed;
    w.front = windowed == 1 ? 2 : 1;   // the query is sequence 0 of every chunk
    w.out = &c->loc_hp;
    w.ms = c->loc_ms;                  // band and hp kernels together
    if (int rc = local_walk(c, w)) return rc;
    c->loc_hp.windowed = windowed;
    return RH_OK;
}

int rh_local_hp_layout(rh_ctx* c, int* n1, int* n2, int* windowed, int* nw)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp_ready(c)) return rc;
    const LocalHp& R = c->loc_hp;
    if (n1) *n1 = R.D.P1.n;
    if (n2) *n2 = R.D.P2.n;
    if (windowed) *windowed = R.windowed;
    if (nw) *nw = R.windowed == 1 ? R.D.P1.nw : R.D.P2.nw;
    return RH_OK;
}

int rh_local_hp_results(rh_ctx* c, double* hp, double* logz_pair)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp_ready(c)) return rc;
    return fetch_hp(c, c->loc_hp, hp, logz_pair);
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
    if (what == 2) return scan_candidates(c, hp_scan(c->loc_hp, threshold), out, cap, &c->loc_ms[1], "rh_local_candidates");
    return local_scan_table(c, what == 0 ? c->d_loc_bp.as<const double>() : c->d_loc_up.as<const double>(), P.n, what == 0 ? P.ld : c->loc_max_w, what, threshold,
                            out, cap, &c->loc_ms[1], "rh_local_candidates");
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
    LocalWalk w;
    std::string why;
    if (int rc = local_duplex2_check(s1, n1, s2, n2, window1, step1, window2, step2, &w.D, &why)) return fail(c, rc, "%s", why.c_str());
    w.s1 = s1; w.s2 = s2;
    w.rows = c->loc2_tile[0]; w.cols = c->loc2_tile[1];
    if (w.rows <= 0 || w.cols <= 0) local_tile_auto(w.D, local_tables(c), &w.rows, &w.cols);
    w.rows = std::min(w.rows, w.D.P1.nw); w.cols = std::min(w.cols, w.D.P2.nw);
    w.out = &c->loc_hp2;
    w.ms = c->loc_hp2.ms;
    return local_walk(c, w);
}

int rh_local_hp2_layout(rh_ctx* c, int* n1, int* n2, int* nw1, int* nw2, int* starts1, int* starts2)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp2_ready(c)) return rc;
    const LocalPlan &P1 = c->loc_hp2.D.P1, &P2 = c->loc_hp2.D.P2;
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
    return fetch_hp(c, c->loc_hp2, hp, logz_pair);
}

int rh_local_hp2_candidates(rh_ctx* c, float threshold, rh_cand* out, int cap)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp2_ready(c)) return rc;
    if (cap < 0 || (cap > 0 && !out)) return fail(c, RH_ERR_ARG, "rh_local_hp2_candidates: bad cap");
    HIP_TRY(c, hipSetDevice(c->device));
    return scan_candidates(c, hp_scan(c->loc_hp2, threshold), out, cap, &c->loc_hp2.ms[1], "rh_local_hp2_candidates");
}

int rh_local_hp2_tile(rh_ctx* c, int* rows, int* cols)
{
    if (!c) return RH_ERR_ARG;
    if (int rc = local_hp2_ready(c)) return rc;
    if (rows) *rows = c->loc_hp2.tile[0];
    if (cols) *cols = c->loc_hp2.tile[1];
    return RH_OK;
}

int rh_local_hp2_times(rh_ctx* c, double ms[2])
{
    if (!c || !ms) return RH_ERR_ARG;
    if (int rc = local_hp2_ready(c)) return rc;
    ms[0] = c->loc_hp2.ms[0]; ms[1] = c->loc_hp2.ms[1];
    return RH_OK;
}

}  // extern "C"
