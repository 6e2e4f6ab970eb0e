// candidates.hip -- threshold scans of the result matrices on the device (rh_batch_candidates, rh_batch_candidates_all).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "kernels.h"

// ---- ordered threshold compaction (the scans of the reference's src/ractip.cpp:557-568, 578-589,
//      598-608, 621-627 done on device): one wavefront per matrix row; probabilities are narrowed
//      to float BEFORE the comparison, as the reference's VF containers do (src/ractip.cpp:82-83).
struct CandView {
    const double* base;
    int kind;   // 0 = bp triangle (row i: j = i+1..n), 1 = hp matrix (row i: j = 1..n2), 2 = up vector
    int n, n2, ld;
};
struct RowSpan {
    const double* p;  // row base: element j of the row is p[j]
    int i, j0, j1;
    bool ok;
};
// kind 2 (up): n2 = max_w, the row is the whole n x max_w matrix, entry j = position*max_w + width index
__device__ __forceinline__ RowSpan cand_row(const double* base, int kind, int n, int n2, int ld, int row)
{
    RowSpan r;
    if (kind == 0) {
        r.i = row + 1; r.j0 = r.i + 1; r.j1 = n;
        r.p = base + (size_t)r.i * (size_t)(2 * (n + 1) - r.i - 1) / 2;
        r.ok = r.i <= n;
    } else if (kind == 1) {
        r.i = row + 1; r.j0 = 1; r.j1 = n2;
        r.p = base + (size_t)r.i * (size_t)ld;
        r.ok = r.i <= n;
    } else {
        r.i = 0; r.j0 = 0; r.j1 = n * n2 - 1; r.p = base;
        r.ok = row == 0;
    }
    return r;
}
__global__ __launch_bounds__(256) void cand_count(const double* __restrict__ base, int kind, int n, int n2, int ld, float th,
                                                  int nrows, int* __restrict__ counts)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= nrows) return;
    const RowSpan r = cand_row(base, kind, n, n2, ld, row);
    if (!r.ok) return;
    int c = 0;
    for (int j = r.j0 + lane; j <= r.j1; j += 64) c += ((float)r.p[j] > th) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) counts[row] = c;
}
__global__ __launch_bounds__(256) void cand_write(const double* __restrict__ base, int kind, int n, int n2, int ld, float th,
                                                  int nrows, const int* __restrict__ counts, const int* __restrict__ offsets,
                                                  rh_cand* __restrict__ out, int cap)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= nrows) return;
    if (counts[row] == 0) return;   // the count pass found nothing in this row: leave it unread
    const RowSpan r = cand_row(base, kind, n, n2, ld, row);
    if (!r.ok) return;
    int pos = offsets[row];
    for (int jb = r.j0; jb <= r.j1; jb += 64) {
        const int j = jb + lane;
        const float pf = j <= r.j1 ? (float)r.p[j] : 0.0f;
        const bool hit = j <= r.j1 && pf > th;
        const unsigned long long m = __ballot(hit);
        if (hit) {
            const int k = pos + __popcll(m & ((1ull << lane) - 1ull));
            if (k < cap) {
                rh_cand e;
                e.i = kind == 2 ? j / n2 : r.i;
                e.j = kind == 2 ? j % n2 : j;
                e.p = pf;
                out[k] = e;
            }
        }
        pos += __popcll(m);
    }
}

// ---- the same compaction for every problem of the batch at once: row index = p*rmax + r.  bp and up rows (which = 0, 1, 3, 4)
// belong to the fold batch: problem p scans sequence idx[per p + side] (per = 2: pair p's s1 / s2 through the index of the upload;
// per = 1, idx = nullptr: sequence p itself, the per-sequence form) with the lengths nn of the fold batch.  hp (which = 2) is per
// pair, and nn the pair-major lengths [2 np] of the duplex batch.
__device__ __forceinline__ RowSpan cand_row_all(const double* bp, const double* hp, const double* up, const int* __restrict__ nn,
                                                const int* __restrict__ idx, int per, size_t tri_stride, size_t hp_stride, int up_ld,
                                                int hp_ld, int which, int p, int r)
{
    if (which == 2) return cand_row(hp + (size_t)p * hp_stride, 1, nn[2 * p], nn[2 * p + 1], hp_ld, r);
    const int slot = per * p + (per == 2 ? (which <= 1 ? which : which - 3) : 0);
    const int sq = idx ? idx[slot] : slot;
    if (which <= 1) return cand_row(bp + (size_t)sq * tri_stride, 0, nn[sq], 0, 0, r);
    return cand_row(up + (size_t)sq * up_ld, 2, nn[sq], hp_ld /* = max_w for the up scans */, 0, r);
}
__global__ __launch_bounds__(256) void cand_count_all(const double* __restrict__ bp, const double* __restrict__ hp, const double* __restrict__ up,
                                                      const int* __restrict__ nn, const int* __restrict__ idx, int per, size_t tri_stride, size_t hp_stride,
                                                      int up_ld, int hp_ld, int which, int rmax, float th, int* __restrict__ counts)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, p = blockIdx.y;
    if (r >= rmax) return;
    const RowSpan rs = cand_row_all(bp, hp, up, nn, idx, per, tri_stride, hp_stride, up_ld, hp_ld, which, p, r);
    int c = 0;
    if (rs.ok)
        for (int j = rs.j0 + lane; j <= rs.j1; j += 64) c += ((float)rs.p[j] > th) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) counts[(size_t)p * rmax + r] = c;
}
__global__ __launch_bounds__(256) void cand_write_all(const double* __restrict__ bp, const double* __restrict__ hp, const double* __restrict__ up,
                                                      const int* __restrict__ nn, const int* __restrict__ idx, int per, size_t tri_stride, size_t hp_stride,
                                                      int up_ld, int hp_ld, int which, int rmax, float th, const int* __restrict__ counts,
                                                      const int* __restrict__ offsets, rh_cand* __restrict__ out, int cap)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, p = blockIdx.y;
    if (r >= rmax) return;
    if (counts[(size_t)p * rmax + r] == 0) return;   // the count pass found nothing in this row: leave it unread
    const RowSpan rs = cand_row_all(bp, hp, up, nn, idx, per, tri_stride, hp_stride, up_ld, hp_ld, which, p, r);
    if (!rs.ok) return;
    int pos = offsets[(size_t)p * rmax + r];
    for (int jb = rs.j0; jb <= rs.j1; jb += 64) {
        const int j = jb + lane;
        const float pf = j <= rs.j1 ? (float)rs.p[j] : 0.0f;
        const bool hit = j <= rs.j1 && pf > th;
        const unsigned long long m = __ballot(hit);
        if (hit) {
            const int k = pos + __popcll(m & ((1ull << lane) - 1ull));
            if (k < cap) {
                rh_cand e;
                e.i = which >= 3 ? j / hp_ld : rs.i;
                e.j = which >= 3 ? j % hp_ld : j;
                e.p = pf;
                out[k] = e;
            }
        }
        pos += __popcll(m);
    }
}

using namespace rh::host;

extern "C" {

int rh_batch_candidates(rh_ctx* c, int p, int which, float threshold, rh_cand* out, int cap)
{
    if (!c) return RH_ERR_ARG;
    if (!c->computed) return fail(c, RH_ERR_ARG, "no computed batch");
    if (p < 0 || p >= c->np || which < 0 || which > 4 || cap < 0 || (cap > 0 && !out)) return fail(c, RH_ERR_ARG, "bad pair/which/cap");
    HIP_TRY(c, hipSetDevice(c->device));
    CandView v{};
    int nrows;
    if (which <= 1) {
        const int sq = seq_of(c, p, which);
        v = CandView{c->d_bp.as<const double>() + (size_t)sq * c->mc.tri_stride, 0, c->n[sq], 0, 0};
        nrows = c->n[sq];
    } else if (which == 2) {
        v = CandView{c->d_hp.as<const double>() + (size_t)p * c->dx.tab_stride, 1, c->n[seq_of(c, p, 0)], c->n[seq_of(c, p, 1)], c->dx.ldd};
        nrows = c->n[seq_of(c, p, 0)];
    } else {
        const int sq = seq_of(c, p, which - 3);
        v = CandView{c->d_up.as<const double>() + (size_t)sq * c->mc.ld * c->max_w, 2, c->n[sq], c->max_w, 0};
        nrows = 1;
    }
    int rc;
    if ((rc = ensure(c, c->d_cnt, sizeof(int) * 2 * (size_t)(nrows + 1), false))) return rc;
    int* d_counts = c->d_cnt.as<int>();
    int* d_offsets = d_counts + (nrows + 1);
    hipLaunchKernelGGL(cand_count, dim3((nrows + 3) / 4), dim3(256), 0, c->s_mc, v.base, v.kind, v.n, v.n2, v.ld, threshold, nrows, d_counts);
    std::vector<int> counts(nrows), offsets(nrows);
    HIP_TRY(c, hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * nrows, hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    int found = 0;
    for (int r = 0; r < nrows; r++) { offsets[r] = found; found += counts[r]; }
    const int take = std::min(found, cap);
    if (take > 0) {
        if ((rc = ensure(c, c->d_cand, sizeof(rh_cand) * (size_t)take, false))) return rc;
        HIP_TRY(c, hipMemcpyAsync(d_offsets, offsets.data(), sizeof(int) * nrows, hipMemcpyHostToDevice, c->s_mc));
        hipLaunchKernelGGL(cand_write, dim3((nrows + 3) / 4), dim3(256), 0, c->s_mc, v.base, v.kind, v.n, v.n2, v.ld, threshold,
                           nrows, d_counts, d_offsets, c->d_cand.as<rh_cand>(), take);
        HIP_TRY(c, hipMemcpyAsync(out, c->d_cand.p, sizeof(rh_cand) * (size_t)take, hipMemcpyDeviceToHost, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    }
    return found;
}

// the scan of every problem of the batch: per = 2 the np pairs (bp and up through the index of the upload), per = 1 the ns sequences
static int candidates_all(rh_ctx* c, int per, int which, float threshold, rh_cand* out, int cap, int* first)
{
    if (!c->computed || !c->has_mc || !c->has_dx) return fail(c, RH_ERR_ARG, "no computed pair batch");
    if (which < 0 || which > 4 || cap < 0 || (cap > 0 && !out) || !first) return fail(c, RH_ERR_ARG, "bad which/cap/first");
    HIP_TRY(c, hipSetDevice(c->device));
    const int np = per == 2 ? c->np : c->ns;
    const int rmax = which >= 3 ? 1 : (which == 2 ? c->dx.n1max : c->mc.nmax);
    const size_t nrows = (size_t)np * rmax;
    const int* nn = which == 2 ? c->dx.n : c->d_n.as<const int>();
    const int* idx = per == 2 ? c->d_pidx.as<const int>() : nullptr;
    int rc;
    if ((rc = ensure(c, c->d_cnt, sizeof(int) * 2 * (nrows + 1), false))) return rc;
    int* d_counts = c->d_cnt.as<int>();
    int* d_offsets = d_counts + (nrows + 1);
    const dim3 grid((rmax + 3) / 4, np);
    hipLaunchKernelGGL(cand_count_all, grid, dim3(256), 0, c->s_mc, c->d_bp.as<const double>(), c->d_hp.as<const double>(), c->d_up.as<const double>(),
                       nn, idx, per, c->mc.tri_stride, c->dx.tab_stride, c->mc.ld * c->max_w, which >= 3 ? c->max_w : c->dx.ldd, which, rmax, threshold, d_counts);
    std::vector<int> counts(nrows), offsets(nrows);
    HIP_TRY(c, hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * nrows, hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    int found = 0;
    for (int p = 0; p < np; p++) {
        first[p] = found;
        for (int r = 0; r < rmax; r++) { offsets[(size_t)p * rmax + r] = found; found += counts[(size_t)p * rmax + r]; }
    }
    first[np] = found;
    const int take = std::min(found, cap);
    if (take > 0) {
        if ((rc = ensure(c, c->d_cand, sizeof(rh_cand) * (size_t)take, false))) return rc;
        HIP_TRY(c, hipMemcpyAsync(d_offsets, offsets.data(), sizeof(int) * nrows, hipMemcpyHostToDevice, c->s_mc));
        hipLaunchKernelGGL(cand_write_all, grid, dim3(256), 0, c->s_mc, c->d_bp.as<const double>(), c->d_hp.as<const double>(), c->d_up.as<const double>(),
                           nn, idx, per, c->mc.tri_stride, c->dx.tab_stride, c->mc.ld * c->max_w, which >= 3 ? c->max_w : c->dx.ldd, which, rmax, threshold, d_counts, d_offsets,
                           c->d_cand.as<rh_cand>(), take);
        HIP_TRY(c, hipMemcpyAsync(out, c->d_cand.p, sizeof(rh_cand) * (size_t)take, hipMemcpyDeviceToHost, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    }
    return found;
}

int rh_batch_candidates_all(rh_ctx* c, int which, float threshold, rh_cand* out, int cap, int* first)
{
    if (!c) return RH_ERR_ARG;
    return candidates_all(c, 2, which, threshold, out, cap, first);
}

int rh_batch_candidates_seq_all(rh_ctx* c, int what, float threshold, rh_cand* out, int cap, int* first_out)
{
    if (!c) return RH_ERR_ARG;
    if (what != 0 && what != 1) return fail(c, RH_ERR_ARG, "rh_batch_candidates_seq_all: what = %d", what);
    return candidates_all(c, 1, what == 0 ? 0 : 3, threshold, out, cap, first_out);
}

}  // extern "C"
