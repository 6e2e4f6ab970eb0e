// pair_index.hip -- pairs by index: every distinct sequence of an upload is encoded, copied to HBM and folded once, and pair p is
// (sequence idx[2p], sequence idx[2p+1]).  The duplex families (dxl_*, dx_*, dxvl_*, dxv_*) address pair p's letters as rows 2p and
// 2p+1 of DxBatch::seq / DxBatch::n; these kernels build that pair-major image on the device from the distinct sequences, so the sweep
// kernels are the same for rh_batch_upload (the identity index) and rh_batch_upload_indexed, and nothing is copied from the host per
// pair.  Copy kernels: what matters is that a workgroup reads and writes consecutive bytes, and that the grid has a workgroup per row.
#include <hip/hip_runtime.h>

#include "batch.h"
#include "kernels.h"

namespace rh {

// One workgroup per (pair, side).  The row of lds bytes (a multiple of 16, rows 16-byte aligned: the buffers come from hipMalloc)
// goes over in 16-byte loads and stores, sentinels included.  For the two-molecule ensemble the same workgroup writes its strand's
// part of the joint row: side 0 the bytes 0..n1 (the "no nucleotide" code 0, then s1), side 1 the bytes n1+1..co_lds-1 (s2, then
// code 0 to the end of the row) and the pair's joint length and cut -- every byte of the joint image exactly once.
__global__ __launch_bounds__(kPairGatherThreads) void pair_gather(PairImage G)
{
    const int p = blockIdx.x, side = blockIdx.y, row = 2 * p + side;
    const int sq = G.idx[row];
    const uint8_t* __restrict__ src = G.seq + (size_t)sq * G.lds;
    const uint4* __restrict__ src16 = reinterpret_cast<const uint4*>(src);
    uint4* __restrict__ dst16 = reinterpret_cast<uint4*>(G.pseq + (size_t)row * G.lds);
    for (int k = threadIdx.x; k < G.lds / 16; k += kPairGatherThreads) dst16[k] = src16[k];
    if (threadIdx.x == 0) G.pn[row] = G.n[sq];
    if (!G.coseq) return;
    const int n1 = G.n[G.idx[2 * p]], n2 = G.n[G.idx[2 * p + 1]];
    uint8_t* __restrict__ joint = G.coseq + (size_t)p * G.co_lds;
    if (side == 0) {
        for (int i = threadIdx.x; i <= n1; i += kPairGatherThreads) joint[i] = i ? src[i] : 0;
    } else {
        for (int i = n1 + 1 + threadIdx.x; i < G.co_lds; i += kPairGatherThreads) joint[i] = i <= n1 + n2 ? src[i - n1] : 0;
        if (threadIdx.x == 0) { G.con[p] = n1 + n2; G.con[G.np + p] = n1; }
    }
}

// two-molecule batch B (pair p = s1+s2, cut after s1) next to the single-molecule batch S of the same upload (sequences idx[2p],
// idx[2p+1]), both in scaled linear space with the same lam: a cell whose letters all lie on one strand has the value it has in that
// molecule folded alone -- the same recurrences over the same letters, and at a strand end the neighbour letter is "none" in
// both (FCX differs at the strand ends, where it looks across the gap, but only loops whose side crosses the gap read it there,
// and those are excluded).  One launch copies four inside tables of both triangles: FCA, FM1, FMS and FM, the multiloop and exterior
// pieces a cell with letters on both strands is built from.  FC, FCX and FCB of a one-strand cell are never used by such a cell: the
// inner pair of its interior loops, bulges and stacks has letters on both strands too (each side of the loop stays on its strand:
// the per-lane limits l1max / l2max, and the strand mask of the staged rows), and every operand that might be one of them is
// discarded by a select, never by a multiplication with 0.  Through the index, N + M folds seed N x M two-molecule sweeps.
__global__ __launch_bounds__(256) void vlin_co_seed(McBatch B, McBatch S, const int* __restrict__ idx)
{
    const int p = blockIdx.y, d = blockIdx.x;
    const int n = B.n[p], n1 = B.cut[p];
    constexpr int NT = 4;
    const int tabs[NT] = {VL_FCA, VL_FM1, VL_FMS, VL_FM};
    double* __restrict__ dst = B.tab + (size_t)p * B.seq_stride + (size_t)d * B.ld;
    for (int strand = 0; strand < 2; strand++) {
        const int cells = (strand ? n - n1 : n1) - 1 - d, off = strand ? n1 : 0;
        if (cells < 1) continue;
        const double* __restrict__ src = S.tab + (size_t)idx[2 * p + strand] * S.seq_stride + (size_t)d * S.ld;
        for (int t = 0; t < NT; t++)
            for (int i = 1 + threadIdx.x; i <= cells; i += 256) dst[tabs[t] * B.tab_stride + off + i] = src[tabs[t] * S.tab_stride + i];
    }
}

}  // namespace rh
