// allow_mask.hip -- the structure-constraint masks McBatch::allow of a whole batch, built where they are read.
//
// The host leaves three small values per letter (constraint_prepass.h: ch, P, enc); one launch writes every byte of the
// [ns][ld][ld] image from them, the zeros of row / column 0, of the lower triangle and of the padding up to ld included: it is
// the only writer of the buffer, so a shorter sequence, or a smaller batch after a larger one, finds nothing stale.
//
// A workgroup owns kAllowRows rows of one sequence, i.e. the bytes [lo, hi) of the flat image.  It stages the sequence's ch / P /
// enc in LDS once (they are indexed by row and by column), then writes the 16-byte-aligned part of [lo, hi) with one 16-byte
// store per lane and the few bytes in front of and behind it one by one: ld is even but no multiple of 16, so neither rows nor
// sequences start on a 16-byte boundary, and every byte is decoded to its own (row, column).
//
// An indexed batch gives the joint constraint of a pair as two shares, one per distinct sequence and role: joint_cons_gather (below)
// composes the three values per letter of every pair on the device, in the rows the host pass would have filled, and the same
// allow_mask_build writes the masks from them.
#include <hip/hip_runtime.h>

#include "constraint_prepass.h"
#include "kernels.h"

namespace rh {

using host::allow_pair;

__global__ __launch_bounds__(kAllowThreads) void allow_mask_build(uint8_t* __restrict__ allow, const int* __restrict__ n_of,
                                                                  const uint8_t* __restrict__ g_ch, const int* __restrict__ g_P,
                                                                  const int* __restrict__ g_enc, int ld, int lds, int in_lds)
{
    extern __shared__ int s_allow[];   // in_lds: P[lds], enc[lds], ch[lds]
    const int sq = blockIdx.x, tid = threadIdx.x;
    const int r0 = blockIdx.y * kAllowRows, r1 = min(r0 + kAllowRows, ld);
    const int n = n_of[sq];
    const int* P = g_P + (size_t)sq * lds;
    const int* enc = g_enc + (size_t)sq * lds;
    const uint8_t* ch = g_ch + (size_t)sq * lds;
    if (in_lds) {   // (a sequence too long for LDS is read from global memory through the same pointers)
        int* sP = s_allow;
        int* sE = s_allow + lds;
        uint8_t* sC = reinterpret_cast<uint8_t*>(s_allow + 2 * lds);
        for (int t = tid; t < lds; t += kAllowThreads) { sP[t] = P[t]; sE[t] = enc[t]; sC[t] = ch[t]; }
        __syncthreads();
        P = sP; enc = sE; ch = sC;
    }
    const size_t base = (size_t)sq * ld * ld;
    const size_t lo = base + (size_t)r0 * ld, hi = base + (size_t)r1 * ld;     // this tile's bytes of the flat image
    const size_t up = (lo + 15) & ~(size_t)15;
    const size_t vlo = up < hi ? up : hi, vhi = (hi & ~(size_t)15) > vlo ? (hi & ~(size_t)15) : vlo;   // its 16-byte-aligned part
    // the bytes in front of and behind the aligned part (fewer than 16 each)
    for (size_t f = lo + tid; f < vlo; f += kAllowThreads) {
        const unsigned off = (unsigned)(f - base);
        const int a = off / ld;
        allow[f] = allow_pair(a, (int)(off - a * ld), n, ch, P, enc) ? 1 : 0;
    }
    for (size_t f = vhi + tid; f < hi; f += kAllowThreads) {
        const unsigned off = (unsigned)(f - base);
        const int a = off / ld;
        allow[f] = allow_pair(a, (int)(off - a * ld), n, ch, P, enc) ? 1 : 0;
    }
    for (size_t f = vlo + 16 * (size_t)tid; f < vhi; f += 16 * (size_t)kAllowThreads) {
        const unsigned off = (unsigned)(f - base);
        int a = off / ld, b = (int)(off - a * ld);
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                v |= (allow_pair(a, b, n, ch, P, enc) ? 1u : 0u) << (8 * k);
                if (++b == ld) { b = 0; ++a; }   // (a == ld only behind the last byte of the image, where this chunk ends)
            }
            w[q] = v;
        }
        *reinterpret_cast<uint4*>(allow + f) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// The joint constraints of an indexed batch: one workgroup per pair writes the pair's row of ch / P / enc, every entry of 0 ..
// co_lds - 1 (the '.' / 0 / 0 of letter 0 and of the padding included: the buffer is reused across batches), from the two shares
// the index names; allow_mask_build then turns the rows into the masks as it does for rows that came from the host.  Each thread
// reads its own letter of one share once, consecutive threads consecutive letters, and at an open bracket one entry of the partner's
// short open list: nothing is read twice, so the shares are not staged in LDS, and shares of any length take this one path.
// The host has checked that both shares of every pair leave the same number of brackets open (joint_pair_check), which keeps the
// reads of the open lists inside them.
__global__ __launch_bounds__(kJointGatherThreads) void joint_cons_gather(JointShares S, uint8_t* __restrict__ ch, int* __restrict__ P,
                                                                         int* __restrict__ enc)
{
    const int p = blockIdx.x;
    const int a = S.idx[2 * p], b = S.ns + S.idx[2 * p + 1];   // the shares: sequence idx[2p] as s1, sequence idx[2p+1] as s2
    const int n = S.con[p], n1 = S.con[S.np + p];
    const int m = S.open_off[a + 1] - S.open_off[a];
    const host::ShareRef A{S.ch + (size_t)a * S.lds, S.P + (size_t)a * S.lds, S.enc + (size_t)a * S.lds, S.open_pos + S.open_off[a]};
    const host::ShareRef B{S.ch + (size_t)b * S.lds, S.P + (size_t)b * S.lds, S.enc + (size_t)b * S.lds, S.open_pos + S.open_off[b]};
    const size_t row = (size_t)p * S.co_lds;
    for (int j = threadIdx.x; j < S.co_lds; j += kJointGatherThreads)
        host::compose_joint_letter(j, n1, n - n1, m, A, B, &ch[row + j], &P[row + j], &enc[row + j]);
}

}  // namespace rh
