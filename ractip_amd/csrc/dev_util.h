// dev_util.h -- the small device helpers that more than one kernel file uses.  Everything here is inlined into the kernel that calls
// it (the library is built without relocatable device code), so sharing the text changes no kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace rh {

namespace {

// AU, CG, GU both ways (InferenceEngine.ipp:391-396); code 4 (unknown letter) never pairs
constexpr uint32_t kPairMask = (1u << (0 * 5 + 3)) | (1u << (3 * 5 + 0)) | (1u << (1 * 5 + 2)) |
                               (1u << (2 * 5 + 1)) | (1u << (2 * 5 + 3)) | (1u << (3 * 5 + 2));
__device__ __forceinline__ bool pairs(int a, int b) { return (kPairMask >> (a * 5 + b)) & 1u; }
// row i of the posterior triangle (McBatch::bp, the reference's triangular layout)
__device__ __forceinline__ size_t tri_off(int n, int i) { return (size_t)i * (size_t)(2 * (n + 1) - i - 1) / 2; }

__device__ __forceinline__ double wsum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Work distribution of the sweeps.  A launch covers every sequence of the batch; `pin` selects the block->(sequence, slot) map:
//   pin = 1: blockIdx.x = sequence (fastest varying).  Workgroups are dealt round-robin over the 8 XCDs by linear id, so with
//            ns % 8 == 0 all blocks of a sequence share one XCD and its 4 MiB L2 sees only ns/8 sequences' rows (speed only).
//   pin = 0: blockIdx.y = sequence: few, large sequences are spread over all XCDs.
__device__ __forceinline__ void block_map(int pin, int* sq, int* slot)
{
    *sq = pin ? blockIdx.x : blockIdx.y;
    *slot = pin ? blockIdx.y : blockIdx.x;
}

// workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the wavefront's outstanding GLOBAL stores and
// loads (s_waitcnt vmcnt(0)): inside a chain of diagonals that would expose one HBM round trip per diagonal.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// volatile LDS pointer: keeps every read a plain ds_read_b64 (256 B/clk/CU); merged into ds_read2_b64 two reads cost 8 cycles on CDNA4
typedef const volatile __attribute__((address_space(3))) double* lds_vp;

// (T+1)-tap filter over an LDS-resident row segment, fully unrolled: the weights are consecutive and
// wave-uniform (wide scalar loads), every tap is one ds_read + one FMA and there is no loop control on the
// scalar unit (a rolled loop costs ~5 SALU instructions per tap and the CU has ONE scalar ALU: measured
// 2.4 SALU per VALU instruction before unrolling).
template <int T>
__device__ __forceinline__ double filt_fwd(const double* __restrict__ wt, const double* seg)
{   // sum_l1 wt[l1] * seg[l1]
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int l1 = 0; l1 <= T; l1 += 2) {
        s0 = fma(wt[l1], seg[l1], s0);
        if (l1 + 1 <= T) s1 = fma(wt[l1 + 1], seg[l1 + 1], s1);
    }
    return s0 + s1;
}
template <int T>
__device__ __forceinline__ double filt_rev(const double* __restrict__ wt, const double* seg)
{   // sum_l1 wt[l1] * seg[T-l1]
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int l1 = 0; l1 <= T; l1 += 2) {
        s0 = fma(wt[l1], seg[T - l1], s0);
        if (l1 + 1 <= T) s1 = fma(wt[l1 + 1], seg[T - l1 - 1], s1);
    }
    return s0 + s1;
}
// the filter lengths that every `*_any` dispatcher has a case for (the CONTRAfold shapes add 0..3, the look-ahead pairs 31)
#define RH_T_CASES_4_30(X) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
    X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30)

}  // namespace

}  // namespace rh
