// pack_results.hip -- the dense results of a computed batch at the width the reference stores them (VF / VVF / pair_info::p are
// float, src/ractip.cpp:82-83): bp, up and hp are read from the padded double tables of the batch, narrowed by one correctly rounded
// conversion each ((float)x, v_cvt_f32_f64 in round-to-nearest with float subnormals kept) and written at their tight sizes into the
// packed image of packed_layout (batch.h).  A streaming kernel: no LDS, no atomics, the source tables are only read.
#include <hip/hip_runtime.h>

#include "batch.h"
#include "kernels.h"

namespace rh {

// One workgroup = one chunk of one block (a sequence's bp or up, a pair's hp).  A thread owns groups of four consecutive floats of the
// block: a block starts at a multiple of four floats of an image that starts 16-byte aligned, so every group is one aligned 16-byte
// store, and the last group of a block carries the block's padding (zeros), which makes the whole image deterministic.
//   bp, up: the block is contiguous in the source and starts 16-byte aligned there (tri_stride and the row pitch of up are even), so
//     a full group is two 16-byte loads.
//   hp: the row pitch changes from ldd to n2+1.  A group whose four floats lie in one source row from an even column on (ldd and
//     hp_stride are even) is two 16-byte loads as well; any other group loads its doubles one by one, walking over the row end.
// Bounds: a group index is below ceil(size / 4); element e of a group is loaded only when e < size, and then lies inside the block's
// source table (bp: e < tri_size(n) <= tri_stride; up: e < n*max_w <= up_stride; hp: row <= n1, col <= n2, row*ldd + col < hp_stride).
// Sizes and in-block indices are 32-bit (the host refuses a block of 2^31 elements or more); offsets between blocks are 64-bit.
__global__ __launch_bounds__(kPackThreads) void pack_results_f32(PackArgs A)
{
    const int nbp = A.bp ? A.nseq : 0, nup = A.up ? A.nseq : 0;
    int b = blockIdx.x;
    const double* __restrict__ src;
    float* __restrict__ dst;
    unsigned size, w = 0;   // w: columns of an hp row (0: the block is contiguous in the source)
    if (b < nbp) {
        src = A.bp + (size_t)b * A.tri_stride;
        dst = A.dst_bp + A.off[b];
        const unsigned n = A.n[b];
        size = (n + 1) * (n + 2) / 2;
    } else if ((b -= nbp) < nup) {
        src = A.up + (size_t)b * A.up_stride;
        dst = A.dst_up + A.off[A.nseq + 1 + b];
        size = (unsigned)A.n[b] * A.max_w;
    } else {
        b -= nup;
        src = A.hp + (size_t)b * A.hp_stride;
        dst = A.dst_hp + A.off[2 * (A.nseq + 1) + b];
        w = A.pn[2 * b + 1] + 1;
        size = (unsigned)(A.pn[2 * b] + 1) * w;
    }
    const unsigned groups = (size + 3) / 4, ldd = A.ldd;
    for (unsigned g = blockIdx.y * kPackThreads + threadIdx.x; g < groups; g += gridDim.y * kPackThreads) {
        const unsigned e = 4 * g;
        const bool full = e + 4 <= size;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        unsigned row = 0, col = e;
        if (w) { row = e / w; col = e - row * w; }
        const double* __restrict__ s = src + (size_t)row * ldd + col;
        if (full && (w == 0 || (col + 4 <= w && (col & 1) == 0))) {
            const double2 lo = reinterpret_cast<const double2*>(s)[0], hi = reinterpret_cast<const double2*>(s)[1];
            v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
        } else if (w == 0) {
            for (unsigned k = 0; k < 4; k++) if (e + k < size) v[k] = s[k];
        } else {
            for (unsigned k = 0; k < 4; k++) {
                if (e + k < size) v[k] = src[(size_t)row * ldd + col];
                if (++col == w) { col = 0; row++; }
            }
        }
        *reinterpret_cast<float4*>(dst + e) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    }
}

}  // namespace rh
