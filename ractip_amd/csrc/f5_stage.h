// f5_stage.h -- index maps of the exterior-sum passes (lin_f5i_pass / lin_f5o_pass, mccaskill_strip.hip): which FCA cells a block of
// kF5Blk entries needs, how 256 threads fetch them as row segments (16 lanes per table row: one or two 128-byte lines per 16 lanes),
// where they stand in the LDS chunk buffer, and which thread sums which of them.  Plain integer functions for host and device:
// the kernels use them, tools/f5_stage_check.cpp runs both passes through them on the CPU, f5_pass_lds (launch_contrafold.hip) sizes
// the dynamic LDS from them.
//
// A block's operands are the cells (table row, entry e) of a band of rows: every row contributes kF5Blk consecutive columns,
//   F5o, entries k0-e:   row r = term r,           column k0+1-e       (exists for e < ne and k0-e+2+r <= n)
//   F5i, entries jj0+e:  row d, term k = jj0+e-2-d, column jj0-1-d+e    (exists for e < ne and k >= 0)
// and the band goes through LDS in chunks of at most R rows, F5o from row 0 up, F5i from the top row down (ascending k for every
// entry, the order of the sums).  Thread t fetches entry t%16 of the chunk rows t/16 + 16 i into slot row*kF5StageStride + entry; an
// element that does not exist fetches the cell (0, 1) instead and its slot is never summed.  The term of a row is summed by thread
// (term mod 256), as in the serial kernels; a chunk has at most 256 rows, so it holds at most one term per thread and entry.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define RH_F5_HD __host__ __device__ inline
#else
#define RH_F5_HD inline
#endif

namespace rh {

constexpr int kF5Blk = 16;            // entries per block = columns per row segment
constexpr int kF5Threads = 256;       // threads per workgroup = the fixed partition of every sum
constexpr int kF5StageRows = 128;     // R unless the F5 vector and the parked operands leave less (tests/test_gpu_f5_staged.py: STAGE_ROWS)
constexpr int kF5StageRowsMin = 32;   // batches whose ld leaves fewer rows keep the serial kernels (ld above about 4300)
constexpr int kF5StageStride = 17;   // doubles per staged row: 16-lane segment writes and stride-17 reads of 32 lanes are conflict-free
constexpr int kF5StageLoads = kF5StageRows * kF5Blk / kF5Threads;   // staging elements per thread and chunk
constexpr int kF5ParkT = 14;          // F5o: threads 0..13 sum entry e >= 2 + t inside the chain, from parked operands
constexpr int kF5LdsDoubles = 64 * 1024 / 8;

// F5o: parked operand of term t + 256 q (t <= e-2) of entry e
RH_F5_HD int f5_park_slot(int q, int e, int t) { return (q * kF5ParkT + (e - 2)) * kF5ParkT + t; }
// dynamic LDS in doubles ahead of the chunk buffer: F5[ld], partial sums [2][4], F5o also the parked operands
RH_F5_HD int f5_fixed_doubles(int ld, int phase) { return ld + 8 + (phase ? (ld + 255) / 256 * kF5ParkT * kF5ParkT : 0); }
// rows per chunk at this ld: what 64 KB leave, in whole workgroup instructions (256 threads x 16 lanes per row = 16 rows), at most
// kF5StageRows
RH_F5_HD int f5_stage_rows(int ld, int phase)
{
    const int room = (kF5LdsDoubles - f5_fixed_doubles(ld, phase)) / kF5StageStride;
    return room >= kF5StageRows ? kF5StageRows : room < 0 ? 0 : room & ~(kF5Threads / kF5Blk - 1);
}
RH_F5_HD int f5_lds_doubles(int ld, int phase) { return f5_fixed_doubles(ld, phase) + f5_stage_rows(ld, phase) * kF5StageStride; }

// chunks of a band of rows 0 .. top (top < 0: none)
RH_F5_HD int f5_chunks(int top, int R) { return top < 0 ? 0 : top / R + 1; }
struct F5Chunk { int lo, hi; };   // rows lo .. hi
RH_F5_HD F5Chunk f5o_chunk(int top, int R, int c) { return F5Chunk{c * R, c * R + R - 1 < top ? c * R + R - 1 : top}; }
RH_F5_HD F5Chunk f5i_chunk(int top, int R, int c) { return f5o_chunk(top, R, f5_chunks(top, R) - 1 - c); }   // the same chunks, from the top

// staging element i (< kF5StageLoads) of thread t: entry t%16 of chunk row t/16 + 16 i
RH_F5_HD int f5_stage_row(int t, int i) { return (t >> 4) + (kF5Threads / kF5Blk) * i; }
RH_F5_HD int f5_stage_entry(int t) { return t & (kF5Blk - 1); }
RH_F5_HD int f5_stage_slot(int row_in_chunk, int e) { return row_in_chunk * kF5StageStride + e; }

// F5o, block k0 (entries k0-e, e < ne) of a sequence of n letters: the operand of term r of entry e exists for rows 0 .. f5o_last_row
RH_F5_HD int f5o_last_row(int n, int k0, int ne, int e) { return e < ne ? n - 2 - k0 + e : -1; }
RH_F5_HD size_t f5o_addr(int ld, int k0, int r, int e) { return (size_t)r * ld + (k0 + 1 - e); }
// the one row >= lo within 256 whose term thread t owns
RH_F5_HD int f5o_owned_row(int lo, int t) { return lo + ((t - lo) & (kF5Threads - 1)); }

// F5i, block jj0 (entries jj0+e, e < ne): row d holds the operand of term jj0+e-2-d of entry e, for rows 0 .. f5i_last_row
RH_F5_HD int f5i_term(int jj0, int d, int e) { return jj0 + e - 2 - d; }
RH_F5_HD int f5i_last_row(int jj0, int ne, int e) { return e < ne ? jj0 + e - 2 : -1; }
RH_F5_HD size_t f5i_addr(int ld, int jj0, int d, int e) { return (size_t)d * ld + (jj0 - 1 - d + e); }
// the one term >= the term of row hi within 256 that thread t owns for entry e (it may be negative or beyond row lo: no term then)
RH_F5_HD int f5i_owned_term(int jj0, int hi, int e, int t)
{
    const int klo = f5i_term(jj0, hi, e);
    return klo + ((t - klo) & (kF5Threads - 1));
}

}  // namespace rh
