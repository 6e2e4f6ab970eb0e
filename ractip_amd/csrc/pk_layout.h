// pk_layout.h -- the order of the 256 doubles of a packed operand tile of the block products (mccaskill_far.hip), as index maps that
// compile for the host and the device: lin_pack_tiles writes through them, pk_loop / far2_loop / the wave kernels read through them,
// and tools/pk_layout_check.cpp checks them on the CPU.
//
// A tile is two halves of 128 doubles (1 KiB each).  An MFMA operand fragment is four registers s = 0..3 per lane l = 0..63;
// register s of lane l sits at (s >> 1) * 128 + 2 * l + (s & 1).  A wavefront therefore reads a fragment with two 16-byte loads per
// lane, half h at byte 1024 h + 16 l: each instruction covers 1 KiB contiguous, eight whole 128-byte lines, and no line is
// requested by both.  What the registers mean, for a 16x16 tile T:
//   layout LA: register s of lane l = T[l & 15][4 s + (l >> 4)]   (the A operand of v_mfma_f64_16x16x4_f64, K step s)
//   layout LB: register s of lane l = T[4 s + (l >> 4)][l & 15]   (the B operand) -- LB of a tile is LA of its transpose
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PK_HD __host__ __device__
#else
#define PK_HD
#endif

namespace rh {

constexpr int kPkTile = 256;   // doubles per packed tile
constexpr int kPkHalf = 128;   // doubles per half = per load instruction of a wavefront

// register s of lane l -> index within the tile
PK_HD constexpr int pk_reg_index(int l, int s) { return (s >> 1) * kPkHalf + 2 * l + (s & 1); }
// what a reader adds to the tile's address for its load of half h (two doubles: registers 2h and 2h + 1)
PK_HD constexpr int pk_half_offset(int l, int h) { return h * kPkHalf + 2 * l; }
// element (u, v) of the tile -> index, in the two layouts
PK_HD constexpr int pk_la_index(int u, int v) { return pk_reg_index(u + 16 * (v & 3), v >> 2); }
PK_HD constexpr int pk_lb_index(int u, int v) { return pk_la_index(v, u); }

// The pack kernel: thread t stores index t of both copies (256 consecutive doubles each).  Index t is register pk_store_reg(t) of
// lane pk_store_lane(t), which in LA is element (pk_store_u, pk_store_v) of the tile and in LB element (pk_store_v, pk_store_u).
PK_HD constexpr int pk_store_lane(int t) { return (t & (kPkHalf - 1)) >> 1; }
PK_HD constexpr int pk_store_reg(int t) { return 2 * (t >> 7) + (t & 1); }
PK_HD constexpr int pk_store_u(int t) { return pk_store_lane(t) & 15; }
PK_HD constexpr int pk_store_v(int t) { return 4 * pk_store_reg(t) + (pk_store_lane(t) >> 4); }

// The pack kernel's fetch.  A workgroup packs a run of up to kPkRun consecutive tiles P0 .. P0 + R - 1 of block diagonal Dblk of one
// table.  Tile (P, P + Dblk) holds the cells (x, y) = (16 P + u, 16 (P + Dblk) + v), which lie on the 31 table diagonals
// y - x = 16 Dblk + dd - 15, dd = 0..30; on each of them the run is ONE contiguous segment x = 16 P0 .. 16 (P0 + R) - 1, whose
// 128-byte lines the workgroup fetches once (one workgroup per tile fetches every line that straddles two tiles twice).  Pass q of
// thread t takes position (t + 256 q) & 127 of diagonal (t + 256 q) >> 7: a wavefront reads 512 contiguous bytes per pass.
constexpr int kPkRun = 8;          // tiles per workgroup
constexpr int kPkRunPasses = 16;   // 31 diagonals x 128 positions in passes of 256 threads
struct PkRunItem { int dd, p, u, v; bool in; };   // table diagonal, tile of the run, element (u, v) of that tile; in: a cell of tile p < R
PK_HD constexpr PkRunItem pk_run_item(int t, int q, int R)
{
    const int item = t + 256 * q, dd = item >> 7, pos = item & 127, p = pos >> 4, u = pos & 15, v = u + dd - 15;
    return PkRunItem{dd, p, u, v, dd < 31 && p < R && v >= 0 && v < 16};
}
// tiles of the run that starts at P0: those with an interior column, Q = P + Dblk < nb and 16 Q <= n - 1 (the others are never read)
PK_HD constexpr int pk_run_tiles(int nb, int n, int Dblk, int P0)
{
    const int lastQ = (n - 1) / 16 < nb - 1 ? (n - 1) / 16 : nb - 1, R = lastQ - Dblk - P0 + 1;
    return R < 0 ? 0 : R < kPkRun ? R : kPkRun;
}
PK_HD constexpr int pk_run_groups(int tiles) { return (tiles + kPkRun - 1) / kPkRun; }

}  // namespace rh
