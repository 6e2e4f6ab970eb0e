// local_windows.h -- the window arithmetic of local folding and local hybridization (rh_local_fold, rh_local_duplex, rh_local_duplex2),
// host only: no HIP, no context (local_windows.cpp; checked on the CPU by tools/local_windows_check.cpp, tools/local_duplex_check.cpp
// and tools/local_duplex2_check.cpp).  The two functions the accumulate and finish kernels of local_fold.hip need
// as well -- the start of a window, the windows that contain a run of letters -- are inline here and compile for both sides.
//
// A sequence of n letters is folded in windows of W letters every S letters, We = min(W, n):
//   n <= W: one window, start 0, n letters;
//   else m = ceil((n - W) / S) windows on the grid 0, S, .., (m-1) S and a last one at n - W, which ends at the last letter: nw = m + 1.
// The starts are distinct and increasing.  A run of len letters from i (0-based) lies in window k iff start(k) <= i and
// i + len <= start(k) + We; the windows that contain a run are consecutive.  With S > 1 a run longer than We - S + 1 letters may lie
// in no window.
#pragma once
#include <cstddef>
#include <string>

#include "batch.h"

#if defined(__HIPCC__)
#define RH_LW_HD __host__ __device__ inline
#else
#define RH_LW_HD inline
#endif

namespace rh::host {

struct LocalPlan {
    int n = 0, W = 0, S = 0;   // as asked for
    int We = 0;                // letters per window = min(W, n)
    int nw = 0;                // windows
    int ld = 0;                // row pitch of the band = We: bp_band[i*ld + d] = bp_loc(i, i+d), column 0 and i + d >= n hold 0
};

// RH_OK with *P filled, or RH_ERR_ARG with the reason in *why; reads nothing of seq but whether it is NULL
int local_check(const char* seq, int n, int window, int step, LocalPlan* P, std::string* why);
// doubles of the band and of up, as size_t (n = 1e6, W = 1000: 1e9 doubles)
inline size_t local_band_size(const LocalPlan& P) { return (size_t)P.n * (size_t)P.ld; }
inline size_t local_up_size(const LocalPlan& P, int max_w) { return (size_t)P.n * (size_t)max_w; }

RH_LW_HD int local_start(const LocalPlan& P, int k) { return k + 1 < P.nw ? k * P.S : P.n - P.We; }

// the windows lo..hi that contain letters i .. i+len-1 (lo > hi: none does)
RH_LW_HD void local_window_range(const LocalPlan& P, int i, int len, int* lo, int* hi)
{
    const int m = P.nw - 1;                        // windows on the grid; window m starts at n - We
    const int a = i + len - P.We, last = P.n - P.We;   // a start s contains the run iff a <= s <= i
    int l = a > 0 ? (a + P.S - 1) / P.S : 0, h = i / P.S;
    if (h > m - 1) h = m - 1;
    if (len >= 1 && i >= 0 && a <= last && last <= i) {   // the last window does: behind the grid windows that do, or alone
        if (l > h) l = m;
        h = m;
    }
    *lo = l; *hi = h;
}

// ---- local hybridization (rh_local_duplex): one of two molecules is windowed as above, the other one -- the query -- is whole, and
// window k is hybridized with it as the pair (query, window k) (windowed = 2) or (window k, query) (windowed = 1).  hp_loc(i, j),
// 1-based letters of s1 and s2, is the mean of the windows' hp over the windows that contain the windowed molecule's letter: every
// letter lies in one, so the matrix has no holes.
struct LocalDuplexPlan {
    LocalPlan P;               // of the windowed molecule
    int n1 = 0, n2 = 0;        // letters of s1 and s2
    int windowed = 0;          // 1 or 2
    int nq = 0;                // letters of the query = the other molecule
};

// RH_OK with *D filled, or RH_ERR_ARG with the reason in *why; reads nothing of s1 / s2 but whether they are NULL
int local_duplex_check(const char* s1, int n1, const char* s2, int n2, int windowed, int window, int step, LocalDuplexPlan* D, std::string* why);
// doubles of hp_loc: (n1+1) x (n2+1), row-major, 1-based (n1 = 200, n2 = 1e6: 2e8 doubles)
inline size_t local_hp_size(const LocalDuplexPlan& D) { return ((size_t)D.n1 + 1) * ((size_t)D.n2 + 1); }
// longest s1 / s2 of a chunk's pairs
inline int local_n1max(const LocalDuplexPlan& D) { return D.windowed == 1 ? D.P.We : D.nq; }
inline int local_n2max(const LocalDuplexPlan& D) { return D.windowed == 2 ? D.P.We : D.nq; }

// ---- chunks.  The windows go through the engine in chunks of consecutive windows, each chunk one batch.  Automatic chunking takes
// the largest chunk whose tables stay under kLocalChunkBytes: 4 GiB hold about 700 fold-only windows of 200 letters, several
// workgroups for each of the 256 CUs in every sweep launch, and leave most of the HBM to the caller's other contexts.  A batch is
// one grid dimension: at most kLocalChunkMax sequences, so kLocalChunkMax - 1 windows next to a query.  The sizes come from the
// layout functions of batch.h, with the table counts of the context's model.
constexpr size_t kLocalChunkBytes = (size_t)4 << 30;
constexpr int kLocalChunkMax = 32768;

struct LocalTables {
    int fold = 0;              // square tables per folded sequence (T_COUNT / VM_COUNT)
    int dx = 0, dxl = 0;       // tables per pair of the log-space and of the linear hybridization kernels, which share one buffer
    bool cofold = false;       // hp from the two-molecule ensemble: VM_COUNT tables over query + window per pair as well
};
// bytes of one folded sequence in a batch whose longest sequence has nmax letters: DP tables, operand tiles, posterior
size_t local_fold_bytes(int nmax, const LocalTables& T);
// bytes of one pair: the hybridization tables, the hp block, and under cofold the tables of the concatenation with their tile copies
size_t local_pair_bytes(int n1max, int n2max, const LocalTables& T);
// windows per automatic chunk of rh_local_fold ...
int local_chunk_auto(const LocalPlan& P, const LocalTables& T);
// ... and of rh_local_duplex, where the query's fold counts once per chunk and every window brings its pair
int local_duplex_chunk_auto(const LocalDuplexPlan& D, const LocalTables& T);

// ---- local hybridization of two windowed molecules (rh_local_duplex2): s1 and s2 are both cut into windows as above, each with a
// window and a step of its own, and every window k of s1 is hybridized with every window l of s2.  hp_loc2(i, j), 1-based letters of
// s1 and s2, is a sum of row sums -- over the windows k that contain i, in increasing k, of the sum over the windows l that contain
// j, in increasing l, of h_kl at the translated coordinates -- divided once by the product of the two window counts.
struct LocalDuplex2Plan {
    LocalPlan P1, P2;          // of s1 and of s2
};

// RH_OK with *D filled, or RH_ERR_ARG with the reason in *why; reads nothing of s1 / s2 but whether they are NULL.  Rejects a grid of
// more window pairs than an int indexes (logz_pair[k*nw2 + l]); the product is taken in 64 bits.
int local_duplex2_check(const char* s1, int n1, const char* s2, int n2, int window1, int step1, int window2, int step2, LocalDuplex2Plan* D,
                        std::string* why);
// rh_local_duplex as a grid of window pairs: the query is the one window of its side (start 0, every letter of it in window 0; not
// a plan local_check would give, a query may have one letter), and hp_loc has the layout of hp_loc2
inline LocalDuplex2Plan local_duplex_grid(const LocalDuplexPlan& D)
{
    LocalPlan Q;
    Q.n = Q.W = Q.We = Q.ld = D.nq; Q.S = 1; Q.nw = 1;
    LocalDuplex2Plan G;
    G.P1 = D.windowed == 1 ? D.P : Q;
    G.P2 = D.windowed == 1 ? Q : D.P;
    return G;
}
// doubles of hp_loc2: (n1+1) x (n2+1), row-major, 1-based (n1 = n2 = 1e5: 1e10 doubles) ...
inline size_t local_hp2_size(const LocalDuplex2Plan& D) { return ((size_t)D.P1.n + 1) * ((size_t)D.P2.n + 1); }
// ... of logz_pair [nw1][nw2] ...
inline size_t local_hp2_logz_size(const LocalDuplex2Plan& D) { return (size_t)D.P1.nw * (size_t)D.P2.nw; }
// ... and of the row buffer R[a][ia][j] of `rows` windows of s1: ia = 0..We1 (row 0 unused), j = 0..n2, pitch n2 + 1
inline size_t local_hp2_rowbuf_size(const LocalDuplex2Plan& D, int rows) { return (size_t)rows * ((size_t)D.P1.We + 1) * ((size_t)D.P2.n + 1); }

// Tiles.  The nw1 x nw2 grid of window pairs is walked in rectangles of `rows` consecutive k by `cols` consecutive l -- row blocks in
// increasing k, inside a row block column tiles in increasing l -- each tile one indexed batch of rows + cols folded windows and
// rows x cols pairs.  The automatic tile: the largest t >= 1 with 2t fold + t^2 pair + t rowbuf <= kLocalChunkBytes (rowbuf = the
// row buffer of one k), rows = min(t, nw1), cols = min(t, nw2); where one side was clipped the other one grows while the same sum
// with the actual rows and cols still fits.  Throughout rows + cols <= kLocalChunkMax (the sequences of a batch) and rows x cols <=
// kLocalChunkMax - 1 (the pairs a chunk of rh_local_duplex reaches); (1, 1) when nothing fits.
struct LocalTile { int kA = 0, kB = 0, lA = 0, lB = 0; };   // windows kA .. kB-1 of s1 with lA .. lB-1 of s2
// tile t of the walk under (rows, cols), both already clipped to nw1 / nw2; false behind the last one.  Without a second molecule
// (P2.nw = 0, cols = 0: the chunks of rh_local_fold) a row block is one tile with lA = lB = 0.
inline bool local_tile_at(const LocalDuplex2Plan& D, int rows, int cols, size_t t, LocalTile* out)
{
    const size_t per_block = D.P2.nw > 0 ? ((size_t)D.P2.nw + cols - 1) / cols : 1, kA = t / per_block * rows, lA = t % per_block * cols;
    if (kA >= (size_t)D.P1.nw) return false;
    out->kA = (int)kA; out->kB = D.P1.nw - (int)kA < rows ? D.P1.nw : (int)kA + rows;
    out->lA = (int)lA; out->lB = D.P2.nw - (int)lA < cols ? D.P2.nw : (int)lA + cols;
    return true;
}
bool local_tile_fits(const LocalDuplex2Plan& D, const LocalTables& T, size_t rows, size_t cols);
void local_tile_auto(const LocalDuplex2Plan& D, const LocalTables& T, int* rows, int* cols);

}  // namespace rh::host
