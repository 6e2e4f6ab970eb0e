// batch.h -- HBM layout of one batch of independent DP problems.
//
// McCaskill side: NS sequences (2 per pair).  Every DP table is a square
// ld x ld array of doubles per sequence (ld = nmax+2, gap indices 0..n on both
// axes, element [r*ld+c]); tables that are read along a column by some
// recurrence are ALSO stored transposed so that every inner loop of every kernel
// streams two contiguous rows.  Only interior cells 1 <= i <= j <= n-1 are ever
// read, and each is fully (re)written by the sweep, so tables need no clearing
// between batches.
//
// Duplex side: NP pairs, tables (n1max+2) x ldd, 1-based letters.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

namespace rh {

// ---- McCaskill tables (gap-indexed cell (i,j): letters i+1..j inside; FC assumes
//      letters (i, j+1) paired -- InferenceEngine.ipp:3556-3567)
enum McTable {
    T_FC = 0,   // FCi[i][j]
    T_FCX,      // FCi + ScoreBasePair(i,j+1) + ScoreJunctionB(j+1,i-1): operand of single-branch loops
    T_FCA,      // FCi + ScoreBasePair(i,j+1) + ScoreJunctionA(j+1,i-1): operand of FM1 / F5
    T_FCAT,     // transpose of T_FCA  ([j][i])
    T_FM1,      // FM1i[i][j]
    T_FM1T,     // [j][i]
    T_FM,       // FMi[i][j]
    T_FMT,      // [j][i]
    T_FCO,      // FCo[i][j]
    T_FCOX,     // FCo + ScoreJunctionB(i,j): operand of the outside single-branch gather
    T_FM2O,     // FM2o[i][j]
    T_FM2OT,    // [j][i]
    T_FMO,      // FMo[i][j]
    T_FM1O,     // FM1o[i][j]
    T_COUNT
};

// ---- scaled linear McCaskill path (mccaskill_lin.hip, mccaskill_strip.hip, mccaskill_far.hip): the same buffer, tables stored
//      DIAGONAL-MAJOR (cell (i, i+d) at [d*ld + i])
enum LinTable { L_FC = 0, L_FCX, L_FCA, L_FM1, L_FM, L_FCO, L_FCOX, L_FM2O, L_FMO, L_FM1O,
                L_FM2F, L_FMOF, L_FM1OF,  // far-block partial sums (mccaskill_far.hip)
                L_COUNT };
static_assert((int)L_COUNT <= (int)T_COUNT, "linear tables reuse the log-space table buffer");

// ---- Vienna-BL model, log space (mccaskill_vienna.hip): square ld x ld tables per sequence; *T = stored transposed ([j][i])
enum VmTable { VM_FC = 0, VM_FCX, VM_FCA, VM_FCAT, VM_FM1, VM_FM1T, VM_FM, VM_FMT, VM_FMST,
               VM_FCO, VM_FCOX, VM_FM2O, VM_FM2OT, VM_FMSOT, VM_FM1O, VM_FCOT,
               VM_COUNT };   // tables per sequence of a Vienna-BL batch, log space or linear

// ---- Vienna-BL model, scaled linear space (mccaskill_vlin.hip): diagonal-major, and the block products of mccaskill_far.hip run on
//      these tables too, so the slots they address are LinTable's
enum VLinTable { VL_FC = L_FC, VL_FCX = L_FCX, VL_FCA = L_FCA, VL_FM1 = L_FM1, VL_FM = L_FM, VL_FCO = L_FCO, VL_FCOX = L_FCOX, VL_FM2O = L_FM2O,
                 VL_FMSO = L_FMO,   // the Vienna grammar keeps FMSo in that slot
                 VL_FM1O = L_FM1O, VL_FM2F = L_FM2F, VL_FMOF = L_FMOF, VL_FM1OF = L_FM1OF,
                 VL_FMS = L_COUNT, VL_FCB, VL_FCOB, VL_COUNT };
static_assert((int)VL_COUNT <= (int)VM_COUNT, "linear tables reuse the log-space table buffer");

struct McBatch {
    const uint8_t* seq;  // [NS][lds] nucleotide codes, seq[0] = seq[n+1] = 4
    const int* n;        // [NS]
    double* tab;         // [NS][T_COUNT][ld*ld]
    double* f5i;         // [NS][ld]  F5i[0..n]
    double* f5o;         // [NS][ld]  F5o[0..n]
    double* bp;          // [NS][tri_stride] posterior, reference triangular layout
    double* up;          // [NS][ld*max_w]  up[i*max_w+w] = P(letters i+1..i+1+w unpaired); max_w = 1 for the CONTRAfold model
    // two-molecule form (co_pf_fold semantics, mccaskill_vienna.hip only): cut[sq] = n1 > 0 means the sequence is s1+s2
    // and the backbone gap after letter n1 does not exist; xp/xs = exterior partition functions of s2's prefixes
    // cut+1..b and s1's suffixes a..cut, xpo/xso their outside counterparts.  cut == nullptr: one molecule each.
    // structure constraints (fold_constrained, Vienna-BL kernels only): allow[sq*ld*ld + a*ld + b] != 0 iff letters a < b may
    // pair; nullptr = unconstrained
    const uint8_t* allow;
    const int* cut;      // [NS] or nullptr
    double* xp;          // [NS][ld]
    double* xs;
    double* xpo;
    double* xso;
    int ns, nmax, ld, lds;
    size_t tab_stride;   // doubles per table  (ld*ld)
    size_t seq_stride;   // doubles per sequence (T_COUNT*ld*ld)
    size_t tri_stride;   // doubles per bp table
    // operand tiles of the block products (mccaskill_far.hip): kPkCopies re-laid copies of the 16x16 tiles (P <= Q) of
    // FM1 / FM / FM2o, each tile 256 doubles in MFMA fragment order; [NS][kPkCopies][pk_stride]
    double* rowp;        // [NS][2][ld] look-ahead partial sums of the next inside diagonal (mccaskill_lin.hip, MODE 1 -> 2)
    double* pk;
    size_t pk_stride;    // doubles per copy = nb*(nb+1)/2 * 256
    int nb;              // 16-blocks per axis = (nmax-1)/16 + 1
    // two-molecule batch, scaled linear kernels: the one-strand cells of the inside tables were copied from the single-molecule
    // folds of the same upload (vlin_co_seed), so the inside sweep computes only the groups that touch both strands
    int seeded;
};
constexpr int kPkCopies = 6;
// sequences of kSmallMin .. kSmallMax letters are folded by mccaskill_small.hip (one workgroup each, tables in LDS); the upper bound is
// what three triangles of doubles plus the partial-sum buffers leave of 160 KB
constexpr int kSmallMin = 8, kSmallMax = 109;
// the strip kernels (mccaskill_strip.hip) run when the longest sequence the sweeps see has at least this many letters (one strip behind the
// 32 bootstrap diagonals); shorter sequences of such a batch get a pass of their own (launch_contrafold.hip: launch_mc_lin)
constexpr int kStripMinN = 40;
// layout of rh_ctx::d_wT: transposed weights of the strip kernels [31][40], their factored tables, zero-padded rows [31][32] for mccaskill_small.hip
constexpr int kStripFiltOff = 31 * 40, kStripFiltLen = 232, kSmallWLen = 31 * 32;

enum DxTable {
    D_IN = 0,  // inside[i][j]
    D_INX,     // inside + terminal_mismatch[s1[i]][s2[j]][s1[i+1]][s2[j-1]]: as upstream pair of a loop
    D_OUT,     // outside[i][j]
    D_OUTX,    // outside + terminal_mismatch[s2[j]][s1[i]][s2[j+1]][s1[i-1]] + base_pair[s1[i]][s2[j]]
    D_COUNT
};
// Vienna-BL model, log space (duplex_vienna.hip): the same layout, IN / OUT and two decorated copies of each
enum DxvTable { V_IN = 0, V_INMM, V_INTAU, V_OUT, V_OUTMM, V_OUTTAU, V_COUNT };

struct DxBatch {
    const uint8_t* seq;  // the McCaskill sequence buffer: pair p = sequences 2p (s1) and 2p+1 (s2)
    const int* n;        // [2*NP]
    double* tab;         // [NP][D_COUNT][rows*ldd]
    double* hp;          // [NP][rows*ldd]  posterior, 1-based, row/col 0 zero
    double* logz;        // [NP]
    int np, n1max, n2max, ldd, lds;
    size_t tab_stride;   // rows*ldd
    size_t pair_stride;  // D_COUNT*rows*ldd
};

// ---- duplex, scaled linear path: anti-diagonal-major tables [sd*lda + kDxPad + a], a = i, sd = i + (L2+1-j)
constexpr int kDxPad = 32;   // zero columns on both sides of every row (>= 29: the longest window reach)
// How far from its cells a row is ever read.  Row sd has cells at columns alo(sd) = max(1, sd-L2) .. ahi(sd) = min(L1, sd-1); both grow
// with sd, by at most one per row.  A kept cell (sd, a), alo(sd) <= a <= ahi(sd), reads, with dir = -1 (inside) / +1 (outside):
//   * row sd + dir*(2+t), t = 0..28, at columns a + dir*(1..t+1)   (windows: win_pass8 / win_pass4 / win_pass; t <= 2: dx_cell_loads;
//     rows of the same strip: finish);
// Inside, that row r = sd-2-t has alo(r) <= alo(sd) and ahi(r) >= ahi(sd)-2-t, and the columns are a-1-t .. a-1: not below
// alo(sd)-1-t >= alo(r)-29 and not above ahi(sd)-1 <= ahi(r)+t+1 <= ahi(r)+29.  Outside, r = sd+2+t has alo(r) <= alo(sd)+2+t and
// ahi(r) >= ahi(sd), and the columns are a+1 .. a+1+t: not below alo(sd)+1 >= alo(r)-t-1 >= alo(r)-29 and not above ahi(sd)+1+t <=
// ahi(r)+29.  So every read of a kept cell lies in [alo(r)-29, ahi(r)+29] of the row it reads (tests/test_gpu_stale_tables.py enumerates it);
// a row kept correct on [alo-kDxBand, ahi+kDxBand] serves every reader, and the zero pad columns are that band where it leaves the row.
constexpr int kDxBand = 32;
static_assert(kDxBand >= 30 && kDxBand <= kDxPad, "the band covers every read and ends inside the pad columns");
// dxl_strip8: the groups of 58 columns that [lo - kDxBand, hi + kDxBand] can touch when lo..hi spans the cells of the eight rows of launch `step`, for any
// pair with L1 <= n1max, L2 <= n2max: a row has at most min(L1, L2, sd-1, L1+L2-sd+1) cells, the first row of the launch (inside
// sd = 2+8 step, outside sd = L1+L2-8 step-7) so at most cnt = min(n1max, n2max, 8 step+8, n1max+n2max-8 step-1), the eight rows together
// span at most cnt+7 columns, and an interval of n columns meets at most (n-1)/58 + 2 groups
inline int dxl_strip8_groups(int n1max, int n2max, int step)
{
    const int all = (n1max + 2 + 57) / 58;
    int cnt = n1max < n2max ? n1max : n2max;
    if (8 * step + 8 < cnt) cnt = 8 * step + 8;
    const int rest = n1max + n2max - 8 * step - 1;
    if ((rest > 1 ? rest : 1) < cnt) cnt = rest > 1 ? rest : 1;
    const int g = (cnt + 7 + 2 * kDxBand - 1) / 58 + 2;
    return g < all ? g : all;
}

enum DxLinTable { DL_IN = 0, DL_INX, DL_OUT, DL_OUTX, DL_COUNT };
// Vienna-BL model (duplex_vlin.hip): VD_COUNT tables per pair under 1.8 semantics, VD_COUNT20 under 2.x; IN / OUT at DL_IN / DL_OUT: dxl_posterior reads them
enum DxvLinTable { VD_IN = 0, VD_INX, VD_OUT, VD_OUTX, VD_INT, VD_OUTT, VD_IN1N, VD_OUT1N, VD_IN23, VD_OUT23, VD_COUNT20, VD_COUNT = VD_IN1N };
static_assert((int)VD_IN == (int)DL_IN && (int)VD_OUT == (int)DL_OUT, "dxl_posterior serves both models");

struct DxLinBatch {
    const uint8_t* seq;
    const int* n;        // [2*NP]
    double* tab;         // [NP][DL_COUNT][rows*lda]
    double* hp;          // same posterior buffer / layout as DxBatch::hp
    int np, n1max, n2max, lda, lds, ldd;
    size_t tab_stride;   // rows*lda (+ slack)
    size_t pair_stride;  // DL_COUNT*tab_stride
    size_t hp_stride;
    double pw_in[2];     // (lam*e^eu)^(sd-2) * lam^2 for the two inside diagonals of this launch
    double pw_out[2];    // (lam*e^eu)^(L1+L2-sd) * lam^2 for the two outside diagonals
    double pw4[4];       // dxl_sweep4: (lam*e^eu)^(4*step+k) * lam^2, k = 0..3 (the same for both directions)
    double pw8[8];       // dxl_strip8: (lam*e^eu)^(8*step+k) * lam^2, k = 0..7
};

// ---- The layout of every table kind, stated once: the upload (staging.hip), the sub-batches of the scale-exponent ladder
// (fallbacks.hip) and the CPU check (tools/batch_request_check.cpp) all size and stride by these.  Host functions; each returns
// zeroed storage with the shape fields filled (an argument of a captured graph is hashed by its bytes) and no pointer bound.
inline size_t tri_size(int n) { return (size_t)(n + 1) * (n + 2) / 2; }
inline int seq_lds(int nmax) { return (nmax + 3 + 15) & ~15; }   // row pitch of the letter codes: 0..n+2 readable

// ns sequences of at most nmax letters with `tables` square tables each (T_COUNT, or VM_COUNT: Vienna-BL, one molecule or s1+s2)
inline McBatch mc_layout(int ns, int nmax, int tables)
{
    McBatch B{};
    B.ns = ns; B.nmax = nmax;
    B.lds = seq_lds(nmax);
    B.ld = (nmax + 2 + 1) & ~1;
    B.tab_stride = (size_t)B.ld * B.ld;
    B.seq_stride = B.tab_stride * tables;
    B.tri_stride = (tri_size(nmax) + 1) & ~(size_t)1;
    B.nb = (nmax - 1) / 16 + 1;
    B.pk_stride = (size_t)B.nb * (B.nb + 1) / 2 * 256;
    return B;
}

// np pairs of at most n1max x n2max letters, `tables` tables of (n1max+2) x ldd each; lds: the row pitch of the codes
inline DxBatch dx_layout(int np, int n1max, int n2max, int lds, int tables)
{
    DxBatch D{};
    D.np = np; D.n1max = n1max; D.n2max = n2max; D.lds = lds;
    D.ldd = (n2max + 2 + 1) & ~1;
    D.tab_stride = (size_t)(n1max + 2) * D.ldd;
    D.pair_stride = D.tab_stride * tables;
    return D;
}

// the same pairs on the linear path: `tables` anti-diagonal-major tables of n1max+n2max+3 rows, kDxPad zero columns on both sides of
// every row and a slack behind the last one (the staged 96-column segments may run past it); ldd: of the posterior they write
inline DxLinBatch dxl_layout(int np, int n1max, int n2max, int lds, int ldd, int tables)
{
    DxLinBatch X{};
    X.np = np; X.n1max = n1max; X.n2max = n2max; X.lds = lds; X.ldd = ldd;
    X.lda = (n1max + 2 + 2 * kDxPad + 1) & ~1;
    const size_t rows = (size_t)n1max + n2max + 3;
    X.tab_stride = rows * X.lda + 128;
    X.pair_stride = X.tab_stride * tables;
    return X;
}

// ---- The packed float image of a batch's dense results (rh_batch_packed_layout; written by pack_results.hip, checked on the CPU by
// tools/packed_layout_check.cpp): three arrays of floats, each a row of blocks at their tight sizes in the reference's layouts --
//   bp: sequence k owns tri_size(n_k) floats, the triangular table for ITS n;  up: n_k * max_w floats, up[i*max_w + w];
//   hp: pair p owns (n1+1) * (n2+1) floats, row-major, 1-based, row 0 and column 0 zero (pair p = sequences pair_seq[2p], pair_seq[2p+1]).
// Every block starts at a multiple of kPackAlign elements (16 bytes); the floats between the end of a block and the start of the next
// one (behind the last block: the total) are padding and hold 0.  Offsets and totals count elements and are 64-bit: 512 pairs of
// 2000 + 2000 letters hold 2.05e9 hp entries (8.2e9 bytes), 2048 of them more than 2^32.  bp_off / up_off have nseq + 1 entries, hp_off npairs + 1; the last entry of
// each is its total.
constexpr size_t kPackAlign = 4;
inline size_t pack_pad(size_t elements) { return (elements + kPackAlign - 1) & ~(kPackAlign - 1); }
inline void packed_layout(int nseq, const int* lens, int npairs, const int* pair_seq, int max_w, size_t* bp_off, size_t* up_off, size_t* hp_off,
                          size_t totals[3])
{
    bp_off[0] = up_off[0] = hp_off[0] = 0;
    for (int k = 0; k < nseq; k++) {
        bp_off[k + 1] = bp_off[k] + pack_pad(tri_size(lens[k]));
        up_off[k + 1] = up_off[k] + pack_pad((size_t)lens[k] * max_w);
    }
    for (int p = 0; p < npairs; p++)
        hp_off[p + 1] = hp_off[p] + pack_pad(((size_t)lens[pair_seq[2 * p]] + 1) * ((size_t)lens[pair_seq[2 * p + 1]] + 1));
    totals[0] = bp_off[nseq]; totals[1] = up_off[nseq]; totals[2] = hp_off[npairs];
}

// chunks of kLzRows = 16 anti-diagonals of the duplex log Z sums
inline int lz_chunks(int n1max, int n2max) { return (n1max + n2max - 1 + 15) / 16; }

// out[d], d < count: the weight of a hairpin of d unpaired letters (beyond 30 as part_func.c extrapolates) x lam^d.  Model: VLinModel
// (vienna_model.h; a template so that this header, and a CPU program that includes it, needs no HIP)
template <class Model>
inline void hairpin_length_weights(const Model& H, int count, double* out)
{
    for (int d = 0; d < count; d++)
        out[d] = (d <= 30 ? H.E_hairpin[d] : std::exp(H.hairpin30 - H.lxc * std::log(d / 30.0))) * std::exp(-H.s * d);
}

}  // namespace rh
