// pk_layout_check.cpp -- stand-alone host program around the index maps of the packed operand tiles (ractip_amd/csrc/pk_layout.h; the
// kernels are lin_pack_tiles and the block products of mccaskill_far.hip).  No GPU, no HIP; meant to be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/pk_layout_check.cpp -o pk_layout_check
//   ./pk_layout_check
//
// Checked: the element -> index maps of both layouts are bijections on 0..255; load half h of lane l addresses bytes
// 1024 h + 16 l .. + 15 of the tile and holds registers 2h, 2h + 1; register s of lane l is T[l & 15][4 s + (l >> 4)] in layout LA and
// T[4 s + (l >> 4)][l & 15] in LB; LB of a tile is LA of its transpose; the pack kernel's thread -> (element, index) map writes every
// index of both copies exactly once, with the element the readers expect there; and a 16x16x16 product formed from the fragments as
// the kernels form it (four K steps of the 16x16x4 instruction: A[l & 15][l >> 4], B[l >> 4][l & 15]) uses every (row, k) and (k, column)
// pair exactly once; the pack kernel's fetch map (a workgroup takes a run of up to eight tiles of a block diagonal, each table diagonal
// of the run as one contiguous segment) covers exactly the cells of the run's tiles, once each, for runs of 0..8 tiles at the first and
// the last run of every block diagonal at row pitches 66, 502, 503, 512 and 2002.  Prints one summary line; exit status 0 only if nothing differs.  tests/test_pk_layout_cpu.py runs it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pk_layout.h"

namespace {

using namespace rh;

struct Counts { long checks = 0, not_bijection = 0, wrong_bytes = 0, wrong_element = 0, transpose = 0, pack = 0, product = 0, runs = 0, run_cells = 0, run = 0; } G;

static_assert(pk_reg_index(0, 0) == 0 && pk_reg_index(63, 1) == 127 && pk_reg_index(0, 2) == 128 && pk_reg_index(63, 3) == 255);
static_assert(kPkTile == 256 && 2 * kPkHalf == kPkTile);

void bijection(int (*index)(int, int))
{
    std::vector<int> hit(kPkTile, 0);
    for (int u = 0; u < 16; u++)
        for (int v = 0; v < 16; v++) {
            const int x = index(u, v);
            G.checks++;
            if (x < 0 || x >= kPkTile) { G.not_bijection++; continue; }
            hit[x]++;
        }
    for (int x = 0; x < kPkTile; x++) if (hit[x] != 1) G.not_bijection++;
}

// One workgroup of lin_pack_tiles: the run of tiles that starts at P0 on block diagonal Dblk of a sequence of n letters in a batch of
// nmax.  Every cell (u, v) of every tile p < R is fetched exactly once and no other; the table address of a fetched cell is that of
// cell (16 (P0 + p) + u, 16 (P0 + p + Dblk) + v); along a table diagonal the positions are consecutive addresses; R is the number of
// tiles with an interior column, as one workgroup per tile would find it.
unsigned run_sizes = 0;   // bit R: a run of R tiles was checked
void run_of_tiles(int ld, int nmax, int n, int Dblk, int P0)
{
    const int nb = (nmax - 1) / 16 + 1;
    const int R = pk_run_tiles(nb, n, Dblk, P0);
    int want = 0;
    for (int P = P0; P < P0 + kPkRun; P++) want += !(P + Dblk >= nb || (P + Dblk) * 16 > n - 1);
    G.runs++;
    run_sizes |= 1u << (R >= 0 && R <= kPkRun ? R : 31);
    if (R != want || R < 0 || R > kPkRun) { G.run++; return; }
    std::vector<int> got(kPkRun * 256, 0);
    std::vector<long> addr(31 * 128, -1);
    for (int t = 0; t < 256; t++)
        for (int q = 0; q < kPkRunPasses; q++) {
            const PkRunItem it = pk_run_item(t, q, R);
            if (!it.in) continue;
            if (it.p < 0 || it.p >= R || it.u < 0 || it.u > 15 || it.v < 0 || it.v > 15 || it.dd < 0 || it.dd > 30) { G.run++; continue; }
            got[it.p * 256 + it.u * 16 + it.v]++;
            const long x = (long)(P0 + it.p) * 16 + it.u, y = (long)(P0 + it.p + Dblk) * 16 + it.v;
            if (y - x != 16 * Dblk + it.dd - 15) G.run++;
            if (x >= 1 && x <= y && y <= n - 1) {   // cellv reads it
                const long a = (y - x) * ld + x;
                if (a < 0 || a >= (long)ld * ld || x >= ld) G.run++;
                addr[it.dd * 128 + (it.p * 16 + it.u)] = a;
            }
        }
    for (int p = 0; p < kPkRun; p++)
        for (int e = 0; e < 256; e++) {
            G.run_cells += p < R;
            if (got[p * 256 + e] != (p < R ? 1 : 0)) G.run++;
        }
    for (int dd = 0; dd < 31; dd++)
        for (int pos = 0; pos + 1 < 128; pos++)
            if (addr[dd * 128 + pos] >= 0 && addr[dd * 128 + pos + 1] >= 0 && addr[dd * 128 + pos + 1] != addr[dd * 128 + pos] + 1) G.run++;
}

int la(int u, int v) { return pk_la_index(u, v); }
int lb(int u, int v) { return pk_lb_index(u, v); }

}  // namespace

int main()
{
    bijection(la);
    bijection(lb);

    // a tile of distinct values and its transpose, packed in both layouts the way lin_pack_tiles does: thread t stores index t
    double T[16][16], Tt[16][16];
    for (int u = 0; u < 16; u++)
        for (int v = 0; v < 16; v++) { T[u][v] = 1000.0 + 16 * u + v; Tt[v][u] = T[u][v]; }
    std::vector<double> LA(kPkTile, -1.0), LB(kPkTile, -1.0), LAt(kPkTile, -1.0);
    std::vector<int> wrote(kPkTile, 0);
    for (int t = 0; t < 256; t++) {
        const int u = pk_store_u(t), v = pk_store_v(t);
        G.checks++;
        if (u < 0 || u > 15 || v < 0 || v > 15) { G.pack++; continue; }
        if (pk_reg_index(pk_store_lane(t), pk_store_reg(t)) != t || pk_la_index(u, v) != t || pk_lb_index(v, u) != t) G.pack++;
        wrote[t]++;
        LA[t] = T[u][v];
        LB[t] = T[v][u];
        LAt[t] = Tt[u][v];
    }
    for (int t = 0; t < 256; t++) if (wrote[t] != 1) G.pack++;

    // the readers: two loads of two doubles per lane
    std::vector<int> byte_hit(kPkTile * 8, 0);
    for (int l = 0; l < 64; l++)
        for (int h = 0; h < 2; h++) {
            const int off = pk_half_offset(l, h);
            G.checks++;
            if (off * 8 != 1024 * h + 16 * l || off < 0 || off + 1 >= kPkTile) { G.wrong_bytes++; continue; }
            for (int b = 0; b < 16; b++) byte_hit[off * 8 + b]++;
            for (int e = 0; e < 2; e++) {
                const int s = 2 * h + e;   // the register the e-th double of this load becomes
                if (pk_reg_index(l, s) != off + e) G.wrong_bytes++;
                if (LA[off + e] != T[l & 15][4 * s + (l >> 4)]) G.wrong_element++;
                if (LB[off + e] != T[4 * s + (l >> 4)][l & 15]) G.wrong_element++;
                if (LB[off + e] != LAt[off + e]) G.transpose++;
            }
        }
    for (int x : byte_hit) if (x != 1) G.wrong_bytes++;

    // C = A x B from the fragments: step s of the instruction takes A[l & 15][k] and B[k][l & 15] from the lanes with k = 4 s + (l >> 4)
    double C[16][16] = {}, R[16][16] = {};
    double B2[16][16];
    for (int u = 0; u < 16; u++)
        for (int v = 0; v < 16; v++) B2[u][v] = 0.5 + u - 3 * v;
    std::vector<double> LB2(kPkTile);
    for (int t = 0; t < 256; t++) LB2[t] = B2[pk_store_v(t)][pk_store_u(t)];
    for (int s = 0; s < 4; s++)
        for (int q = 0; q < 4; q++)          // k = 4 s + q: the lanes with l >> 4 == q
            for (int r = 0; r < 16; r++)     // A from lane r + 16 q
                for (int c = 0; c < 16; c++) // B from lane c + 16 q
                    C[r][c] += LA[pk_reg_index(r + 16 * q, s)] * LB2[pk_reg_index(c + 16 * q, s)];
    for (int r = 0; r < 16; r++)
        for (int c = 0; c < 16; c++) {
            for (int k = 0; k < 16; k++) R[r][c] += T[r][k] * B2[k][c];
            G.checks++;
            if (std::memcmp(&C[r][c], &R[r][c], sizeof(double)) != 0) G.product++;   // small integers and halves: exact in any order
        }

    // runs of 1..8 tiles at the first and the last run of a block diagonal, at several row pitches; a shorter sequence in the batch too
    for (int ld : {66, 502, 503, 512, 2002}) {
        const int nmax = ld - 2;   // (staging gives even pitches, (nmax + 3) & ~1; the maps do not depend on that)
        const int nb = (nmax - 1) / 16 + 1;
        for (int n : {nmax, nmax - 1, nmax - 17, 66, 40})
            for (int Dblk = 2; Dblk < nb; Dblk++) {
                if (n < 1) continue;
                const int tiles = nb - Dblk;
                if (pk_run_groups(tiles) != (tiles + 7) / 8) G.run++;
                run_of_tiles(ld, nmax, n, Dblk, 0);
                run_of_tiles(ld, nmax, n, Dblk, (pk_run_groups(tiles) - 1) * kPkRun);
            }
    }

    if ((run_sizes & 0x1ffu) != 0x1ffu || run_sizes >> 9) G.run++;   // every run size 0..8 and nothing else

    std::printf("checks %ld not_bijection %ld wrong_bytes %ld wrong_element %ld transpose %ld pack %ld product %ld runs %ld run_cells %ld run %ld\n", G.checks, G.not_bijection,
                G.wrong_bytes, G.wrong_element, G.transpose, G.pack, G.product, G.runs, G.run_cells, G.run);
    return G.not_bijection || G.wrong_bytes || G.wrong_element || G.transpose || G.pack || G.product || G.run ? 1 : 0;
}
