// launch_contrafold.hip -- launch sequences of the CONTRAfold-model McCaskill sweeps: the log-space path, the scaled
// linear path with its block products, strips and per-sequence routing, and the strip kernels' weight tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "kernels.h"

// log-space path: logZ = F5i[n] (InferenceEngine.ipp:4089-4094)
__global__ void log_finish(rh::McBatch B, double* __restrict__ logz)
{
    const int sq = blockIdx.x * blockDim.x + threadIdx.x;
    if (sq < B.ns) logz[sq] = B.f5i[(size_t)sq * B.ld + B.n[sq]];
}

namespace rh::host {

// ---- McCaskill sweeps, log-space path (always valid)
int launch_mc_log(rh_ctx* c, int pin, const McBatch& B, double* logz_out)
{
    hipLaunchKernelGGL(mc_init, dim3((B.ns + 63) / 64), dim3(64), 0, c->s_mc, B);
    for (int d = 0; d <= B.nmax - 1; d++) {
        const int waves = std::max(B.nmax - 1 - d, 0) + 1;
        KLAUNCH(c, 0, mc_inside_diag, pin ? dim3(B.ns, (waves + 3) / 4) : dim3((waves + 3) / 4, B.ns), dim3(256), c->s_mc, B, c->d_model, d, pin);
        c->n_launch[0]++;
    }
    HIP_TRY(c, hipEventRecord(c->ev[1], c->s_mc));
    for (int d = B.nmax - 2; d >= 0; d--) {
        const int waves = (B.nmax - 1 - d) + 1;
        KLAUNCH(c, 2, mc_outside_diag, pin ? dim3(B.ns, (waves + 3) / 4) : dim3((waves + 3) / 4, B.ns), dim3(256), c->s_mc, B, c->d_model, d, pin);
        c->n_launch[1]++;
    }
    hipLaunchKernelGGL(log_finish, dim3((B.ns + 63) / 64), dim3(64), 0, c->s_mc, B, logz_out);
    hipLaunchKernelGGL(mc_unpaired, dim3((B.nmax + 63) / 64, B.ns), dim3(256), 0, c->s_mc, B);
    return RH_OK;
}
int launch_mc_log(rh_ctx* c, int pin) { return launch_mc_log(c, pin, c->mc, c->d_mclogz.as<double>()); }

// ---- block products (mccaskill_far.hip, BS = 16) on re-laid operand tiles: the tiles of block diagonal Dblk are packed once,
// right after their last cell is final, and then read by every product that uses them as two contiguous 2 KB fragments.
//   inside : far(D) uses FM1/FM tiles of block diagonals 2..D-2; block diagonal D-2 completes with fine diagonal (D-1)*16-1
//   outside: far(D) uses FM2o tiles of block diagonals >= D+2 (final before fine diagonal (D+1)*16-1) and FM1/FM tiles of
//            every block diagonal (the last two are packed when the outside phase starts)
// returns the number of launches it counts: 1 (the pack launch rides with its product; bench.py adds its traffic to the product's)
// two-level products (64x64 macro tiles under the 16x16 tile kernels, mccaskill_far.hip) pay from 6 macro blocks per axis on
// (measured: n = 200, 300 equal, n = 400 +2 %, n = 500 +4 %, n = 2000 +27 %)
// returns the length from which a SEQUENCE takes the two-level form (0: no sequence of this batch does)
int far_two_level(const rh_ctx* c, const McBatch& B)
{
    const int from = c->far2 >= 0 ? (c->far2 ? 1 : 0) : 384;
    return from > 0 && B.nmax >= from ? from : 0;
}

int far_inside_step(rh_ctx* c, const McBatch& B, hipStream_t st, int D, int last_block, int banded)
{
    if (!c->far_pk) { KLAUNCH(c, 1, lin_far_inside_mfma, dim3(last_block - D + 1, B.ns), dim3(256), st, B, D); return 1; }
    const int l2 = far_two_level(c, B);
    KLAUNCH(c, 1, lin_pack_tiles<0>, dim3(B.nb - (D - 2), B.ns, 2), dim3(256), st, B, D - 2, 0, banded);
    if (l2 && (D + 3) % 4 == 0) {   // D = 4*D2-3: every operand tile of macro block diagonal D2 is packed now
        const int D2 = (D + 3) / 4, last2 = (B.nmax - 1) / 64;
        if (D2 >= 4 && D2 <= last2) KLAUNCH(c, 1, lin_far2_inside, dim3(last2 - D2 + 1, B.ns), dim3(256), st, B, D2, l2);
    }
    KLAUNCH(c, 1, lin_far_inside_pk, dim3(last_block - D + 1, B.ns), dim3(256), st, B, D, l2);
    return 1;
}
// repack2: the inside sweep left block diagonal 2 packed in the other form (masked for the banded split / plain for the block split)
int far_outside_begin(rh_ctx* c, const McBatch& B, hipStream_t st, int last_block, int banded, bool repack2)
{
    if (!c->far_pk) return 0;
    c->far2_next = (B.nmax - 1) / 64;   // macro block diagonals whose 64-block products are still to be launched (descending)
    if (repack2 && last_block - 1 > 2) KLAUNCH(c, 3, lin_pack_tiles<1>, dim3(B.nb - 2, B.ns, 2), dim3(256), st, B, 2, 0, banded);
    for (int Dblk = std::max(2, last_block - 1); Dblk <= last_block; Dblk++)
        KLAUNCH(c, 3, lin_pack_tiles<1>, dim3(B.nb - Dblk, B.ns, 2), dim3(256), st, B, Dblk, 0, banded);
    return 0;
}
int far_outside_step(rh_ctx* c, const McBatch& B, hipStream_t st, int D, int last_block)
{
    if (!c->far_pk) { KLAUNCH(c, 3, lin_far_outside_mfma, dim3(last_block - D + 1, B.ns, 2), dim3(256), st, B, D); return 1; }
    const int l2 = far_two_level(c, B);
    if (D + 2 <= last_block) KLAUNCH(c, 3, lin_pack_tiles<1>, dim3(B.nb - (D + 2), B.ns, 1), dim3(256), st, B, D + 2, 1, 0);
    if (l2) {   // macro block diagonal D2 holds tile block diagonals 4*D2-3 .. 4*D2+3: its products go first, their FM2o tiles (block diagonals >= 4*D2+5) are packed
        const int last2 = (B.nmax - 1) / 64;
        for (; c->far2_next >= 0 && 4 * c->far2_next + 3 >= D; c->far2_next--)
            KLAUNCH(c, 3, lin_far2_outside, dim3(last2 - c->far2_next + 1, B.ns, 2), dim3(256), st, B, c->far2_next, l2);
    }
    KLAUNCH(c, 3, lin_far_outside_pk, dim3(last_block - D + 1, B.ns, 2), dim3(256), st, B, D, l2);
    return 1;
}

// ---- McCaskill sweeps, scaled linear-space path (fast; flags sequences that left the double range)
// BS > 0: block products (mccaskill_far.hip) take the k-terms of complete blocks; schedule:
//   inside : far(D) right after fine diagonal (D-1)*BS-1  (its operands are final, tile (I,I+D) starts at (D-1)*BS+1)
//   outside: far(D) right before fine diagonal (D+1)*BS-1 (operands: spans >= (D+1)*BS+1, already final)
// the strip kernels need the packed block products (masked tiles) and at least one strip behind the 32 bootstrap diagonals
bool strip_inside(const rh_ctx* c, const McBatch& B) { return (c->strip & 1) && c->far_pk && c->far_mfma && c->lin_bs == 16 && B.nmax >= kStripMinN; }
bool strip_outside(const rh_ctx* c, const McBatch& B) { return (c->strip & 2) && c->far_pk && c->far_mfma && c->lin_bs == 16 && B.nmax >= kStripMinN; }

// the sweeps of one phase over the sequences B shows (lengths 0 hide a sequence); BR: the batch as uploaded (lin_init / lin_finish /
// mc_unpaired see every sequence)
template <int W, int BS>
int launch_mc_lin_body(rh_ctx* c, int pin, int phase, const McBatch& B, const McBatch& BR, bool init, bool finish)
{
    int* bad = c->d_bad.as<int>();
    const int last_block = BS > 0 ? (B.nmax - 1) / BS : 0;
    if (phase == 0) {
    if (init) hipLaunchKernelGGL(lin_init, dim3((BR.ns + 63) / 64), dim3(64), 0, c->s_mc, BR, c->lin->d, bad);
    if constexpr (W == 4 && BS == 16) {
        if (strip_inside(c, B)) {
            // diagonals 0..31 by pairs (every row is "near" there), then strips of kStripKD diagonals (mccaskill_strip.hip)
            constexpr int KD = 8, GS = 64 - (KD - 1);
            for (int d = 0; d < 32; d += 2) {
                const int groups = (std::max(B.nmax - 1 - d, 0) + 62) / 63 + 1;
                KLAUNCH(c, 0, (lin_inside_diag<4, 16, 3>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64 * W), c->s_mc, B, c->lin->d, d,
                        std::exp(-c->lin->h.s * d), pin);
                c->n_launch[0]++;
            }
            int d0 = 32;
            for (; d0 <= B.nmax - 2; d0 += KD) {
                const int groups = (std::max(B.nmax - 1 - d0, 0) + GS - 1) / GS + 1;
                if (c->strip_w == 4)
                    KLAUNCH(c, 0, (lin_inside_strip<KD, 4, 0>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(256), c->s_mc, B, c->lin->d, c->lin->wT, d0,
                            d0 == 32 ? 32 : d0 - KD + 2, std::exp(-c->lin->h.s * d0), (pin && c->strip_xcd) ? 2 : pin);
                else if (c->strip_filt && c->strip_filt_ok)
                    KLAUNCH(c, 0, (lin_inside_strip<KD, 8, 1>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(512), c->s_mc, B, c->lin->d, c->lin->wT, d0,
                            d0 == 32 ? 32 : d0 - KD + 2, std::exp(-c->lin->h.s * d0), (pin && c->strip_xcd) ? 2 : pin);
                else
                    KLAUNCH(c, 0, (lin_inside_strip<KD, 8, 0>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(512), c->s_mc, B, c->lin->d, c->lin->wT, d0,
                            d0 == 32 ? 32 : d0 - KD + 2, std::exp(-c->lin->h.s * d0), (pin && c->strip_xcd) ? 2 : pin);
                c->n_launch[0]++;
                if ((d0 + KD) % BS == 0) {
                    const int D = (d0 + KD) / BS + 1;
                    if (D >= 4 && D <= last_block) { c->n_launch[0] += far_inside_step(c, B, c->s_mc, D, last_block, 1); c->n_far[0]++; }
                }
            }
            hipLaunchKernelGGL(lin_f5i_tail, dim3(B.ns), dim3(256), 0, c->s_mc, B, c->lin->d, d0 - KD + 2);
            return RH_OK;
        }
        if (c->lookahead == 2) {   // two diagonals per launch (lin_inside_diag MODE 3); the last launch may hold only F5i[nmax]
            for (int d = 0; d <= B.nmax; d += 2) {
                const int groups = (std::max(B.nmax - 1 - d, 0) + 62) / 63 + 1;
                KLAUNCH(c, 0, (lin_inside_diag<4, 16, 3>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64 * W), c->s_mc, B, c->lin->d, d,
                        std::exp(-c->lin->h.s * d), pin);
                c->n_launch[0]++;
                if ((d + 2) % BS == 0) {
                    const int D = (d + 2) / BS + 1;
                    if (D >= 4 && D <= last_block) { c->n_launch[0] += far_inside_step(c, B, c->s_mc, D, last_block); c->n_far[0]++; }
                }
            }
            return RH_OK;
        }
    }
    for (int d = 0; d <= B.nmax - 1; d++) {
        const int groups = (std::max(B.nmax - 1 - d, 0) + 63) / 64 + 1;
        if constexpr (W == 4 && BS == 16) {
            if (c->lookahead && (d & 1) == 0)      // even diagonal: also accumulates the look-ahead sums of d+1 ...
                KLAUNCH(c, 0, (lin_inside_diag<4, 16, 1>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64 * W), c->s_mc, B, c->lin->d, d,
                        std::exp(-c->lin->h.s * d), pin);
            else if (c->lookahead)                 // ... which then needs one wavefront per group
                KLAUNCH(c, 0, (lin_inside_diag<4, 16, 2>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64), c->s_mc, B, c->lin->d, d,
                        std::exp(-c->lin->h.s * d), pin);
            else
                KLAUNCH(c, 0, (lin_inside_diag<W, BS, 0>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64 * W), c->s_mc, B, c->lin->d, d,
                        std::exp(-c->lin->h.s * d), pin);
        } else {
            KLAUNCH(c, 0, (lin_inside_diag<W, BS, 0>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64 * W), c->s_mc, B, c->lin->d, d,
                    std::exp(-c->lin->h.s * d), pin);
        }
        c->n_launch[0]++;
        if (BS > 0 && (d + 1) % BS == 0) {
            const int D = (d + 1) / BS + 1;
            if (D >= 4 && D <= last_block) {
                if (BS == 16 && c->far_mfma) c->n_launch[0] += far_inside_step(c, B, c->s_mc, D, last_block);
                else {
                    KLAUNCH(c, 1, lin_far_inside<(BS > 0 ? BS : 16)>, dim3(last_block - D + 1, B.ns), dim3(256), c->s_mc, B, D);
                    c->n_launch[0]++;
                }
                c->n_far[0]++;
            }
        }
    }
    return RH_OK;
    }
    const bool in_banded = (W == 4 && BS == 16) && strip_inside(c, B);
    if constexpr (W == 4 && BS == 16) {
        if (strip_outside(c, B)) {
            // strips of KD diagonals from the top (mccaskill_strip.hip), banded near/far split: block diagonal 2 of FM1 / FM is packed masked
            constexpr int KD = 8, GS = 64 - (KD - 1);
            c->n_launch[1] += far_outside_begin(c, B, c->s_mc, last_block, 1, !in_banded);
            const int d0_top = (B.nmax - 2) | (KD - 1);
            for (int D = last_block; D >= 0 && (D + 1) * BS - 1 > d0_top; D--) { c->n_launch[1] += far_outside_step(c, B, c->s_mc, D, last_block); c->n_far[1]++; }
            hipLaunchKernelGGL(lin_f5o_head, dim3(B.ns), dim3(256), 0, c->s_mc, B, c->lin->d, B.nmax - 1, d0_top - 5);
            for (int d0 = d0_top; d0 >= KD - 1; d0 -= KD) {
                if ((d0 + 1) % BS == 0) {
                    const int D = (d0 + 1) / BS - 1;
                    if (D >= 0 && D <= last_block) { c->n_launch[1] += far_outside_step(c, B, c->s_mc, D, last_block); c->n_far[1]++; }
                }
                const int groups = (std::max(B.nmax - 1 - (d0 - (KD - 1)), 0) + GS - 1) / GS + 1;
                if (c->strip_w == 4)
                    KLAUNCH(c, 2, (lin_outside_strip<KD, 4, 0>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(256), c->s_mc, B, c->lin->d, c->lin->wT, d0,
                            d0 - 6, d0 - 13, (pin && c->strip_xcd) ? 2 : pin, bad);
                else if (c->strip_filt && c->strip_filt_ok)
                    KLAUNCH(c, 2, (lin_outside_strip<KD, 8, 1>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(512), c->s_mc, B, c->lin->d, c->lin->wT, d0,
                            d0 - 6, d0 - 13, (pin && c->strip_xcd) ? 2 : pin, bad);
                else
                    KLAUNCH(c, 2, (lin_outside_strip<KD, 8, 0>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(512), c->s_mc, B, c->lin->d, c->lin->wT, d0,
                            d0 - 6, d0 - 13, (pin && c->strip_xcd) ? 2 : pin, bad);
                c->n_launch[1]++;
            }
            if (finish) hipLaunchKernelGGL(lin_finish, dim3((BR.ns + 63) / 64), dim3(64), 0, c->s_mc, BR, c->lin->d, c->d_mclogz.as<double>(), bad);
            if (finish) hipLaunchKernelGGL(mc_unpaired, dim3((BR.nmax + 63) / 64, BR.ns), dim3(256), 0, c->s_mc, BR);
            return RH_OK;
        }
    }
    if (BS == 16 && c->far_mfma) c->n_launch[1] += far_outside_begin(c, B, c->s_mc, last_block, 0, in_banded);
    if (BS > 0)  // tiles whose first cell would come before the first outside diagonal: their far sums are empty
        for (int D = last_block; D >= 0 && (D + 1) * BS - 1 > B.nmax - 2; D--) {
            if (BS == 16 && c->far_mfma) c->n_launch[1] += far_outside_step(c, B, c->s_mc, D, last_block);
            else {
                KLAUNCH(c, 3, lin_far_outside<(BS > 0 ? BS : 16)>, dim3(last_block - D + 1, B.ns, 2), dim3(256), c->s_mc, B, D);
                c->n_launch[1]++;
            }
            c->n_far[1]++;
        }
    if constexpr (BS == 16 && (W == 8 || W == 4)) {
        if (c->lookahead == 2 && c->far_mfma) {   // two diagonals per launch (lin_outside_pair)
            // pairs are (odd, even) whatever the batch: a sequence's results do not depend on its neighbours' lengths
            for (int d = (B.nmax - 2) | 1; d >= 0; d -= 2) {
                for (int r = d; r >= d - 1 && r >= 0; r--)   // block products whose tiles start on either diagonal of the pair
                    if ((r + 1) % BS == 0) {
                        const int D = (r + 1) / BS - 1;
                        if (D >= 0 && D <= last_block) { c->n_launch[1] += far_outside_step(c, B, c->s_mc, D, last_block); c->n_far[1]++; }
                    }
                const int ncol = B.nmax - 1 - d + 1;          // columns of the longer diagonal d-1 (d = 0: diagonal 0 alone, one less)
                const int groups = std::max(1, (ncol - 1 + 62) / 63) + 1;
                KLAUNCH(c, 2, (lin_outside_pair<W, BS>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64 * W), c->s_mc, B, c->lin->d, d,
                        d, pin, bad);
                c->n_launch[1]++;
            }
            if (finish) hipLaunchKernelGGL(lin_finish, dim3((BR.ns + 63) / 64), dim3(64), 0, c->s_mc, BR, c->lin->d, c->d_mclogz.as<double>(), bad);
            if (finish) hipLaunchKernelGGL(mc_unpaired, dim3((BR.nmax + 63) / 64, BR.ns), dim3(256), 0, c->s_mc, BR);
            return RH_OK;
        }
    }
    for (int d = B.nmax - 2; d >= 0; d--) {
        if (BS > 0 && (d + 1) % BS == 0) {
            const int D = (d + 1) / BS - 1;
            if (D >= 0 && D <= last_block) {
                if (BS == 16 && c->far_mfma) c->n_launch[1] += far_outside_step(c, B, c->s_mc, D, last_block);
                else {
                    KLAUNCH(c, 3, lin_far_outside<(BS > 0 ? BS : 16)>, dim3(last_block - D + 1, B.ns, 2), dim3(256), c->s_mc, B, D);
                    c->n_launch[1]++;
                }
                c->n_far[1]++;
            }
        }
        const int groups = (B.nmax - 1 - d + 63) / 64 + 1;
        KLAUNCH(c, 2, (lin_outside_diag<W, BS>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64 * W), c->s_mc, B,
                           c->lin->d, d, pin, bad);
        c->n_launch[1]++;
    }
    if (finish) hipLaunchKernelGGL(lin_finish, dim3((BR.ns + 63) / 64), dim3(64), 0, c->s_mc, BR, c->lin->d, c->d_mclogz.as<double>(), bad);
    if (finish) hipLaunchKernelGGL(mc_unpaired, dim3((BR.nmax + 63) / 64, BR.ns), dim3(256), 0, c->s_mc, BR);
    return RH_OK;
}


// Which sequences run where is decided per sequence, by its length alone: 8..109 letters by their own workgroup when RH_SMALL=1
// (mccaskill_small.hip), fewer than kStripMinN letters next to longer ones in a pass of their own (the organisation they would get
// alone), everyone else in the sweeps.  Sub-batches of the scale ladder (c->mc.n is not the upload's length array) run as they are.
template <int W, int BS>
int launch_mc_lin(rh_ctx* c, int pin, int phase)
{
    const McBatch BR = c->mc;
    const bool routed = (const void*)BR.n == c->d_n.p && (!c->small_list.empty() || c->n_short > 0);
    if (!routed) return launch_mc_lin_body<W, BS>(c, pin, phase, BR, BR, true, true);
    int* bad = c->d_bad.as<int>();
    McBatch BL = BR, BSH = BR;
    BL.n = c->d_n_sweep.as<const int>(); BL.nmax = c->nmax_sweep;
    BSH.n = c->d_n_short.as<const int>(); BSH.nmax = c->nmax_short;
    int rc;
    if (phase == 0) {
        hipLaunchKernelGGL(lin_init, dim3((BR.ns + 63) / 64), dim3(64), 0, c->s_mc, BR, c->lin->d, bad);
        if (!c->small_list.empty()) {
            launch_lin_small(BR, c->lin->d, c->lin->wT + kStripFiltOff + kStripFiltLen, c->d_small_list.as<const int>(), (int)c->small_list.size(), bad, c->s_mc);
            c->n_launch[0]++;
        }
        if (BL.nmax > 0 && (rc = launch_mc_lin_body<W, BS>(c, pin, 0, BL, BR, false, false))) return rc;
        if (c->n_short > 0 && (rc = launch_mc_lin_body<W, BS>(c, pin, 0, BSH, BR, false, false))) return rc;
        return RH_OK;
    }
    if (BL.nmax > 0 && (rc = launch_mc_lin_body<W, BS>(c, pin, 1, BL, BR, false, false))) return rc;
    if (c->n_short > 0 && (rc = launch_mc_lin_body<W, BS>(c, pin, 1, BSH, BR, false, false))) return rc;
    hipLaunchKernelGGL(lin_finish, dim3((BR.ns + 63) / 64), dim3(64), 0, c->s_mc, BR, c->lin->d, c->d_mclogz.as<double>(), bad);
    hipLaunchKernelGGL(mc_unpaired, dim3((BR.nmax + 63) / 64, BR.ns), dim3(256), 0, c->s_mc, BR);
    return RH_OK;
}

template <int BS>
int launch_mc_lin_w(rh_ctx* c, int pin, int phase)
{
    switch (phase == 0 ? c->lin_w_in : c->lin_w) {
        case 16: return launch_mc_lin<16, BS>(c, pin, phase);
        case 4: if (BS == 16) return launch_mc_lin<4, 16>(c, pin, phase); else return launch_mc_lin<8, BS>(c, pin, phase);
        default: return launch_mc_lin<8, BS>(c, pin, phase);
    }
}
int launch_mc_lin_any(rh_ctx* c, int pin, int phase)
{
    switch (c->lin_bs) {
        case 0: return launch_mc_lin_w<0>(c, pin, phase);
        case 32: return launch_mc_lin_w<32>(c, pin, phase);
        default: return launch_mc_lin_w<16>(c, pin, phase);
    }
}

// single-branch weights of the strip kernels: wT[l1*40 + t+1] = shape_w(l1, t-l1), zero where the shape does not exist (the dense
// filter, FILT = 0), followed by the FACTORED form of the same weights at offset kStripFiltOff (FILT = 1, mccaskill_strip.hip):
// cache_score_single[l1][l2] (InferenceEngine.ipp:1161-1197) of an interior loop is length term(l1+l2) + asymmetry term(|l1-l2|)
// plus corrections on a sparse set (bulges l1 = 0 | l2 = 0, the symmetric term on l1 == l2, the explicit terms for l1, l2 <= 4), so
//   w(l1, t-l1) = A(t) * B(|2 l1 - t|) + R(l1, t),   R != 0 only for bulge ends, the centre tap and a few (l1, l2 <= 4) shapes,
// and the B-weighted row sums obey S_{t+2}[i-1] = S_t[i] + B(t) (x[i+1] + x[i+t+1]): two diagonals later the same table row needs
// two more taps instead of a whole pass.  A, B (any gauge) and R are taken from the weights themselves and the reconstruction is
// verified entry by entry; a weight set without this structure keeps the dense filter (`*ok` = false).
//   F[0..159]   W4[t+1][4] = {A(t), bulge weight wb(t), Bstep(t), centre residual Rc(t)}, t = -1..38 (zero outside 0..30)
//   F[160..191] Bp[parity][j] = B(parity + 2j)
//   F[192..231] Rx[t][l1-1], t = 0..9, l1 = 1..4: residuals of the shapes with 1 <= l1 <= 4 that are neither bulge end nor centre
std::vector<double> strip_weights(const LinModel& L, bool* ok_out)
{
    std::vector<double> wT(kStripFiltOff + kStripFiltLen + kSmallWLen, 0.0);
    for (int t = 0; t <= kMaxSingle; t++)   // zero-padded rows for mccaskill_small.hip
        for (int l1 = 0; l1 <= t; l1++) wT[kStripFiltOff + kStripFiltLen + t * 32 + l1] = L.shape_w[t * (t + 1) / 2 + l1];
    double W[31][31] = {};
    for (int t = 0; t <= kMaxSingle; t++)
        for (int l1 = 0; l1 <= t; l1++) { W[t][l1] = L.shape_w[t * (t + 1) / 2 + l1]; wT[(size_t)l1 * 40 + t + 1] = W[t][l1]; }
    double* F = wT.data() + kStripFiltOff;
    double B[40] = {}, A[40] = {};
    bool ok = W[30][14] > 0.0 && W[29][14] > 0.0;
    if (ok) {
        for (int k = 2; k <= 28; k += 2) B[k] = W[30][15 - k / 2] / W[30][14];     // gauge B(2) = 1 on the even, B(1) = 1 on the odd differences
        B[0] = B[2];                                                                  // (the centre tap carries the symmetric term: residual)
        for (int k = 1; k <= 27; k += 2) B[k] = W[29][(29 - k) / 2] / W[29][14];
        for (int t = 3; t <= 30; t++) A[t] = B[t - 2] > 0.0 ? W[t][1] / B[t - 2] : 0.0;
    }
    for (int t = 0; ok && t <= 30; t++) {
        for (int l1 = 0; l1 <= t; l1++) {
            const int l2 = t - l1;
            const double ab = (l1 >= 1 && l2 >= 1) ? A[t] * B[std::abs(l1 - l2)] : 0.0;
            double R = W[t][l1] - ab;
            if (std::fabs(R) <= 1e-13 * std::fabs(W[t][l1])) R = 0.0;
            if (R == 0.0) continue;
            if (l1 == 0 || l2 == 0) { if (W[t][0] != W[t][t]) ok = false; F[(t + 1) * 4 + 1] = W[t][0]; }   // one bulge weight per length
            else if (l1 == l2) F[(t + 1) * 4 + 3] = R;
            else if (l1 <= 4 && l2 <= 4) F[192 + t * 4 + (l1 - 1)] = R;                                      // (t <= 8)
            else ok = false;
        }
        F[(t + 1) * 4 + 0] = A[t];
        F[(t + 1) * 4 + 2] = t == 0 ? 0.5 * B[0] : (t <= 28 ? B[t] : 0.0);
    }
    for (int j = 0; j < 16; j++) { F[160 + j] = 2 * j <= 28 ? B[2 * j] : 0.0; F[176 + j] = 2 * j + 1 <= 27 ? B[2 * j + 1] : 0.0; }
    // verification: the factored form reproduces every weight
    for (int t = 0; ok && t <= 30; t++)
        for (int l1 = 0; l1 <= t; l1++) {
            const int l2 = t - l1;
            double w = (l1 >= 1 && l2 >= 1) ? A[t] * B[std::abs(l1 - l2)] : 0.0;
            if (l1 == 0 || l2 == 0) w += t >= 1 ? F[(t + 1) * 4 + 1] : 0.0;
            else if (l1 == l2) w += F[(t + 1) * 4 + 3];
            else if (l1 <= 4 && l2 <= 4) w += F[192 + t * 4 + (l1 - 1)];
            if (std::fabs(w - W[t][l1]) > 1e-12 * std::fabs(W[t][l1])) ok = false;
        }
    if (ok && (F[(0 + 1) * 4 + 1] != 0.0 || F[(1 + 1) * 4 + 1] != 0.0)) ok = false;   // shapes (0,0), (0,1), (1,0) are not filter taps (weight 0 here)
    if (ok_out) *ok_out = ok;
    return wT;
}

}  // namespace rh::host
