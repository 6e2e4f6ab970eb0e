// launch_vienna.hip -- launch sequences of the Vienna-BL model: log-space sweeps + accessibility, the scaled linear
// sweeps (single-molecule and s1+s2 batches), the two-molecule ensemble in log space, and the scale-exponent models.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "kernels.h"

namespace rh::host {

// ---- McCaskill sweeps + accessibility, Vienna-BL model (log space; mccaskill_vienna.hip)
int launch_mc_vienna(rh_ctx* c, int pin)
{
    const McBatch& B = c->mc;
    hipLaunchKernelGGL(mcv_init, dim3((B.ns + 63) / 64), dim3(64), 0, c->s_mc, B);
    for (int d = 0; d <= B.nmax - 1; d++) {
        const int waves = std::max(B.nmax - 1 - d, 0) + 1;
        KLAUNCH(c, 0, mcv_inside_diag, pin ? dim3(B.ns, (waves + 3) / 4) : dim3((waves + 3) / 4, B.ns), dim3(256), c->s_mc, B, c->d_vienna, d, pin);
        c->n_launch[0]++;
    }
    HIP_TRY(c, hipEventRecord(c->ev[1], c->s_mc));
    for (int d = B.nmax - 2; d >= 0; d--) {
        const int waves = (B.nmax - 1 - d) + 1;
        KLAUNCH(c, 2, mcv_outside_diag, pin ? dim3(B.ns, (waves + 3) / 4) : dim3((waves + 3) / 4, B.ns), dim3(256), c->s_mc, B, c->d_vienna, d, pin);
        c->n_launch[1]++;
    }
    hipLaunchKernelGGL(mcv_finish, dim3((B.ns + 63) / 64), dim3(64), 0, c->s_mc, B, c->d_mclogz.as<double>());
    // accessibility P(i..i+w unpaired), w < max_w, from the finished tables
    const int tiles = (B.ld + 31) / 32;
    hipLaunchKernelGGL(mcv_acc_prep, dim3(tiles * tiles, B.ns, 3), dim3(256), 0, c->s_mc, B, c->d_vienna);
    hipLaunchKernelGGL(mcv_acc_hscan, dim3((B.nmax + 1 + 255) / 256, B.ns), dim3(256), 0, c->s_mc, B, 1 /* VM_FCX */);
    hipLaunchKernelGGL(mcv_acc_gaps, dim3((B.nmax * 30 + 3) / 4, B.ns, 2), dim3(256), 0, c->s_mc, B, c->d_vienna, c->d_gaps.as<double>());
    hipLaunchKernelGGL(mcv_acc_final, dim3((B.nmax + 3) / 4, B.ns), dim3(256), 0, c->s_mc, B, c->d_vienna, c->d_gaps.as<const double>(), c->max_w);
    c->n_launch[1] += 4;
    return RH_OK;
}

// ---- Vienna-BL McCaskill sweeps, scaled linear-space path (mccaskill_vlin.hip) with the block products of mccaskill_far.hip.
// co = false: the single-molecule batch on the McCaskill stream (+ accessibility); co = true: the s1+s2 batch of the
// two-molecule hybridization matrix on the duplex stream (two more groups per launch for the exterior halves XS / XP)
template <int BS>
int launch_mc_vlin_bs(rh_ctx* c, int pin, int phase, bool co)
{
    constexpr int W = 8;
    const McBatch& B = co ? c->co : c->mc;
    hipStream_t st = co ? c->s_dx : c->s_mc;
    int* bad = (int*)(co ? c->d_cobad.p : c->d_bad.p);
    int* nl = co ? &c->n_launch[2] : (phase == 0 ? &c->n_launch[0] : &c->n_launch[1]);
    int* nf = co ? &c->n_far[2] : (phase == 0 ? &c->n_far[0] : &c->n_far[1]);
    const int extra = co ? 3 : 1;   // F5 (+ XP, XS)
    const int last_block = BS > 0 ? (B.nmax - 1) / BS : 0;
    // two-molecule sweeps: the groups of diagonal dd with a cell on both strands are 1 + 64 slot <= cut < 1 + 64 slot + 64 + dd; the
    // union over the batch's cuts is launched behind the three F5 / XP / XS groups (window_slot_vl); cells = all cell groups of the launch
    const bool window = co && c->co_window && c->co_cut_min >= 1;
    const auto windowed = [&](int dd, int cells, int* pin_arg) -> int {
        const int t = c->co_cut_min - 65 - dd;
        const int lo = std::max(0, (t >= 0 ? t / 64 : -((-t + 63) / 64)) + 1), hi = std::min(cells - 1, (c->co_cut_max - 1) / 64);
        *pin_arg = pin | 128 | (lo << 8);
        return 3 + std::max(0, hi - lo + 1);
    };
    if (phase == 0) {
        hipLaunchKernelGGL(vlin_init, dim3((B.ns + 63) / 64), dim3(64), 0, st, B, bad);
        if (co && B.seeded) hipLaunchKernelGGL(vlin_co_seed, dim3(c->mc.nmax, B.ns), dim3(256), 0, st, B, c->mc);
        for (int d = 0; d <= B.nmax - 1; d++) {
            const int cells = (std::max(B.nmax - 1 - d, 0) + 63) / 64;
            const bool la1 = BS == 16 && c->lookahead && (d & 1) == 0;   // this launch also feeds diagonal d+1
            int pin_k = pin;
            const int groups = (window && B.seeded) ? windowed(la1 ? d + 1 : d, cells, &pin_k) : cells + extra;
            const double hp_d = c->h_hplen[d];
            const dim3 grid = pin ? dim3(B.ns, groups) : dim3(groups, B.ns);
            bool done = false;
            if constexpr (BS == 16) {
                if (c->lookahead) {   // look-ahead pairs: even diagonal = full launch that also accumulates d+1's sums, odd = one wavefront per group
                    done = true;
                    if ((d & 1) == 0) {
                        if (co) KLAUNCH(c, 0, (vlin_inside_diag<W, 16, true, 1>), grid, dim3(64 * W), st, B, c->d_vlin, d, hp_d, pin_k);
                        else KLAUNCH(c, 0, (vlin_inside_diag<W, 16, false, 1>), grid, dim3(64 * W), st, B, c->d_vlin, d, hp_d, pin);
                    } else {
                        if (co) KLAUNCH(c, 0, (vlin_inside_diag<W, 16, true, 2>), grid, dim3(64), st, B, c->d_vlin, d, hp_d, pin_k);
                        else KLAUNCH(c, 0, (vlin_inside_diag<W, 16, false, 2>), grid, dim3(64), st, B, c->d_vlin, d, hp_d, pin);
                    }
                }
            }
            if (!done) {
                if (co) KLAUNCH(c, 0, (vlin_inside_diag<W, BS, true, 0>), grid, dim3(64 * W), st, B, c->d_vlin, d, hp_d, pin_k);
                else KLAUNCH(c, 0, (vlin_inside_diag<W, BS, false, 0>), grid, dim3(64 * W), st, B, c->d_vlin, d, hp_d, pin);
            }
            (*nl)++;
            if (BS > 0 && (d + 1) % BS == 0) {
                const int D = (d + 1) / BS + 1;
                if (D >= 4 && D <= last_block) { (*nl) += far_inside_step(c, B, st, D, last_block); (*nf)++; }
            }
        }
        return RH_OK;
    }
    if (BS > 0) {
        (*nl) += far_outside_begin(c, B, st, last_block);
        for (int D = last_block; D >= 0 && (D + 1) * BS - 1 > B.nmax - 2; D--) { (*nl) += far_outside_step(c, B, st, D, last_block); (*nf)++; }
    }
    const bool la = BS == 16 && c->lookahead;   // look-ahead pairs (odd diagonal: full launch + the sums of the next, even: one wavefront per group)
    for (int d = la ? ((B.nmax - 2) | 1) : B.nmax - 2; d >= 0; d--) {
        if (BS > 0 && (d + 1) % BS == 0 && d <= B.nmax - 2) {
            const int D = (d + 1) / BS - 1;
            if (D >= 0 && D <= last_block) { (*nl) += far_outside_step(c, B, st, D, last_block); (*nf)++; }
        }
        bool done = false;
        if constexpr (BS == 16) {
            if (la) {
                done = true;
                int pin_k = pin;
                if (d & 1) {
                    const int cells = (B.nmax - d + 63) / 64;   // cells of diagonal d-1
                    const int groups = window ? windowed(d, cells, &pin_k) : cells + extra;
                    const dim3 grid = pin ? dim3(B.ns, groups) : dim3(groups, B.ns);
                    if (co) KLAUNCH(c, 2, (vlin_outside_diag<W, 16, true, 1>), grid, dim3(64 * W), st, B, c->d_vlin, d, pin_k, bad);
                    else KLAUNCH(c, 2, (vlin_outside_diag<W, 16, false, 1>), grid, dim3(64 * W), st, B, c->d_vlin, d, pin, bad);
                } else {
                    const int cells = (B.nmax - 1 - d + 63) / 64;
                    const int groups = window ? windowed(d, cells, &pin_k) : cells + extra;
                    const dim3 grid = pin ? dim3(B.ns, groups) : dim3(groups, B.ns);
                    if (co) KLAUNCH(c, 2, (vlin_outside_diag<W, 16, true, 2>), grid, dim3(64), st, B, c->d_vlin, d, pin_k, bad);
                    else KLAUNCH(c, 2, (vlin_outside_diag<W, 16, false, 2>), grid, dim3(64), st, B, c->d_vlin, d, pin, bad);
                }
            }
        }
        if (!done) {
            const int cells = (B.nmax - 1 - d + 63) / 64;
            int pin_k = pin;
            const int groups = window ? windowed(d, cells, &pin_k) : cells + extra;
            if (co) KLAUNCH(c, 2, (vlin_outside_diag<W, BS, true, 0>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64 * W), st, B, c->d_vlin, d, pin_k, bad);
            else KLAUNCH(c, 2, (vlin_outside_diag<W, BS, false, 0>), pin ? dim3(B.ns, groups) : dim3(groups, B.ns), dim3(64 * W), st, B, c->d_vlin, d, pin, bad);
        }
        (*nl)++;
    }
    if (co) {
        const DxBatch& D = c->dx;
        hipLaunchKernelGGL(mcv_extract_hp, dim3((D.n1max * D.n2max + 255) / 256, B.ns), dim3(256), 0, st, B, D.hp, D.tab_stride, D.ldd, D.logz,
                           c->h_vlin->s, bad);
        return RH_OK;
    }
    hipLaunchKernelGGL(vlin_finish, dim3((B.ns + 63) / 64), dim3(64), 0, st, B, c->d_vlin, c->d_mclogz.as<double>(), bad);
    // accessibility P(i..i+w unpaired), w < max_w
    const int tiles = (B.ld + 31) / 32;
    hipLaunchKernelGGL(vlin_acc_prep, dim3(tiles * tiles, B.ns), dim3(256), 0, st, B, c->d_vlin, c->d_hplen.as<const double>());
    hipLaunchKernelGGL(mcv_acc_hscan, dim3((B.nmax + 1 + 255) / 256, B.ns), dim3(256), 0, st, B, 10 /* VL_FM2F */);
    hipLaunchKernelGGL(vlin_acc_hsum, dim3((B.nmax + 3) / 4, B.ns), dim3(256), 0, st, B, c->max_w);
    if (c->acc_wide && (size_t)kViennaMcTables * B.tab_stride * sizeof(double) < ((size_t)1 << 32)) {   // (vlin_acc_gaps_wide addresses a sequence's tables with 32-bit offsets)
        // gap lengths 1, 2 (the tabulated shapes: six times the loads of a generic length): one thread per letter and length, the inner
        // spans in 8 chunks; 3..30: the lanes over the gap length (vlin_acc_gaps_wide)
        constexpr int NG = 2, NCH = 8;
        double* part = c->d_gaps.as<double>() + (size_t)2 * 32 * B.ld * B.ns;
        // (one wavefront per workgroup: the loop runs to the longest inner span of the workgroup's letters, which differ by the block width)
        hipLaunchKernelGGL(vlin_acc_gaps, dim3((B.nmax + 63) / 64, B.ns, 2 * NG * NCH), dim3(64), 0, st, B, c->d_vlin, c->d_gaps.as<double>(), NG, NCH, part);
        hipLaunchKernelGGL(vlin_acc_gsum, dim3((B.nmax + 255) / 256, B.ns, 2 * NG), dim3(256), 0, st, B, c->d_gaps.as<double>(), (const double*)part, NG, NCH);
        hipLaunchKernelGGL(vlin_acc_gaps_wide, dim3((B.nmax + 3) / 4, B.ns, 2), dim3(256), 0, st, B, c->d_vlin, c->d_gaps.as<double>());
    } else
        hipLaunchKernelGGL(vlin_acc_gaps, dim3((B.nmax + 255) / 256, B.ns, 60), dim3(256), 0, st, B, c->d_vlin, c->d_gaps.as<double>(), 30, 1, (double*)nullptr);
    hipLaunchKernelGGL(vlin_acc_gsuf, dim3((B.nmax + 255) / 256, B.ns, 2), dim3(256), 0, st, B, c->d_gaps.as<double>());
    if (c->acc_final_t && c->max_w <= 15)   // one thread per letter, all widths (the operands of the fifteen widths overlap)
        hipLaunchKernelGGL(vlin_acc_final_t, dim3((B.nmax + 255) / 256, B.ns), dim3(256), 0, st, B, c->d_vlin, c->d_gaps.as<const double>(), c->max_w);
    else
        hipLaunchKernelGGL(vlin_acc_final, dim3((B.nmax + 255) / 256, B.ns, c->max_w), dim3(256), 0, st, B, c->d_vlin, c->d_gaps.as<const double>(), c->max_w);
    c->n_launch[1] += 6;
    return RH_OK;
}

int launch_mc_vlin(rh_ctx* c, int pin, int phase, bool co)
{
    return c->lin_bs != 0 ? launch_mc_vlin_bs<16>(c, pin, phase, co) : launch_mc_vlin_bs<0>(c, pin, phase, co);
}

// ---- hybridization matrix from the two-molecule ensemble (co_pf_fold semantics): the same sweeps over s1+s2 with a cut
int launch_cofold(rh_ctx* c)
{
    const McBatch& B = c->co;
    const DxBatch& D = c->dx;
    const int pin = B.ns % 8 == 0 ? 1 : 0;
    hipLaunchKernelGGL(mcv_init, dim3((B.ns + 63) / 64), dim3(64), 0, c->s_dx, B);
    for (int d = 0; d <= B.nmax - 1; d++) {
        const int waves = std::max(B.nmax - 1 - d, 0) + 3;   // cells, F5i, XP, XS
        KLAUNCH(c, 4, mcv_inside_diag, pin ? dim3(B.ns, (waves + 3) / 4) : dim3((waves + 3) / 4, B.ns), dim3(256), c->s_dx, B, c->d_vienna, d, pin);
        c->n_launch[2]++;
    }
    for (int d = B.nmax - 2; d >= 0; d--) {
        const int waves = (B.nmax - 1 - d) + 3;
        KLAUNCH(c, 4, mcv_outside_diag, pin ? dim3(B.ns, (waves + 3) / 4) : dim3((waves + 3) / 4, B.ns), dim3(256), c->s_dx, B, c->d_vienna, d, pin);
        c->n_launch[2]++;
    }
    hipLaunchKernelGGL(mcv_extract_hp, dim3((D.n1max * D.n2max + 255) / 256, B.ns), dim3(256), 0, c->s_dx, B, D.hp, D.tab_stride, D.ldd, D.logz,
                       -1.0, (int*)nullptr);
    return RH_OK;
}

// ---- Vienna-BL: other scale exponents before the log-space kernels.  The linear path stores Q * exp(-s * span) with s = 0.28 (random ACGU
// under the BL* energies: 0.21-0.33 per nucleotide); a 900-nt chain of stable hairpins (0.87) or a ribosomal RNA (~0.6 at 1500 nt)
// passes 1e200, and one such sequence used to send the whole batch -- single-molecule folds, accessibility and the two-molecule
// sweeps -- to the log-space kernels.  Now the batch is run again on the linear kernels with s = 0.7, then 1.8, then 0 (models built
// on first use), and goes to log space only when every exponent left some problem outside the range.  Whole batches, not problems
// (the two-molecule sweeps are seeded from the single folds of the same pass); the exponent that worked is where the next batch of at
// least eight sequences starts.  rh_last_path = 3 and rh_batch_fallbacks(which = 2) = the sequences the first attempts flagged.
const double kVRungS[Ctx::kVRungs] = {0.7, 1.8, 0.0};

int select_vlin(rh_ctx* c, int model)
{
    if (model == c->vlin_cur) return RH_OK;
    VLinSet& v = c->vlin_m[model + 1];
    if (!v.h) {
        v.h = new VLinModel;
        build_vlin_model(*c->h_vienna, kVRungS[model], v.h);
        HIP_TRY(c, v.d.upload(v.h));
    }
    c->h_vlin = v.h;
    c->d_vlin = v.d;
    c->vlin_cur = model;
    // hairpin length weights x lam^d (kernel arguments of the inside sweeps; the device copy serves the accessibility)
    const VLinModel& H = *c->h_vlin;
    for (size_t d = 0; d < c->h_hplen.size(); d++)
        c->h_hplen[d] = (d <= 30 ? H.E_hairpin[d] : std::exp(H.hairpin30 - H.lxc * std::log(d / 30.0))) * std::exp(-H.s * (double)d);
    if (c->d_hplen.p && c->has_mc) {
        HIP_TRY(c, hipMemcpyAsync(c->d_hplen.p, c->h_hplen.data(), sizeof(double) * std::min((size_t)c->mc.ld, c->h_hplen.size()), hipMemcpyHostToDevice, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    }
    return RH_OK;
}

}  // namespace rh::host
