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
    HIP_TRY(c, hipEventRecord(c->ev[kEvMcInside], c->s_mc));
    for (int d = B.nmax - 2; d >= 0; d--) {
        const int waves = (B.nmax - 1 - d) + 1;
        KLAUNCH(c, 2, mcv_outside_diag, pin ? dim3(B.ns, (waves + 3) / 4) : dim3((waves + 3) / 4, B.ns), dim3(256), c->s_mc, B, c->d_vienna, d, pin);
        c->n_launch[1]++;
    }
    hipLaunchKernelGGL(mcv_finish, dim3((B.ns + 63) / 64), dim3(64), 0, c->s_mc, B, c->d_mclogz.as<double>());
    // accessibility P(i..i+w unpaired), w < max_w, from the finished tables
    const int tiles = (B.ld + 31) / 32;
    hipLaunchKernelGGL(mcv_acc_prep, dim3(tiles * tiles, B.ns, 3), dim3(256), 0, c->s_mc, B, c->d_vienna);
    hipLaunchKernelGGL(mcv_acc_hscan, dim3((B.nmax + 1 + 255) / 256, B.ns), dim3(256), 0, c->s_mc, B, VM_FCX);
    hipLaunchKernelGGL(mcv_acc_gaps, dim3((B.nmax * 30 + 3) / 4, B.ns, 2), dim3(256), 0, c->s_mc, B, c->d_vienna, c->d_gaps.as<double>());
    hipLaunchKernelGGL(mcv_acc_final, dim3((B.nmax + 3) / 4, B.ns), dim3(256), 0, c->s_mc, B, c->d_vienna, c->d_gaps.as<const double>(), c->max_w);
    c->n_launch[1] += 4;
    return RH_OK;
}

// ---- Vienna-BL McCaskill sweeps, scaled linear-space path (mccaskill_vlin.hip) with the block products of mccaskill_far.hip.
// co = false: the single-molecule batch on the McCaskill stream (+ accessibility); co = true: the s1+s2 batch of the
// two-molecule hybridization matrix on the duplex stream (two more groups per launch for the exterior halves XS / XP)
using VInsideK = void (*)(McBatch, const VLinModel*, int, double, int);
using VOutsideK = void (*)(McBatch, const VLinModel*, int, int, int*);
// the kernels of one <W = 8, BS, CUT> by MODE (0: one launch per diagonal; 1, 2: the full and the one-wavefront launch of a
// look-ahead pair, BS = 16 only), on one line with the names reported for them
struct VlinKernels { int BS; bool cut; VInsideK in[3]; VOutsideK out[3]; const char *in_name, *out_name; };
#define VLIN_NAMES(BS, CUT) "vlin_inside_diag<8, " #BS ", " #CUT ">", "vlin_outside_diag<8, " #BS ", " #CUT ">"
#define VLIN(BS, CUT) {BS, CUT, {vlin_inside_diag<8, BS, CUT, 0>}, {vlin_outside_diag<8, BS, CUT, 0>}, VLIN_NAMES(BS, CUT)}
#define VLIN_AHEAD(BS, CUT) {BS, CUT, {vlin_inside_diag<8, BS, CUT, 0>, vlin_inside_diag<8, BS, CUT, 1>, vlin_inside_diag<8, BS, CUT, 2>}, \
                             {vlin_outside_diag<8, BS, CUT, 0>, vlin_outside_diag<8, BS, CUT, 1>, vlin_outside_diag<8, BS, CUT, 2>}, VLIN_NAMES(BS, CUT)}
const VlinKernels kVlin[] = {VLIN(0, false), VLIN(0, true), VLIN_AHEAD(16, false), VLIN_AHEAD(16, true)};
#undef VLIN_NAMES
#undef VLIN
#undef VLIN_AHEAD
static const VlinKernels& vlin_kernels(int BS, bool cut) { return row_of(kVlin, [&](const VlinKernels& r) { return r.BS == BS && r.cut == cut; }); }

SweepPlan plan_mc_vlin(const rh_ctx* c, int phase, bool co, int nmax)
{
    SweepPlan P;
    P.W = 8;
    P.BS = c->lin_bs != 0 ? 16 : 0;
    P.org = P.BS == 16 && c->lookahead ? SweepPlan::kLookahead : SweepPlan::kDiagonals;
    far_products(c, phase, nmax, true, &P);
    const VlinKernels& k = vlin_kernels(P.BS, co);
    P.fine = phase == 0 ? k.in_name : k.out_name;
    // Reported as before where the report has never named what runs (the strings are an interface of bench.py and the profiles):
    // RH_LIN_BS=32 as block size 32 and RH_FAR_MFMA=0 as the LDS products (these kernels have BS = 16 on the MFMA products only);
    // the two-molecule sweeps as one descriptive string, BS = 16 whatever RH_LIN_BS says, and without a block-product name.
    if (c->lin_bs == 32) P.fine = phase == 0 ? "vlin_inside_diag<8, 32, false>" : "vlin_outside_diag<8, 32, false>";
    if (P.BS && (c->lin_bs == 32 || !c->far_mfma)) P.far_name = far_name(SweepPlan::kFarLds, c->lin_bs == 32 ? 32 : 16, phase);
    if (co) { P.fine = "vlin_inside_diag<8, 16, true> + vlin_outside_diag<8, 16, true> (s1+s2)"; P.far_name = ""; }
    return P;
}

// The grid of one launch over `cells` groups of 64 cells: behind them F5 (+ XP, XS for the two-molecule sweeps).  window: of the
// two-molecule sweeps, only the groups of diagonal dd with a cell on both strands, 1 + 64 slot <= cut < 1 + 64 slot + 64 + dd --
// the union over the batch's cuts -- are launched, behind the three F5 / XP / XS groups (window_slot_vl); the kernel finds its
// group through the pin argument
struct VlinGrid { dim3 grid; int pin; };
static VlinGrid vlin_grid(const McVlinArgs& A, int dd, int cells)
{
    int groups = cells + (A.co ? 3 : 1), pin_k = A.pin;
    if (A.window) {
        const int t = A.cut_min - 65 - dd;
        const int lo = std::max(0, (t >= 0 ? t / 64 : -((-t + 63) / 64)) + 1), hi = std::min(cells - 1, (A.cut_max - 1) / 64);
        pin_k = A.pin | 128 | (lo << 8);
        groups = 3 + std::max(0, hi - lo + 1);
    }
    return {seq_grid(A.pin, A.B.ns, groups), pin_k};
}

// one launch per diagonal, or look-ahead pairs: the even diagonal is a full launch that also accumulates the sums of d+1, which then
// needs one wavefront per group
static void vlin_inside(const SweepPass& S, const McVlinArgs& A)
{
    rh_ctx* c = S.c;
    const McBatch& B = S.B;
    const VlinKernels& K = vlin_kernels(S.P.BS, A.co);
    const bool ahead = S.P.org == SweepPlan::kLookahead;
    hipLaunchKernelGGL(vlin_init, dim3((B.ns + 63) / 64), dim3(64), 0, S.st, B, A.bad);
    if (A.co && B.seeded) hipLaunchKernelGGL(vlin_co_seed, dim3(A.from.nmax, B.ns), dim3(256), 0, S.st, B, A.from, A.pair_seq);
    for (int d = 0; d <= B.nmax - 1; d++) {
        const int mode = !ahead ? 0 : (d & 1) ? 2 : 1;
        const int cells = (std::max(B.nmax - 1 - d, 0) + 63) / 64;
        const VlinGrid G = vlin_grid(A, mode == 1 ? d + 1 : d, cells);   // (mode 1 also feeds diagonal d+1)
        KLAUNCH(c, 0, (K.in[mode]), G.grid, dim3(mode == 2 ? 64 : 64 * S.P.W), S.st, B, A.d_vlin, d, A.hplen[d], G.pin);
        c->n_launch[S.k]++;
        far_inside_after(S, d + 1);
    }
}

// accessibility P(i..i+w unpaired), w < max_w, behind the single-molecule sweeps
static void vlin_finish_acc(rh_ctx* c, const McVlinArgs& A, hipStream_t st)
{
    const McBatch& B = A.B;
    const VLinModel* d_vlin = A.d_vlin;
    hipLaunchKernelGGL(vlin_finish, dim3((B.ns + 63) / 64), dim3(64), 0, st, B, d_vlin, A.logz, A.bad);
    const int tiles = (B.ld + 31) / 32;
    hipLaunchKernelGGL(vlin_acc_prep, dim3(tiles * tiles, B.ns), dim3(256), 0, st, B, d_vlin, A.d_hplen);
    hipLaunchKernelGGL(mcv_acc_hscan, dim3((B.nmax + 1 + 255) / 256, B.ns), dim3(256), 0, st, B, VL_FM2F);
    hipLaunchKernelGGL(vlin_acc_hsum, dim3((B.nmax + 3) / 4, B.ns), dim3(256), 0, st, B, A.max_w);
    if (A.acc_wide) {
        // gap lengths 1, 2 (the tabulated shapes: six times the loads of a generic length): one thread per letter and length, the inner
        // spans in 8 chunks; 3..30: the lanes over the gap length (vlin_acc_gaps_wide)
        constexpr int NG = 2, NCH = 8;
        double* part = A.gaps + (size_t)2 * 32 * B.ld * B.ns;
        // (one wavefront per workgroup: the loop runs to the longest inner span of the workgroup's letters, which differ by the block width)
        hipLaunchKernelGGL(vlin_acc_gaps, dim3((B.nmax + 63) / 64, B.ns, 2 * NG * NCH), dim3(64), 0, st, B, d_vlin, A.gaps, NG, NCH, part);
        hipLaunchKernelGGL(vlin_acc_gsum, dim3((B.nmax + 255) / 256, B.ns, 2 * NG), dim3(256), 0, st, B, A.gaps, (const double*)part, NG, NCH);
        hipLaunchKernelGGL(vlin_acc_gaps_wide, dim3((B.nmax + 3) / 4, B.ns, 2), dim3(256), 0, st, B, d_vlin, A.gaps);
    } else
        hipLaunchKernelGGL(vlin_acc_gaps, dim3((B.nmax + 255) / 256, B.ns, 60), dim3(256), 0, st, B, d_vlin, A.gaps, 30, 1, (double*)nullptr);
    hipLaunchKernelGGL(vlin_acc_gsuf, dim3((B.nmax + 255) / 256, B.ns, 2), dim3(256), 0, st, B, A.gaps);
    if (A.acc_final_t)   // one thread per letter, all widths (the operands of the fifteen widths overlap)
        hipLaunchKernelGGL(vlin_acc_final_t, dim3((B.nmax + 255) / 256, B.ns), dim3(256), 0, st, B, d_vlin, (const double*)A.gaps, A.max_w);
    else
        hipLaunchKernelGGL(vlin_acc_final, dim3((B.nmax + 255) / 256, B.ns, A.max_w), dim3(256), 0, st, B, d_vlin, (const double*)A.gaps, A.max_w);
    c->n_launch[1] += 6;
}

// the same from the top; look-ahead pairs: the odd diagonal is the full launch (+ the sums of the next), the even one a wavefront per group
static void vlin_outside(SweepPass& S, const McVlinArgs& A)
{
    rh_ctx* c = S.c;
    const McBatch& B = S.B;
    const VlinKernels& K = vlin_kernels(S.P.BS, A.co);
    const bool ahead = S.P.org == SweepPlan::kLookahead;
    far_outside_begin(S, B.nmax - 2);
    for (int d = ahead ? ((B.nmax - 2) | 1) : B.nmax - 2; d >= 0; d--) {
        if (d <= B.nmax - 2) far_outside_before(S, d);
        const int mode = !ahead ? 0 : (d & 1) ? 1 : 2;
        const int cells = mode == 1 ? (B.nmax - d + 63) / 64 : (B.nmax - 1 - d + 63) / 64;   // (mode 1: the cells of diagonal d-1)
        const VlinGrid G = vlin_grid(A, d, cells);
        KLAUNCH(c, 2, (K.out[mode]), G.grid, dim3(mode == 2 ? 64 : 64 * S.P.W), S.st, B, A.d_vlin, d, G.pin, A.bad);
        c->n_launch[S.k]++;
    }
    if (A.co)
        hipLaunchKernelGGL(mcv_extract_hp, dim3((A.n1max * A.n2max + 255) / 256, B.ns), dim3(256), 0, S.st, B, A.hp, A.hp_stride, A.hp_ldd, A.hp_logz,
                           A.h_vlin->s, A.bad);
    else
        vlin_finish_acc(c, A, S.st);
}

int launch_mc_vlin(rh_ctx* c, const McVlinArgs& A)
{
    SweepPass S{c, A.plan, A.B, A.co ? c->s_dx : c->s_mc, A.co ? 2 : A.phase};
    if (A.phase == 0) vlin_inside(S, A);
    else vlin_outside(S, A);
    return RH_OK;
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
    hairpin_length_weights(*c->h_vlin, (int)c->h_hplen.size(), c->h_hplen.data());
    if (c->d_hplen.p && c->has_mc) {
        HIP_TRY(c, hipMemcpyAsync(c->d_hplen.p, c->h_hplen.data(), sizeof(double) * std::min((size_t)c->mc.ld, c->h_hplen.size()), hipMemcpyHostToDevice, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    }
    return RH_OK;
}

}  // namespace rh::host
