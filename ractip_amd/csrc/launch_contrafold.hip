// launch_contrafold.hip -- launch sequences of the CONTRAfold-model McCaskill sweeps: the log-space path, the scaled
// linear path with its block products, strips and per-sequence routing, and the strip kernels' weight tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "f5_stage.h"
#include "kernels.h"
#include "pk_layout.h"

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
    HIP_TRY(c, hipEventRecord(c->ev[kEvMcInside], c->s_mc));
    for (int d = B.nmax - 2; d >= 0; d--) {
        const int waves = (B.nmax - 1 - d) + 1;
        KLAUNCH(c, 2, mc_outside_diag, pin ? dim3(B.ns, (waves + 3) / 4) : dim3((waves + 3) / 4, B.ns), dim3(256), c->s_mc, B, c->d_model, d, pin);
        c->n_launch[1]++;
    }
    hipLaunchKernelGGL(log_finish, dim3((B.ns + 63) / 64), dim3(64), 0, c->s_mc, B, logz_out);
    hipLaunchKernelGGL(mc_unpaired, dim3((B.nmax + 63) / 64, B.ns), dim3(256), 0, c->s_mc, B, c->max_w);
    return RH_OK;
}

// ---- region accessibility, widths 2..max_w (rh_set_region_accessibility; mccaskill_acc.hip): behind the outside sweep of the
// sequences B, on the tables that sweep left -- the scaled linear ones at the exponent of `lin`, or (lin == nullptr) the log-space
// ones -- and before anything else writes them.  Column 0 of up is mc_unpaired's.  Launched from the host, outside the captured
// graphs: the scratch is allocated here, and `timed` brackets the kernels with the event pair rh_batch_acc_time reads.
template <int PATH>
static void acc_kernels(const McBatch& B, const AccArgs& A, hipStream_t st)
{
    const int n = B.nmax, ns = B.ns, w = A.max_w;
    hipLaunchKernelGGL(cf_acc_hrows<PATH>, dim3((n + 255) / 256, ns), dim3(256), 0, st, B, A);
    hipLaunchKernelGGL(cf_acc_hcols<PATH>, dim3((n + 255) / 256, ns), dim3(256), 0, st, B, A);
    hipLaunchKernelGGL(cf_acc_gaps<PATH>, dim3((n + 127) / 128, 2 * kMaxSingle, ns), dim3(128), 0, st, B, A);
    hipLaunchKernelGGL(cf_acc_final<PATH>, dim3((n + 127) / 128, w - 1, ns), dim3(128), 0, st, B, A);
    if (n < 5) return;   // (no multiloop, no chain)
    hipLaunchKernelGGL(cf_acc_sbuild<PATH>, dim3(ns), dim3(1024), 0, st, B, A);
    hipLaunchKernelGGL(cf_acc_seed<PATH>, dim3((n + 255) / 256, n - 1, ns), dim3(256), 0, st, B, A);   // (behind cf_acc_final: it reuses the hairpin sums' table)
    const int tiles = (n - 1) / kAccTile + 1;
    for (int j = 1; j < w; j++) {   // A_j = mu A_{j-1} S, then its term of width j + 1
        hipLaunchKernelGGL(cf_acc_link<PATH>, dim3(tiles, tiles, ns), dim3(256), 0, st, B, A, (j - 1) & 1);
        hipLaunchKernelGGL(cf_acc_close<PATH>, dim3((n + 3) / 4, ns), dim3(256), 0, st, B, A, j, j & 1);
    }
}

int launch_mc_acc(rh_ctx* c, const McBatch& B, const LinSet* lin, bool timed)
{
    if (!c->region_acc || c->model != RH_MODEL_CONTRAFOLD || c->max_w <= 1 || B.ns <= 0 || B.nmax < 1) return RH_OK;
    if (B.ns > 65535 || B.nmax > 65535) return fail(c, RH_ERR_UNSUPPORTED, "region accessibility: more than 65535 sequences (or letters) in one batch");
    if (int rc = ensure(c, c->d_acc, sizeof(double) * acc_scratch_doubles(B.ld) * B.ns, false)) return rc;
    AccArgs A{};
    A.lin = lin ? (const LinModel*)lin->d : nullptr;
    A.score = c->d_model;
    A.scratch = c->d_acc.as<double>();
    A.max_w = c->max_w;
    if (timed) {
        for (auto& e : c->acc_ev) if (!e) HIP_TRY(c, hipEventCreate(&e));
        HIP_TRY(c, hipEventRecord(c->acc_ev[0], c->s_mc));
    }
    if (lin) acc_kernels<0>(B, A, c->s_mc);
    else acc_kernels<1>(B, A, c->s_mc);
    HIP_TRY(c, hipGetLastError());
    if (timed) {
        HIP_TRY(c, hipEventRecord(c->acc_ev[1], c->s_mc));
        c->acc_timed = true;
    }
    return RH_OK;
}

// ---- the kernels of the scaled linear sweeps, each on one line with the name rh_batch_kernels reports for it: plan_mc_lin takes
// the name and the schedules take the kernel from the same row
using InsideDiagK = void (*)(McBatch, const LinModel*, int, double, int);
struct DiagKernels { int W, BS; Named<InsideDiagK> in; Named<decltype(&lin_outside_diag<4, 16>)> out; };   // one launch per diagonal
#define DIAG(W, BS) {W, BS, NAMED(lin_inside_diag<W, BS, 0>), NAMED(lin_outside_diag<W, BS>)}
const DiagKernels kDiag[] = {DIAG(8, 0), DIAG(16, 0), DIAG(4, 16), DIAG(8, 16), DIAG(16, 16), DIAG(8, 32), DIAG(16, 32)};
const Named<InsideDiagK> kInsidePair = NAMED(lin_inside_diag<4, 16, 3>);    // two diagonals per launch
// look-ahead pairs of launches: the even diagonal also accumulates the sums of the next one, which then needs one wavefront per group
const Named<InsideDiagK> kInsideAhead[2] = {NAMED(lin_inside_diag<4, 16, 1>), NAMED(lin_inside_diag<4, 16, 2>)};
struct PairKernels { int W; Named<decltype(&lin_outside_pair<4, 16>)> out; };
const PairKernels kOutsidePair[] = {{4, NAMED(lin_outside_pair<4, 16>)}, {8, NAMED(lin_outside_pair<8, 16>)}};
struct StripKernels { int W, filt; Named<decltype(&lin_inside_strip<8, 4, 0>)> in; Named<decltype(&lin_outside_strip<8, 4, 0>)> out; };   // KD = 8 diagonals per launch
#define STRIP(W, FILT) {W, FILT, NAMED(lin_inside_strip<8, W, FILT>), NAMED(lin_outside_strip<8, W, FILT>)}
const StripKernels kStrip[] = {STRIP(4, 0), STRIP(8, 1), STRIP(8, 0)};
// block products: LDS/FMA kernels by block size, MFMA kernels on gathered and on packed operand tiles ([0] inside, [1] outside)
struct LdsKernels { int BS; Named<decltype(&lin_far_inside<16>)> in, out; };
const LdsKernels kLds[] = {{16, NAMED(lin_far_inside<16>), NAMED(lin_far_outside<16>)}, {32, NAMED(lin_far_inside<32>), NAMED(lin_far_outside<32>)}};
const Named<decltype(&lin_far_inside_mfma)> kFarGather[2] = {NAMED(lin_far_inside_mfma), NAMED(lin_far_outside_mfma)};
const Named<decltype(&lin_far_inside_pk)> kFarPacked[2] = {NAMED(lin_far_inside_pk), NAMED(lin_far_outside_pk)};      // a wavefront per tile
const Named<decltype(&lin_far_inside_pk)> kFarPacked4[2] = {NAMED(lin_far_inside_pk4), NAMED(lin_far_outside_pk4)};   // a workgroup per tile
#undef DIAG
#undef STRIP
static const DiagKernels& diag_kernels(int W, int BS) { return row_of(kDiag, [&](const DiagKernels& r) { return r.W == W && r.BS == BS; }); }
static const PairKernels& pair_kernels(int W) { return row_of(kOutsidePair, [&](const PairKernels& r) { return r.W == W; }); }
static const StripKernels& strip_kernels(int W, int filt) { return row_of(kStrip, [&](const StripKernels& r) { return r.W == W && r.filt == filt; }); }
static const LdsKernels& lds_kernels(int BS) { return row_of(kLds, [&](const LdsKernels& r) { return r.BS == BS; }); }

// ---- block products on v_mfma_f64_16x16x4_f64 (mccaskill_far.hip, BS = 16), by gather or on re-laid operand tiles: the tiles of
// block diagonal Dblk are packed once, right after their last cell is final, and then read by every product that uses them as two
// contiguous 2 KB fragments.
//   inside : far(D) uses FM1/FM tiles of block diagonals 2..D-2; block diagonal D-2 completes with fine diagonal (D-1)*16-1
//   outside: far(D) uses FM2o tiles of block diagonals >= D+2 (final before fine diagonal (D+1)*16-1) and FM1/FM tiles of
//            every block diagonal (the last two are packed when the outside phase starts)
// Each step counts as one launch: the pack launch rides with its product (bench.py adds its traffic to the product's).
// Two-level products (64x64 macro tiles under the 16x16 tile kernels) pay from 6 macro blocks per axis on (measured: n = 200, 300
// equal, n = 400 +2 %, n = 500 +4 %, n = 2000 +27 %): SweepPlan::far2_from is the length from which a SEQUENCE takes that form.
const char* far_name(SweepPlan::Far far, int BS, int phase)
{
    switch (far) {
        case SweepPlan::kFarLds: return phase == 0 ? lds_kernels(BS).in.name : lds_kernels(BS).out.name;
        case SweepPlan::kFarGather: return kFarGather[phase].name;
        case SweepPlan::kFarPacked: return kFarPacked[phase].name;
        case SweepPlan::kFarPacked4: return kFarPacked4[phase].name;
        default: return "";
    }
}
// the block-product form of a sweep with block size P->BS (mfma: on the MFMA kernels, BS = 16) and the name reported for it
void far_products(const rh_ctx* c, int phase, int nmax, bool mfma, SweepPlan* P)
{
    const int from = c->far2 >= 0 ? (c->far2 ? 1 : 0) : 384;
    P->far = P->BS == 0 ? SweepPlan::kFarNone : !mfma ? SweepPlan::kFarLds : !c->far_pk ? SweepPlan::kFarGather : c->far_wave ? SweepPlan::kFarPacked : SweepPlan::kFarPacked4;
    P->far2_from = P->packed() && from > 0 && nmax >= from ? from : 0;
    P->far_name = far_name(P->far, P->BS, phase);
}

// schedule of the block products (BS > 0) against the fine diagonals:
//   inside : far(D) right after fine diagonal (D-1)*BS-1  (its operands are final, tile (I,I+D) starts at (D-1)*BS+1)
//   outside: far(D) right before fine diagonal (D+1)*BS-1 (operands: spans >= (D+1)*BS+1, already final)
// the 16-tile products of block diagonal D on packed tiles: four tiles per workgroup (one per wavefront) or one
static void far_packed_launch(const SweepPass& S, int phase, int D, int l2)
{
    rh_ctx* c = S.c;
    const bool wave = S.P.far == SweepPlan::kFarPacked;
    const int tiles = S.last_block() - D + 1;
    const dim3 grid(wave ? (tiles + 3) / 4 : tiles, S.B.ns, phase == 0 ? 1 : 2);
    KLAUNCH(c, phase == 0 ? 1 : 3, ((wave ? kFarPacked : kFarPacked4)[phase].kern), grid, dim3(256), S.st, S.B, D, l2);
}
void far_inside_after(const SweepPass& S, int done)   // done: the fine diagonals 0 .. done-1 are final
{
    rh_ctx* c = S.c;
    const McBatch& B = S.B;
    const int D = S.P.BS ? done / S.P.BS + 1 : 0, last_block = S.last_block(), l2 = S.P.far2_from;
    if (S.P.BS == 0 || done % S.P.BS != 0 || D < 4 || D > last_block) return;
    if (S.P.far == SweepPlan::kFarLds) KLAUNCH(c, 1, (lds_kernels(S.P.BS).in.kern), dim3(last_block - D + 1, B.ns), dim3(256), S.st, B, D);
    else if (S.P.far == SweepPlan::kFarGather) KLAUNCH(c, 1, (kFarGather[0].kern), dim3(last_block - D + 1, B.ns), dim3(256), S.st, B, D);
    else {
        KLAUNCH(c, 1, lin_pack_tiles<0>, dim3(pk_run_groups(B.nb - (D - 2)), B.ns, 2), dim3(256), S.st, B, D - 2, 0, (int)S.P.banded);
        if (l2 && (D + 3) % 4 == 0) {   // D = 4*D2-3: every operand tile of macro block diagonal D2 is packed now
            const int D2 = (D + 3) / 4, last2 = (B.nmax - 1) / 64;
            if (D2 >= 4 && D2 <= last2) KLAUNCH(c, 1, lin_far2_inside, dim3(last2 - D2 + 1, B.ns), dim3(256), S.st, B, D2, l2);
        }
        far_packed_launch(S, 0, D, l2);
    }
    c->n_launch[S.k]++;
    c->n_far[S.k]++;
}
void far_outside_before(SweepPass& S, int d)
{
    rh_ctx* c = S.c;
    const McBatch& B = S.B;
    const int D = S.P.BS ? (d + 1) / S.P.BS - 1 : 0, last_block = S.last_block(), l2 = S.P.far2_from;
    if (S.P.BS == 0 || (d + 1) % S.P.BS != 0 || D < 0 || D > last_block) return;
    if (S.P.far == SweepPlan::kFarLds) KLAUNCH(c, 3, (lds_kernels(S.P.BS).out.kern), dim3(last_block - D + 1, B.ns, 2), dim3(256), S.st, B, D);
    else if (S.P.far == SweepPlan::kFarGather) KLAUNCH(c, 3, (kFarGather[1].kern), dim3(last_block - D + 1, B.ns, 2), dim3(256), S.st, B, D);
    else {
        if (D + 2 <= last_block) KLAUNCH(c, 3, lin_pack_tiles<1>, dim3(pk_run_groups(B.nb - (D + 2)), B.ns, 1), dim3(256), S.st, B, D + 2, 1, 0);
        if (l2) {   // macro block diagonal D2 holds tile block diagonals 4*D2-3 .. 4*D2+3: its products go first, their FM2o tiles (block diagonals >= 4*D2+5) are packed
            const int last2 = (B.nmax - 1) / 64;
            for (; S.far2_next >= 0 && 4 * S.far2_next + 3 >= D; S.far2_next--)
                KLAUNCH(c, 3, lin_far2_outside, dim3(last2 - S.far2_next + 1, B.ns, 2), dim3(256), S.st, B, S.far2_next, l2);
        }
        far_packed_launch(S, 1, D, l2);
    }
    c->n_launch[S.k]++;
    c->n_far[S.k]++;
}
// start of the outside sweep at fine diagonal `top`: the last operand tiles are packed, and the tiles whose first cell would come
// before `top` get their (empty) far sums
void far_outside_begin(SweepPass& S, int top)
{
    if (S.P.BS == 0) return;
    rh_ctx* c = S.c;
    const McBatch& B = S.B;
    const int last_block = S.last_block(), banded = S.P.banded;
    if (S.P.packed()) {
        S.far2_next = (B.nmax - 1) / 64;   // macro block diagonals whose 64-block products are still to be launched (descending)
        if (S.P.repack2 && last_block - 1 > 2) KLAUNCH(c, 3, lin_pack_tiles<1>, dim3(pk_run_groups(B.nb - 2), B.ns, 2), dim3(256), S.st, B, 2, 0, banded);
        for (int Dblk = std::max(2, last_block - 1); Dblk <= last_block; Dblk++)
            KLAUNCH(c, 3, lin_pack_tiles<1>, dim3(pk_run_groups(B.nb - Dblk), B.ns, 2), dim3(256), S.st, B, Dblk, 0, banded);
    }
    for (int d = (last_block + 1) * S.P.BS - 1; d > top; d -= S.P.BS) far_outside_before(S, d);
}

// ---- McCaskill sweeps, scaled linear-space path (fast; flags sequences that left the double range)
// The organisation of one sweep over sequences of up to nmax letters.  W = 4, BS = 16 has every organisation; the others one launch
// per diagonal (outside, W = 8: diagonal pairs too).  The strip kernels need the packed block products (masked tiles) and at least
// one strip behind the 32 bootstrap diagonals.
SweepPlan plan_mc_lin(const rh_ctx* c, int phase, int nmax)
{
    SweepPlan P;
    const int w = phase == 0 ? c->lin_w_in : c->lin_w;
    P.BS = c->lin_bs == 0 || c->lin_bs == 32 ? c->lin_bs : 16;
    P.W = w == 16 ? 16 : (w == 4 && P.BS == 16 ? 4 : 8);
    const bool all_orgs = P.W == 4 && P.BS == 16, strips_ok = c->far_pk && c->far_mfma && c->lin_bs == 16 && nmax >= kStripMinN;
    const bool strips_on = (c->strip & (phase == 0 ? 1 : 2)) && strips_ok, strips = all_orgs && strips_on;
    const StripKernels& strip = strip_kernels(c->strip_w, c->strip_w == 8 && c->strip_filt && c->strip_filt_ok);
    const DiagKernels& diag = diag_kernels(P.W, P.BS);
    bool mfma = P.BS == 16 && c->far_mfma;
    P.org = SweepPlan::kDiagonals;
    P.fine = phase == 0 ? diag.in.name : diag.out.name;
    if (strips) {
        P.org = SweepPlan::kStrips;
        P.W = strip.W;
        P.filt = strip.filt;
    } else if (phase == 0 && all_orgs && c->lookahead == 2) {
        P.org = SweepPlan::kPairs;
        P.fine = kInsidePair.name;
        mfma = true;   // (this schedule has the MFMA products whatever RH_FAR_MFMA says)
    } else if (phase == 0 && all_orgs && c->lookahead) {
        P.org = SweepPlan::kLookahead;
        P.fine = kInsideAhead[0].name;
    } else if (phase == 1 && mfma && (P.W == 4 || P.W == 8) && c->lookahead == 2) {
        P.org = SweepPlan::kPairs;
        P.fine = pair_kernels(P.W).out.name;
    }
    far_products(c, phase, nmax, mfma, &P);
    // packed tiles of block diagonal 2: masked for the strips' banded near/far split, plain otherwise; the outside sweep packs them
    // again when the inside sweep left the other form.  (What the inside sweep left is judged with THIS sweep's W, as it always has
    // been: right unless RH_LIN_W_IN differs from RH_LIN_W while both strip bits are set.)
    P.banded = strips;
    P.repack2 = phase == 1 && strips != (all_orgs && (c->strip & 1) && strips_ok);
    // The strip kernels are reported whenever the strip switches hold: also for W != 4, which runs one launch per diagonal.  With
    // RH_FAR_MFMA=0 the inside sweep is reported as one launch per diagonal with the LDS products; it runs diagonal pairs with the
    // MFMA products.  (Kept: the strings are an interface of bench.py and the profiles.)
    if (strips_on) P.fine = phase == 0 ? strip.in.name : strip.out.name;
    if (phase == 0 && P.org == SweepPlan::kPairs && !c->far_mfma) { P.fine = diag.in.name; P.far_name = far_name(SweepPlan::kFarLds, 16, 0); }
    return P;
}

// ---- the schedules: one function per organisation and sweep, over the sequences B shows (lengths 0 hide a sequence)
// two diagonals per launch (lin_inside_diag MODE 3 has W = 4: 256 threads) up to diagonal `last`, pairs start even; the last launch
// may hold only F5i[nmax]
static void inside_pairs(const SweepPass& S, const McLinArgs& A, int last)
{
    for (int d = 0; d <= last; d += 2) {
        const int groups = (std::max(S.B.nmax - 1 - d, 0) + 62) / 63 + 1;
        KLAUNCH(S.c, 0, (kInsidePair.kern), seq_grid(A.pin, S.B.ns, groups), dim3(256), S.st, S.B, A.lin->d, d, std::exp(-A.lin->h.s * d), A.pin);
        S.c->n_launch[0]++;
        far_inside_after(S, d + 2);   // (the first one is due behind diagonal 47)
    }
}
// dynamic LDS of the exterior-sum passes (mccaskill_strip.hip): F5 and the partial sums, outside also the parked operands, and the
// chunk buffer of staged FCA rows, which shrinks where the rest leaves less than kF5StageRows rows of 64 KB (f5_stage.h)
size_t f5_pass_lds(int ld, int phase) { return sizeof(double) * (size_t)f5_lds_doubles(ld, phase); }
bool f5_pass_fits(int ld) { return f5_stage_rows(ld, 1) >= kF5StageRowsMin; }

// diagonals 0..31 by pairs (every row is "near" there), then strips of KD diagonals (mccaskill_strip.hip); the bootstrap leaves
// F5i[0..31], the rest is one pass behind the last strip (no inside cell reads F5i).  A.f5_pass = 0: the serial kernel instead.
static void inside_strips(const SweepPass& S, const McLinArgs& A)
{
    rh_ctx* c = S.c;
    const McBatch& B = S.B;
    constexpr int KD = 8, GS = 64 - (KD - 1);
    const auto strip = strip_kernels(S.P.W, S.P.filt).in.kern;
    inside_pairs(S, A, 30);
    for (int d0 = 32; d0 <= B.nmax - 2; d0 += KD) {
        const int groups = (B.nmax - 1 - d0 + GS - 1) / GS;
        KLAUNCH(c, 0, strip, seq_grid(A.pin, B.ns, groups), dim3(64 * S.P.W), S.st, B, A.lin->d, A.lin->wT, d0, std::exp(-A.lin->h.s * d0),
                (A.pin && A.strip_xcd) ? 2 : A.pin);
        c->n_launch[0]++;
        far_inside_after(S, d0 + KD);
    }
    if (A.f5_pass) hipLaunchKernelGGL(lin_f5i_pass, dim3(B.ns), dim3(256), f5_pass_lds(B.ld, 0), S.st, B, A.lin->d, A.f5_jlo);
    else hipLaunchKernelGGL(lin_f5i_tail, dim3(B.ns), dim3(256), 0, S.st, B, A.lin->d, A.f5_jlo);
}
// one launch per diagonal, or (ahead) look-ahead pairs of launches
static void inside_diagonals(const SweepPass& S, const McLinArgs& A, bool ahead)
{
    const InsideDiagK full = diag_kernels(S.P.W, S.P.BS).in.kern;
    for (int d = 0; d <= S.B.nmax - 1; d++) {
        const int groups = (std::max(S.B.nmax - 1 - d, 0) + 63) / 64 + 1;
        const bool odd = ahead && (d & 1);
        KLAUNCH(S.c, 0, (!ahead ? full : kInsideAhead[odd].kern), seq_grid(A.pin, S.B.ns, groups), dim3(odd ? 64 : 64 * S.P.W), S.st, S.B, A.lin->d, d,
                std::exp(-A.lin->h.s * d), A.pin);
        S.c->n_launch[0]++;
        far_inside_after(S, d + 1);
    }
}

// strips of KD diagonals from the top, aligned so that a sequence's strips do not depend on the batch.  F5o needs FCA and itself
// only, so all of it is there before the first strip: one pass, or (A.f5_pass = 0) the serial kernel over the same range.
static void outside_strips(SweepPass& S, const McLinArgs& A)
{
    rh_ctx* c = S.c;
    const McBatch& B = S.B;
    constexpr int KD = 8, GS = 64 - (KD - 1);
    const auto strip = strip_kernels(S.P.W, S.P.filt).out.kern;
    const int d0_top = (B.nmax - 2) | (KD - 1);
    far_outside_begin(S, d0_top);
    if (A.f5_pass) hipLaunchKernelGGL(lin_f5o_pass, dim3(B.ns), dim3(256), f5_pass_lds(B.ld, 1), S.st, B, A.lin->d);
    else hipLaunchKernelGGL(lin_f5o_head, dim3(B.ns), dim3(256), 0, S.st, B, A.lin->d, B.nmax - 1, 1);
    for (int d0 = d0_top; d0 >= KD - 1; d0 -= KD) {
        far_outside_before(S, d0);
        const int groups = (B.nmax - 1 - (d0 - (KD - 1)) + GS - 1) / GS;
        KLAUNCH(c, 2, strip, seq_grid(A.pin, B.ns, groups), dim3(64 * S.P.W), S.st, B, A.lin->d, A.lin->wT, d0, (A.pin && A.strip_xcd) ? 2 : A.pin, A.bad);
        c->n_launch[1]++;
    }
}
// two diagonals per launch (lin_outside_pair); pairs are (odd, even) whatever the batch: a sequence's results do not depend on
// its neighbours' lengths
static void outside_pairs(SweepPass& S, const McLinArgs& A)
{
    const auto pair = pair_kernels(S.P.W).out.kern;
    far_outside_begin(S, S.B.nmax - 2);
    for (int d = (S.B.nmax - 2) | 1; d >= 0; d -= 2) {
        for (int r = d; r >= d - 1 && r >= 0; r--) far_outside_before(S, r);   // block products whose tiles start on either diagonal of the pair
        const int ncol = S.B.nmax - 1 - d + 1;          // columns of the longer diagonal d-1 (d = 0: diagonal 0 alone, one less)
        const int groups = std::max(1, (ncol - 1 + 62) / 63) + 1;
        KLAUNCH(S.c, 2, pair, seq_grid(A.pin, S.B.ns, groups), dim3(64 * S.P.W), S.st, S.B, A.lin->d, d, d, A.pin, A.bad);
        S.c->n_launch[1]++;
    }
}
static void outside_diagonals(SweepPass& S, const McLinArgs& A)
{
    const auto diag = diag_kernels(S.P.W, S.P.BS).out.kern;
    far_outside_begin(S, S.B.nmax - 2);
    for (int d = S.B.nmax - 2; d >= 0; d--) {
        far_outside_before(S, d);
        const int groups = (S.B.nmax - 1 - d + 63) / 64 + 1;
        KLAUNCH(S.c, 2, diag, seq_grid(A.pin, S.B.ns, groups), dim3(64 * S.P.W), S.st, S.B, A.lin->d, d, A.pin, A.bad);
        S.c->n_launch[1]++;
    }
}

// One phase (0 inside, 1 outside) over the batch A.B.  A routed pass (the batch as uploaded) decides per sequence, by its length
// alone, what runs it: 8..109 letters their own workgroup when RH_SMALL=1 (mccaskill_small.hip), fewer than kStripMinN letters next to
// longer ones a pass of their own (the organisation they would get alone, a plan of its own), everyone else the sweeps.  Sub-batches
// of the scale ladder run as they are (not routed: see ADVICE.md).  lin_init / lin_finish / mc_unpaired see every sequence.
int launch_mc_lin(rh_ctx* c, const McLinArgs& A)
{
    const McBatch& BR = A.B;
    const int phase = A.phase;
    const auto sweep = [&](const McBatch& B, const SweepPlan& Q) {
        SweepPass S{c, Q, B, c->s_mc, phase};
        if (Q.org == SweepPlan::kStrips) return phase == 0 ? inside_strips(S, A) : outside_strips(S, A);
        if (Q.org == SweepPlan::kPairs) return phase == 0 ? inside_pairs(S, A, B.nmax) : outside_pairs(S, A);
        return phase == 0 ? inside_diagonals(S, A, Q.org == SweepPlan::kLookahead) : outside_diagonals(S, A);
    };
    if (phase == 0) {
        hipLaunchKernelGGL(lin_init, dim3((BR.ns + 63) / 64), dim3(64), 0, c->s_mc, BR, A.lin->d, A.bad);
        if (A.routed && A.n_small > 0) {
            launch_lin_small(BR, A.lin->d, A.lin->wT + kStripFiltOff + kStripFiltLen, A.small_list, A.n_small, A.bad, c->s_mc);
            c->n_launch[0]++;
        }
    }
    if (A.routed) {
        McBatch BL = BR, BSH = BR;
        BL.n = A.n_sweep; BL.nmax = A.nmax_sweep;
        BSH.n = A.n_short; BSH.nmax = A.nmax_short;
        if (BL.nmax > 0) sweep(BL, A.plan_sweep);
        if (A.short_count > 0) sweep(BSH, A.plan_short);
    } else
        sweep(BR, A.plan);
    if (phase == 1) {
        hipLaunchKernelGGL(lin_finish, dim3((BR.ns + 63) / 64), dim3(64), 0, c->s_mc, BR, A.lin->d, A.logz, A.bad);
        hipLaunchKernelGGL(mc_unpaired, dim3((BR.nmax + 63) / 64, BR.ns), dim3(256), 0, c->s_mc, BR, A.up_w);
    }
    return RH_OK;
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
