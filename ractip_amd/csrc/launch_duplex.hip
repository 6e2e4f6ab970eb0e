// launch_duplex.hip -- launch sequences of the duplex (hybridization) sweeps: log space and scaled linear space,
// CONTRAfold and Vienna-BL models.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "ctx.h"
#include "kernels.h"

namespace rh::host {

// ---- duplex sweeps, log-space path
int launch_dx_log(rh_ctx* c, const DxBatch& D)
{
    const int smax = D.n1max + D.n2max;
    const int steps = smax / 2;
    const int waves = 2 * std::min(D.n1max, D.n2max);
    for (int t = 0; t < steps; t++) {
        KLAUNCH(c, 4, dx_sweep_diag, dim3((waves + 3) / 4, D.np, 2), dim3(256), c->s_dx, D, c->d_model, t);
        c->n_launch[2]++;
    }
    hipLaunchKernelGGL(dx_logz, dim3(D.np), dim3(1024), 0, c->s_dx, D, c->d_model);
    const int cells = D.n1max * D.n2max;
    hipLaunchKernelGGL(dx_posterior, dim3((cells + 255) / 256, D.np), dim3(256), 0, c->s_dx, D);
    return RH_OK;
}

// ---- duplex sweeps, scaled linear path: eight (dxl_strip8), four (dxl_sweep4) or two (dxl_sweep<W>) anti-diagonals per launch;
// W = 4 has all three, W = 2 and 8 the last.  Each kernel on one line with the name reported for it.
using DxSweepK = void (*)(DxLinBatch, const DxLinModel*, int, int);
const Named<void (*)(DxLinBatch, const DxLinModel*, int)> kDxStrip8 = NAMED(dxl_strip8);
const Named<DxSweepK> kDxSweep4 = NAMED(dxl_sweep4);
struct DxSweepKernels { int W; Named<DxSweepK> k; };
const DxSweepKernels kDxSweepW[] = {{4, NAMED(dxl_sweep<4>)}, {2, NAMED(dxl_sweep<2>)}, {8, NAMED(dxl_sweep<8>)}};
static const DxSweepKernels& dx_sweep_kernels(int W) { return row_of(kDxSweepW, [&](const DxSweepKernels& r) { return r.W == W; }); }
// Vienna-BL: [0] ViennaRNA-1.8 loop energies, [1] 2.x (four more tables per pair)
const Named<void (*)(DxLinBatch, const VLinModel*, const VDxLin*, int)> kDxvlSweep4[2] = {NAMED(dxvl_sweep4<false>), NAMED(dxvl_sweep4<true>)};

SweepPlan plan_dx_lin(const rh_ctx* c, int w)
{
    SweepPlan P;
    P.W = w == 2 || w == 8 ? w : 4;
    P.org = !(P.W == 4 && c->dx_quad) ? SweepPlan::kDxSweepW : c->dx_strip ? SweepPlan::kDxStrip8 : SweepPlan::kDxSweep4;
    P.fine = P.org == SweepPlan::kDxStrip8 ? kDxStrip8.name : P.org == SweepPlan::kDxSweep4 ? kDxSweep4.name : dx_sweep_kernels(P.W).k.name;
    return P;
}
SweepPlan plan_dx_vlin(bool sem20)   // (one organisation, an instantiation per semantics)
{
    SweepPlan P;
    P.org = SweepPlan::kDxSweep4;
    P.fine = kDxvlSweep4[sem20 ? 1 : 0].name;
    return P;
}

// A.X: the whole batch, or a compacted sub-batch of the scale-exponent ladder with its own tables
int launch_dx_lin(rh_ctx* c, const DxLinArgs& A)
{
    DxLinBatch X = A.X;
    const SweepPlan& P = A.plan;
    const DxLinModel* dm = A.dm;
    const int smax = X.n1max + X.n2max;
    const int steps = smax / 2;
    const int groups = (X.n1max + 2 + 63) / 64;
    const double leu = A.hm->lam_eu, l2 = A.hm->lam_pow[2];
    const size_t lz_lds = dxl_logz_lds_bytes(X.lds);
    if (!lz_lds) return fail(c, RH_ERR_UNSUPPORTED, "duplex log Z: the letters of a pair do not fit in LDS");
    if (P.org == SweepPlan::kDxStrip8) {
        for (int t = 0; 8 * t < smax - 1; t++) {
            for (int k = 0; k < 8; k++) X.pw8[k] = std::pow(leu, 8.0 * t + k) * l2;
            // (only the groups the bands of this step's rows can touch; the kernel places them per pair)
            KLAUNCH(c, 4, (kDxStrip8.kern), dim3(dxl_strip8_groups(X.n1max, X.n2max, t), X.np, 2), dim3(512), c->s_dx, X, dm, t);
            c->n_launch[2]++;
        }
    } else if (P.org == SweepPlan::kDxSweep4) {
        const int groups4 = (X.n1max + 2 + 61) / 62;
        for (int t = 0; 4 * t < smax - 1; t++) {
            for (int k = 0; k < 4; k++) X.pw4[k] = std::pow(leu, 4.0 * t + k) * l2;
            KLAUNCH(c, 4, (kDxSweep4.kern), dim3(groups4, X.np, 2), dim3(256), c->s_dx, X, dm, t, groups4);
            c->n_launch[2]++;
        }
    } else
    for (int t = 0; t < steps; t++) {   // two anti-diagonals per launch
        // inside diagonal sd = 2+2t+k: (lam e^eu)^(sd-2) lam^2 ; outside sd = Smax-2t-1+k: (lam e^eu)^(2t+1-k) lam^2
        X.pw_in[0] = std::pow(leu, 2.0 * t) * l2;      X.pw_in[1] = X.pw_in[0] * leu;
        X.pw_out[1] = std::pow(leu, 2.0 * t) * l2;     X.pw_out[0] = X.pw_out[1] * leu;
        KLAUNCH(c, 4, (dx_sweep_kernels(P.W).k.kern), dim3(groups, X.np, 2), dim3(64 * P.W), c->s_dx, X, dm, t, groups);
        c->n_launch[2]++;
    }
    int* cpart = (int*)(A.zpart + (size_t)X.np * A.lz_chunks);
    hipLaunchKernelGGL(dxl_logz_part, dim3(A.lz_chunks, X.np), dim3(kLzThreads), lz_lds, c->s_dx, X, dm, A.zpart, cpart, A.lz_chunks);
    hipLaunchKernelGGL(dxl_logz_final, dim3((X.np + 63) / 64), dim3(64), 0, c->s_dx, X, dm, (const double*)A.zpart, (const int*)cpart,
                       A.lz_chunks, A.zbar, A.logz, A.bad);
    hipLaunchKernelGGL(dxl_posterior, dim3((X.n1max + 31) / 32, (smax - 1 + 31) / 32, X.np), dim3(256), 0, c->s_dx, X, (const double*)A.zbar, A.bad);
    return RH_OK;
}

// Vienna-BL pf_duplex, scaled linear space (duplex_vlin.hip)
int launch_dx_vlin(rh_ctx* c, const DxLinArgs& A)
{
    DxLinBatch X = A.X;
    const int smax = X.n1max + X.n2max;
    const int groups4 = (X.n1max + 2 + 61) / 62;
    const double lam = std::exp(-A.vdx_s);
    for (int t = 0; 4 * t < smax - 1; t++) {
        for (int k = 0; k < 4; k++) X.pw4[k] = std::pow(lam, 2.0 + 4.0 * t + k);
        KLAUNCH(c, 4, (kDxvlSweep4[A.sem20 ? 1 : 0].kern), dim3(groups4, X.np, 2), dim3(256), c->s_dx, X, c->d_vdxl, c->d_vdx, t);
        c->n_launch[2]++;
    }
    int* cpart = (int*)(A.zpart + (size_t)X.np * A.lz_chunks);
    if (A.sem20) hipLaunchKernelGGL(dxvl_logz_part<true>, dim3(A.lz_chunks, X.np), dim3(256), 0, c->s_dx, X, c->d_vdxl, c->d_vdx, A.zpart, cpart, A.lz_chunks);
    else hipLaunchKernelGGL(dxvl_logz_part<false>, dim3(A.lz_chunks, X.np), dim3(256), 0, c->s_dx, X, c->d_vdxl, c->d_vdx, A.zpart, cpart, A.lz_chunks);
    hipLaunchKernelGGL(dxvl_logz_final, dim3((X.np + 63) / 64), dim3(64), 0, c->s_dx, X, A.vdx_s, (const double*)A.zpart, (const int*)cpart,
                       A.lz_chunks, A.zbar, A.logz, A.bad);
    hipLaunchKernelGGL(dxl_posterior, dim3((X.n1max + 31) / 32, (smax - 1 + 31) / 32, X.np), dim3(256), 0, c->s_dx, X, (const double*)A.zbar, A.bad);
    return RH_OK;
}
int launch_dx_vlog(rh_ctx* c)
{
    const DxBatch& D = c->dx;
    const int steps = (D.n1max + D.n2max) / 2;
    const int waves = 2 * std::min(D.n1max, D.n2max);
    for (int t = 0; t < steps; t++) {
        KLAUNCH(c, 4, dxv_sweep_diag, dim3((waves + 3) / 4, D.np, 2), dim3(256), c->s_dx, D, c->d_vienna, t);
        c->n_launch[2]++;
    }
    hipLaunchKernelGGL(dxv_logz, dim3(D.np), dim3(1024), 0, c->s_dx, D, c->d_vienna);
    hipLaunchKernelGGL(dxv_posterior, dim3((D.n1max * D.n2max + 255) / 256, D.np), dim3(256), 0, c->s_dx, D);
    return RH_OK;
}

}  // namespace rh::host
