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
int launch_dx_log(rh_ctx* c) { return launch_dx_log(c, c->dx); }

// ---- duplex sweeps, scaled linear path
// X: the batch (the whole one, or a compacted sub-batch of the scale-exponent ladder with its own tables); dm / hm: the model at the
// scale exponent of this pass; logz_out / bad: per pair of X
template <int W>
int launch_dx_lin_on(rh_ctx* c, DxLinBatch X, const DxLinModel* dm, const DxLinModel& hm, double* logz_out, int* bad)
{
    const int smax = X.n1max + X.n2max;
    const int steps = smax / 2;
    const int groups = (X.n1max + 2 + 63) / 64;
    const double leu = hm.lam_eu, l2 = hm.lam_pow[2];
    if (W == 4 && c->dx_quad && c->dx_strip) {   // eight anti-diagonals per launch (dxl_strip8)
        const int groups8 = (X.n1max + 2 + 57) / 58;
        for (int t = 0; 8 * t < smax - 1; t++) {
            for (int k = 0; k < 8; k++) X.pw8[k] = std::pow(leu, 8.0 * t + k) * l2;
            KLAUNCH(c, 4, dxl_strip8, dim3(groups8, X.np, 2), dim3(512), c->s_dx, X, dm, t);
            c->n_launch[2]++;
        }
    } else
    if (W == 4 && c->dx_quad) {   // four anti-diagonals per launch (dxl_sweep4)
        const int groups4 = (X.n1max + 2 + 61) / 62;
        for (int t = 0; 4 * t < smax - 1; t++) {
            for (int k = 0; k < 4; k++) X.pw4[k] = std::pow(leu, 4.0 * t + k) * l2;
            KLAUNCH(c, 4, dxl_sweep4, dim3(groups4, X.np, 2), dim3(256), c->s_dx, X, dm, t, groups4);
            c->n_launch[2]++;
        }
    } else
    for (int t = 0; t < steps; t++) {
        // inside diagonal sd = 2+2t+k: (lam e^eu)^(sd-2) lam^2 ; outside sd = Smax-2t-1+k: (lam e^eu)^(2t+1-k) lam^2
        X.pw_in[0] = std::pow(leu, 2.0 * t) * l2;      X.pw_in[1] = X.pw_in[0] * leu;
        X.pw_out[1] = std::pow(leu, 2.0 * t) * l2;     X.pw_out[0] = X.pw_out[1] * leu;
        KLAUNCH(c, 4, dxl_sweep<W>, dim3(groups, X.np, 2), dim3(64 * W), c->s_dx, X, dm, t, groups);
        c->n_launch[2]++;
    }
    double* zpart = c->d_zpart.as<double>();
    int* cpart = (int*)(zpart + (size_t)X.np * c->lz_chunks);
    hipLaunchKernelGGL(dxl_logz_part, dim3(c->lz_chunks, X.np), dim3(256), 0, c->s_dx, X, dm, zpart, cpart, c->lz_chunks);
    hipLaunchKernelGGL(dxl_logz_final, dim3((X.np + 63) / 64), dim3(64), 0, c->s_dx, X, dm, (const double*)zpart, (const int*)cpart,
                       c->lz_chunks, c->d_zbar.as<double>(), logz_out, bad);
    hipLaunchKernelGGL(dxl_posterior, dim3((X.n1max + 31) / 32, (smax - 1 + 31) / 32, X.np), dim3(256), 0, c->s_dx, X, c->d_zbar.as<const double>(), bad);
    return RH_OK;
}
template int launch_dx_lin_on<4>(rh_ctx*, DxLinBatch, const DxLinModel*, const DxLinModel&, double*, int*);   // (fallbacks.hip: retry_dx_lin_rungs)
template <int W>
int launch_dx_lin(rh_ctx* c) { return launch_dx_lin_on<W>(c, c->dxl, c->d_dxlin, c->h_dxlin, c->d_logz.as<double>(), c->d_dxbad.as<int>()); }

// Vienna-BL pf_duplex, scaled linear space (duplex_vlin.hip)
int launch_dx_vlin(rh_ctx* c)
{
    DxLinBatch X = c->dxl;
    const int smax = X.n1max + X.n2max;
    const int groups4 = (X.n1max + 2 + 61) / 62;
    const double lam = std::exp(-c->vdx_s);
    for (int t = 0; 4 * t < smax - 1; t++) {
        for (int k = 0; k < 4; k++) X.pw4[k] = std::pow(lam, 2.0 + 4.0 * t + k);
        KLAUNCH(c, 4, dxvl_sweep4, dim3(groups4, X.np, 2), dim3(256), c->s_dx, X, c->d_vdxl, c->d_vdx, t);
        c->n_launch[2]++;
    }
    double* zpart = c->d_zpart.as<double>();
    int* cpart = (int*)(zpart + (size_t)X.np * c->lz_chunks);
    hipLaunchKernelGGL(dxvl_logz_part, dim3(c->lz_chunks, X.np), dim3(256), 0, c->s_dx, X, c->d_vdxl, c->d_vdx, zpart, cpart, c->lz_chunks);
    hipLaunchKernelGGL(dxvl_logz_final, dim3((X.np + 63) / 64), dim3(64), 0, c->s_dx, X, c->vdx_s, (const double*)zpart, (const int*)cpart,
                       c->lz_chunks, c->d_zbar.as<double>(), c->d_logz.as<double>(), c->d_dxbad.as<int>());
    hipLaunchKernelGGL(dxl_posterior, dim3((X.n1max + 31) / 32, (smax - 1 + 31) / 32, X.np), dim3(256), 0, c->s_dx, X, c->d_zbar.as<const double>(),
                       c->d_dxbad.as<int>());
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
int launch_dx_lin_any(rh_ctx* c)
{
    switch (c->dx_w) {
        case 2: return launch_dx_lin<2>(c);
        case 8: return launch_dx_lin<8>(c);
        default: return launch_dx_lin<4>(c);
    }
}

}  // namespace rh::host
