// dx_fused_check.cpp -- stand-alone host program around the fused, pair-indexed weight tables of dxl_strip8 (DxLinModel::F,
// ractip_amd/csrc/lin_model.h; built by build_dx_lin_model, param_loader.cpp).  No GPU, no HIP; meant to be built with the sanitizers too:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc
//       tools/dx_fused_check.cpp ractip_amd/csrc/param_loader.cpp -o dx_fused_check        (one command line)
//   ./dx_fused_check PARAMS|synthetic [S]
//
// For every pairing (x, y), every combination of the four neighbour letters (codes 0..4: A, C, G, U, and 4 for an unknown letter or the
// sentinel at positions 0 and L+1 of a row) and both directions, the seven weights are looked up the way the kernel looks them up (own
// entry, decorating entry) and compared AS BITS with the products evaluated from the plain tables in the order dx_cell_weights
// (duplex_lin.hip) writes them.  `synthetic` fills the score tables with distinct values, so that a transposed index cannot hide behind
// equal table entries.  Prints one summary line; exit status 0 only if every weight has the same bits and every entry was reached.
// tests/test_dx_fused_cpu.py runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "lin_model.h"

namespace {

struct Weights { double e_up, e_dn, e_ends, e_st, e_b01, e_b10, e_11; };

// dx_cell_weights, verbatim
Weights plain(const rh::DxLinModel* L, bool outside, int x, int xm, int xp, int y, int ym, int yp)
{
    Weights o;
    o.e_up = L->E_tm[((x * 5 + y) * 5 + xp) * 5 + ym];
    o.e_dn = L->E_tm[((y * 5 + x) * 5 + yp) * 5 + xm] * L->E_bp[x * 5 + y];
    if (!outside) {
        o.e_ends = L->E_dr[y * 25 + x * 5 + xm] * L->E_dl[y * 25 + x * 5 + yp] * L->E_bp[y * 5 + x] * L->E_hc[y * 5 + x];
        o.e_st = L->E_bp[x * 5 + y] * L->E_hs[((xm * 5 + yp) * 5 + x) * 5 + y];
        o.e_b01 = L->E_b01[yp]; o.e_b10 = L->E_b10[xm]; o.e_11 = L->E_11[xm * 5 + yp];
    } else {
        o.e_ends = L->E_dl[x * 25 + y * 5 + xp] * L->E_dr[x * 25 + y * 5 + ym] * L->E_hc[x * 5 + y];
        o.e_st = L->E_bp[xp * 5 + ym] * L->E_hs[((x * 5 + y) * 5 + xp) * 5 + ym];
        o.e_b01 = L->E_b01[ym]; o.e_b10 = L->E_b10[xp]; o.e_11 = L->E_11[xp * 5 + ym];
    }
    return o;
}

// the look-up of dxl_strip8
Weights fused(const rh::DxLinModel* L, bool outside, int x, int xm, int xp, int y, int ym, int yp, std::vector<int>* seen)
{
    const double* wt = L->F[outside ? 1 : 0];
    const int pt = rh::dx_pair_type(x, y);
    const int eo = ((pt * 5 + (outside ? xp : xm)) * 5 + (outside ? ym : yp)) * rh::kDxFusedK;
    const int ed = ((pt * 5 + (outside ? xm : xp)) * 5 + (outside ? yp : ym)) * rh::kDxFusedK;
    if (eo < 0 || eo + rh::kDxFusedK > rh::kDxFused || ed < 0 || ed + rh::kDxFusedK > rh::kDxFused) { std::fprintf(stderr, "entry out of range\n"); std::exit(1); }
    (*seen)[(outside ? rh::kDxFusedEntries : 0) + eo / rh::kDxFusedK] |= 2;
    (*seen)[(outside ? rh::kDxFusedEntries : 0) + ed / rh::kDxFusedK] |= 1;
    Weights o;
    const double f_dec = wt[ed], f_own = wt[eo + 1];
    o.e_up = outside ? f_own : f_dec;
    o.e_dn = outside ? f_dec : f_own;
    o.e_ends = wt[eo + 2]; o.e_st = wt[eo + 3]; o.e_b01 = wt[eo + 4]; o.e_b10 = wt[eo + 5]; o.e_11 = wt[eo + 6];
    return o;
}

void fill_synthetic(rh::ScoreModel* m)
{
    std::memset(m, 0, sizeof(*m));
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {   // distinct scores in (-1.5, 1.5)
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return ((double)(state >> 11) / 9007199254740992.0 - 0.5) * 3.0;
    };
    for (double& v : m->base_pair) v = next();
    for (double& v : m->helix_closing) v = next();
    for (double& v : m->internal_1x1) v = next();
    for (int k = 0; k < 5; k++) { m->bulge_0x1[k] = next(); m->bulge_1x0[k] = next(); }
    for (double& v : m->dangle_left) v = next();
    for (double& v : m->dangle_right) v = next();
    for (double& v : m->terminal_mismatch) v = next();
    for (double& v : m->helix_stacking) v = next();
    m->external_unpaired = next();
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s PARAMS|synthetic [S]\n", argv[0]); return 2; }
    const double s = argc > 2 ? std::atof(argv[2]) : 0.65;
    auto m = std::make_unique<rh::ScoreModel>();
    if (!std::strcmp(argv[1], "synthetic")) fill_synthetic(m.get());
    else {
        char err[256] = "";
        if (!rh::load_score_model(argv[1], m.get(), err, sizeof(err))) { std::fprintf(stderr, "%s: %s\n", argv[1], err); return 2; }
    }
    auto L = std::make_unique<rh::DxLinModel>();
    rh::build_dx_lin_model(*m, s, L.get());

    int types = 0, seen_type[6] = {};
    long compared = 0, differ = 0;
    std::vector<int> seen(2 * rh::kDxFusedEntries, 0);
    for (int x = 0; x < 5; x++) for (int y = 0; y < 5; y++) {
        if (!((rh::kDxPairMask >> (x * 5 + y)) & 1u)) continue;
        const int pt = rh::dx_pair_type(x, y);
        if (pt < 0 || pt >= 6 || seen_type[pt]++) { std::fprintf(stderr, "pair type of (%d, %d) is %d\n", x, y, pt); return 1; }
        types++;
        for (int outside = 0; outside < 2; outside++)
            for (int xm = 0; xm < 5; xm++) for (int xp = 0; xp < 5; xp++) for (int ym = 0; ym < 5; ym++) for (int yp = 0; yp < 5; yp++) {
                const Weights a = plain(L.get(), outside, x, xm, xp, y, ym, yp);
                const Weights b = fused(L.get(), outside, x, xm, xp, y, ym, yp, &seen);
                const double* pa = &a.e_up;
                const double* pb = &b.e_up;
                for (int k = 0; k < 7; k++) {
                    compared++;
                    if (std::memcmp(pa + k, pb + k, sizeof(double))) {
                        if (!differ++) std::fprintf(stderr, "first difference: %s (x, y) = (%d, %d), xm xp ym yp = %d %d %d %d, weight %d: %.17g != %.17g\n",
                                                    outside ? "outside" : "inside", x, y, xm, xp, ym, yp, k, pa[k], pb[k]);
                    }
                }
            }
    }
    int unreached = 0;
    for (int v : seen) unreached += v != 3;
    // distinct values among the fused doubles: how much a transposed index could hide
    std::vector<double> all(&L->F[0][0], &L->F[0][0] + 2 * rh::kDxFused);
    long distinct = 0;
    {
        std::vector<uint64_t> bits(all.size());
        std::memcpy(bits.data(), all.data(), all.size() * sizeof(double));
        std::sort(bits.begin(), bits.end());
        distinct = std::unique(bits.begin(), bits.end()) - bits.begin();
    }
    std::printf("types %d compared %ld differ %ld unreached %d distinct %ld of %d\n", types, compared, differ, unreached, distinct, 2 * rh::kDxFused);
    return (types == 6 && differ == 0 && unreached == 0) ? 0 : 1;
}
