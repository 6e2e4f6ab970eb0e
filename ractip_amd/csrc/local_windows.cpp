// local_windows.cpp -- the argument checks of rh_local_fold, rh_local_duplex and rh_local_duplex2, the shapes they give and the
// automatic chunk and tile sizes (local_windows.h).  Host only: no HIP, no context.
#include "local_windows.h"

#include "../../include/ractip_hot.h"

namespace rh::host {

static int reject(std::string* why, const std::string& text) { *why = text; return RH_ERR_ARG; }

int local_check(const char* seq, int n, int window, int step, LocalPlan* P, std::string* why)
{
    if (!seq) return reject(why, "local fold: the sequence is NULL");
    if (n < 1) return reject(why, "local fold: the sequence has length " + std::to_string(n) + " (must be >= 1)");
    if (window < 2) return reject(why, "local fold: window " + std::to_string(window) + " (must be >= 2)");
    if (step < 1) return reject(why, "local fold: step " + std::to_string(step) + " (must be >= 1)");
    if (step > window) return reject(why, "local fold: step " + std::to_string(step) + " exceeds the window " + std::to_string(window));
    *P = LocalPlan();
    P->n = n; P->W = window; P->S = step;
    P->We = n < window ? n : window;
    P->nw = n <= window ? 1 : (n - window + step - 1) / step + 1;
    P->ld = P->We;
    return RH_OK;
}

int local_duplex_check(const char* s1, int n1, const char* s2, int n2, int windowed, int window, int step, LocalDuplexPlan* D, std::string* why)
{
    if (!s1 || !s2) return reject(why, std::string("local duplex: sequence ") + (!s1 ? "1" : "2") + " is NULL");
    if (n1 < 1) return reject(why, "local duplex: sequence 1 has length " + std::to_string(n1) + " (must be >= 1)");
    if (n2 < 1) return reject(why, "local duplex: sequence 2 has length " + std::to_string(n2) + " (must be >= 1)");
    if (windowed != 1 && windowed != 2) return reject(why, "local duplex: windowed " + std::to_string(windowed) + " (must be 1 or 2)");
    LocalPlan P;
    std::string inner;
    if (local_check(windowed == 1 ? s1 : s2, windowed == 1 ? n1 : n2, window, step, &P, &inner))
        return reject(why, "local duplex" + inner.substr(std::string("local fold").size()));   // (the window and the step, as local_check words them)
    *D = LocalDuplexPlan();
    D->P = P; D->n1 = n1; D->n2 = n2; D->windowed = windowed;
    D->nq = windowed == 1 ? n2 : n1;
    return RH_OK;
}

size_t local_fold_bytes(int nmax, const LocalTables& T)
{
    const McBatch B = mc_layout(1, nmax, T.fold);
    return sizeof(double) * (B.seq_stride + B.pk_stride * kPkCopies + B.tri_stride);
}

size_t local_pair_bytes(int n1max, int n2max, const LocalTables& T)
{
    const int lds = seq_lds(n1max > n2max ? n1max : n2max);
    const DxBatch D = dx_layout(1, n1max, n2max, lds, T.dx);
    const DxLinBatch X = dxl_layout(1, n1max, n2max, lds, D.ldd, T.dxl);
    size_t doubles = (D.pair_stride > X.pair_stride ? D.pair_stride : X.pair_stride) + D.tab_stride;   // tables (one buffer) + the hp block
    if (T.cofold) {
        const McBatch C = mc_layout(1, n1max + n2max, (int)VM_COUNT);
        doubles += C.seq_stride + C.pk_stride * kPkCopies + C.tri_stride;
    }
    return sizeof(double) * doubles;
}

// the largest count within [1, most] whose bytes fit: a multiple of 8 above 8 (the XCD count: xcd_pin)
static int chunk_of(size_t budget, size_t per_window, int most)
{
    size_t chunk = budget / per_window;
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)most) chunk = (size_t)most;
    if (chunk > 8) chunk &= ~(size_t)7;
    return (int)chunk;
}

int local_chunk_auto(const LocalPlan& P, const LocalTables& T)
{
    return chunk_of(kLocalChunkBytes, local_fold_bytes(P.We, T), kLocalChunkMax);
}

int local_duplex_chunk_auto(const LocalDuplexPlan& D, const LocalTables& T)
{
    const int nmax = D.nq > D.P.We ? D.nq : D.P.We;   // every sequence of the batch has tables for the longest one
    const size_t fold = local_fold_bytes(nmax, T);
    const size_t budget = kLocalChunkBytes > fold ? kLocalChunkBytes - fold : 0;   // the query, once per chunk
    return chunk_of(budget, fold + local_pair_bytes(local_n1max(D), local_n2max(D), T), kLocalChunkMax - 1);
}

int local_duplex2_check(const char* s1, int n1, const char* s2, int n2, int window1, int step1, int window2, int step2, LocalDuplex2Plan* D,
                        std::string* why)
{
    const std::string head = "local duplex2: ";
    if (!s1 || !s2) return reject(why, head + "sequence " + (!s1 ? "1" : "2") + " is NULL");
    const int n[2] = {n1, n2}, window[2] = {window1, window2}, step[2] = {step1, step2};
    for (int m = 0; m < 2; m++)
        if (n[m] < 1) return reject(why, head + "sequence " + std::to_string(m + 1) + " has length " + std::to_string(n[m]) + " (must be >= 1)");
    LocalPlan P[2];
    for (int m = 0; m < 2; m++) {
        const std::string side = std::to_string(m + 1), w = std::to_string(window[m]), s = std::to_string(step[m]);
        if (window[m] < 2) return reject(why, head + "window" + side + " " + w + " (must be >= 2)");
        if (step[m] < 1) return reject(why, head + "step" + side + " " + s + " (must be >= 1)");
        if (step[m] > window[m]) return reject(why, head + "step" + side + " " + s + " exceeds window" + side + " " + w);
        std::string inner;
        if (local_check(m ? s2 : s1, n[m], window[m], step[m], &P[m], &inner)) return reject(why, head + inner);
    }
    const long long pairs = (long long)P[0].nw * (long long)P[1].nw;
    if (pairs > 0x7fffffffLL)
        return reject(why, head + std::to_string(P[0].nw) + " x " + std::to_string(P[1].nw) + " window pairs (at most " + std::to_string(0x7fffffff) + ")");
    *D = LocalDuplex2Plan();
    D->P1 = P[0]; D->P2 = P[1];
    return RH_OK;
}

bool local_tile_fits(const LocalDuplex2Plan& D, const LocalTables& T, size_t rows, size_t cols)
{
    if (rows + cols > (size_t)kLocalChunkMax || rows * cols > (size_t)kLocalChunkMax - 1) return false;
    const size_t fold = local_fold_bytes(D.P1.We > D.P2.We ? D.P1.We : D.P2.We, T);   // every sequence of the batch has tables for the longest one
    const size_t pair = local_pair_bytes(D.P1.We, D.P2.We, T);
    const size_t rowbuf = sizeof(double) * local_hp2_rowbuf_size(D, 1);
    return (rows + cols) * fold + rows * cols * pair + rows * rowbuf <= kLocalChunkBytes;
}

void local_tile_auto(const LocalDuplex2Plan& D, const LocalTables& T, int* rows, int* cols)
{
    size_t t = 1;
    while (local_tile_fits(D, T, t + 1, t + 1)) t++;
    const size_t nw1 = (size_t)D.P1.nw, nw2 = (size_t)D.P2.nw;
    size_t r = t < nw1 ? t : nw1, c = t < nw2 ? t : nw2;
    if (r < t) while (c < nw2 && local_tile_fits(D, T, r, c + 1)) c++;
    else if (c < t) while (r < nw1 && local_tile_fits(D, T, r + 1, c)) r++;
    *rows = (int)r; *cols = (int)c;
}

}  // namespace rh::host
