// local_windows.cpp -- the argument checks of rh_local_fold and rh_local_duplex, the shapes they give and the automatic chunk sizes
// (local_windows.h).  Host only: no HIP, no context.
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

}  // namespace rh::host
