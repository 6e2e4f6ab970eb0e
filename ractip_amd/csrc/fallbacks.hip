// fallbacks.hip -- what happens to the problems whose scaled values left the double range: other scale exponents on the
// linear kernels (the ladders), the log-space kernels on a compacted sub-batch, or a helper context (Vienna-BL pairs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "kernels.h"

namespace rh::host {

// ---- per-problem fallback (CONTRAfold model): only the sequences / pairs whose scaled values left the double range are
// recomputed by the log-space kernels, as a compacted sub-batch; everyone else keeps the linear-path result, bit for bit.
// (The reference has no such cliff at all: its log-space arithmetic, LogSpace.hpp:232-244, is always valid.)
//
// The four paths below share the compaction: gather the flagged problems' codes and lengths from the host mirror of the upload,
// upload them to the d_sub* buffers, run, and copy the result rows back to the flagged slots.  What differs stays in each path:
// which tables are cleared, whether the sub-batch has tables of its own, the stream, and what an error has to undo.
struct SubBatch {
    int nsub = 0;                  // problems: sequences (per = 1) or pairs (per = 2: both sequences of pair p, through seq_of)
    std::vector<uint8_t> codes;    // [per * nsub][lds]
    std::vector<int> lens;         // [per * nsub]
    int nmax[2] = {0, 0};          // longest sequence (pairs: longest first / second strand)
};

SubBatch gather(const rh_ctx* c, const std::vector<int>& F, int per, int lds)
{
    SubBatch s;
    s.nsub = (int)F.size();
    s.codes.resize((size_t)per * s.nsub * lds);
    s.lens.resize((size_t)per * s.nsub);
    for (int k = 0; k < s.nsub; k++)
        for (int h = 0; h < per; h++) {
            const size_t to = (size_t)per * k + h, from = per == 2 ? (size_t)seq_of(c, F[k], h) : (size_t)F[k];
            std::memcpy(s.codes.data() + to * lds, c->h_codes.data() + from * lds, lds);
            s.lens[to] = c->n[from];
            s.nmax[h] = std::max(s.nmax[h], s.lens[to]);
        }
    return s;
}

// Sequences, on the McCaskill stream: codes, lengths and zeroed bp rows in the d_sub* buffers; *S = the sub-batch as the kernels see
// it.  It keeps ld and the strides of the staged batch and REUSES its tables and f5 rows (dead after the pass that flagged these
// sequences), so result rows go back one for one (scatter_mc).  The uploads are in flight on return: `sub` has to outlive the
// caller's hipStreamSynchronize.
int stage_mc_sub(rh_ctx* c, const SubBatch& sub, McBatch* S)
{
    const McBatch& B = c->mc;
    const int nsub = sub.nsub;
    const size_t up_per = (size_t)B.ld * c->max_w;
    int rc;
    if ((rc = ensure(c, c->d_subseq, sub.codes.size(), false))) return rc;
    if ((rc = ensure(c, c->d_subn, sizeof(int) * nsub, false))) return rc;
    if ((rc = ensure(c, c->d_subbp, sizeof(double) * B.tri_stride * nsub, false))) return rc;
    if ((rc = ensure(c, c->d_subup, sizeof(double) * (up_per + 1) * nsub, false))) return rc;   // (+ 1: log Z behind the up rows)
    HIP_TRY(c, hipMemcpyAsync(c->d_subseq.p, sub.codes.data(), sub.codes.size(), hipMemcpyHostToDevice, c->s_mc));
    HIP_TRY(c, hipMemcpyAsync(c->d_subn.p, sub.lens.data(), sizeof(int) * nsub, hipMemcpyHostToDevice, c->s_mc));
    HIP_TRY(c, hipMemsetAsync(c->d_subbp.p, 0, sizeof(double) * B.tri_stride * nsub, c->s_mc));
    *S = B;
    S->ns = nsub; S->nmax = sub.nmax[0];
    S->seq = c->d_subseq.as<const uint8_t>(); S->n = c->d_subn.as<const int>();
    S->f5i = c->d_f5.as<double>(); S->f5o = c->d_f5.as<double>() + (size_t)B.ld * nsub;
    S->bp = c->d_subbp.as<double>(); S->up = c->d_subup.as<double>();
    return RH_OK;
}

// bp and up rows of sub-batch sequence k -> sequence `slot` of the staged batch
hipError_t scatter_mc(rh_ctx* c, int k, int slot)
{
    const size_t tri = c->mc.tri_stride, up_per = (size_t)c->mc.ld * c->max_w;
    const hipError_t e = hipMemcpyAsync(c->d_bp.as<double>() + (size_t)slot * tri, c->d_subbp.as<double>() + (size_t)k * tri, sizeof(double) * tri,
                                        hipMemcpyDeviceToDevice, c->s_mc);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(c->d_up.as<double>() + (size_t)slot * up_per, c->d_subup.as<double>() + (size_t)k * up_per, sizeof(double) * up_per,
                          hipMemcpyDeviceToDevice, c->s_mc);
}

// Pairs, on the duplex stream: codes and lengths in d_subdseq / d_subdn, and `own_bytes` of d_subdx for the sub-batch's OWN tables and
// result rows, which the caller lays out (the linear duplex image of the staged batch keeps zero pad columns between runs).
// As above, `sub` has to outlive the caller's hipStreamSynchronize.
int stage_dx_sub(rh_ctx* c, const SubBatch& sub, size_t own_bytes)
{
    int rc;
    if ((rc = ensure(c, c->d_subdseq, sub.codes.size(), false))) return rc;
    if ((rc = ensure(c, c->d_subdn, sizeof(int) * sub.lens.size(), false))) return rc;
    if ((rc = ensure(c, c->d_subdx, own_bytes, false))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_subdseq.p, sub.codes.data(), sub.codes.size(), hipMemcpyHostToDevice, c->s_dx));
    HIP_TRY(c, hipMemcpyAsync(c->d_subdn.p, sub.lens.data(), sizeof(int) * sub.lens.size(), hipMemcpyHostToDevice, c->s_dx));
    return RH_OK;
}

// hp matrix and log Z of sub-batch pair k -> pair `slot` of the staged batch (hp rows have the staged batch's stride in both)
hipError_t scatter_dx(rh_ctx* c, const double* sub_hp, const double* sub_logz, int k, int slot)
{
    const size_t hp = c->dx.tab_stride;
    const hipError_t e = hipMemcpyAsync(c->d_hp.as<double>() + (size_t)slot * hp, sub_hp + (size_t)k * hp, sizeof(double) * hp, hipMemcpyDeviceToDevice, c->s_dx);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(c->d_logz.as<double>() + slot, sub_logz + k, sizeof(double), hipMemcpyDeviceToDevice, c->s_dx);
}

int recompute_mc_subset_log(rh_ctx* c, const std::vector<int>& F)
{
    const SubBatch sub = gather(c, F, 1, c->mc.lds);
    const int nsub = sub.nsub;
    McBatch S;
    int rc;
    if ((rc = stage_mc_sub(c, sub, &S))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));   // (the uploads of `sub`)
    // (no table is cleared: the tables of the linear pass are dead, and the log-space kernels run over them as they are)
    double* sub_logz = c->d_subup.as<double>() + (size_t)c->mc.ld * c->max_w * nsub;
    if ((rc = launch_mc_log(c, xcd_pin(nsub), S, sub_logz))) return rc;
    if ((rc = launch_mc_acc(c, S, nullptr, false))) return rc;
    for (int k = 0; k < nsub; k++) {   // scatter to the flagged sequences' slots
        HIP_TRY(c, scatter_mc(c, k, F[k]));
        HIP_TRY(c, hipMemcpyAsync(c->d_mclogz.as<double>() + F[k], sub_logz + k, sizeof(double), hipMemcpyDeviceToDevice, c->s_mc));
    }
    return RH_OK;
}

// ---- other scale exponents before the log-space kernels (CONTRAfold model).  The scaled linear path stores Q * exp(-s * span): with
// s = 0.12 (random ACGU: log Z per nucleotide 0.11-0.13) a 1100-nt RNA made of stable hairpins (0.58 per nucleotide) passes 1e200.
// Such a sequence is recomputed on the SAME kernels with a larger exponent -- rung 0: s = 0.45, rung 1: s = 1.5 -- and one whose
// values vanish (log Z per nucleotide far below 0.12 on a long sequence) with rung 2: s = 0; only what leaves the range there too
// goes to the log-space kernels (3x slower).  An exponent costs dynamic range only, never accuracy: a cell that underflows to 0
// while Z~ stays inside (1e-200, 1e200) is below 1e-100 of the terms that make up Z.  Flagged sequences are compacted into a
// sub-batch that reuses the (dead) tables of the main pass; results are scattered back into their slots.
const double kRungS[rh_ctx::kRungs] = {0.45, 1.5, 0.0};

int ensure_rungs(rh_ctx* c)
{
    if (c->lin_r) return RH_OK;
    c->lin_r = new LinSet[rh_ctx::kRungs];
    for (int r = 0; r < rh_ctx::kRungs; r++) {
        LinSet& m = c->lin_r[r];
        build_lin_model(*c->h_score, kRungS[r], &m.h);
        bool fok = false;
        const std::vector<double> wT = strip_weights(m.h, &fok);
        if (!fok) c->strip_filt_ok = false;   // (the structure does not depend on the exponent; kept as a guard)
        HIP_TRY(c, m.d.upload(&m.h));
        HIP_TRY(c, m.wT.upload(wT.data(), wT.size()));
    }
    return RH_OK;
}

// `first`: the model of the main pass (-1: the default exponent, k: rung k); `rest`: the sequences it flagged, on return those that
// no rung could hold (for the log-space kernels); rescued_by: the sequences moved to the default exponent [0] / to rung k [k + 1]
int retry_mc_lin_rungs(rh_ctx* c, int first_model, std::vector<int>* rest, int (&rescued_by)[rh_ctx::kRungs + 1])
{
    for (int& q : rescued_by) q = 0;
    if (!c->scale_ladder || rest->empty()) return RH_OK;
    int rc;
    if ((rc = ensure_rungs(c))) return rc;
    const McBatch& B = c->mc;
    const LinSet* first = first_model < 0 ? &c->lin0 : &c->lin_r[first_model];
    // direction: log Z = log(Z~) + s n of the failed pass is +Inf / NaN / large after an overflow, -Inf or below s n after an underflow
    std::vector<double> lz(B.ns);
    HIP_TRY(c, hipMemcpyAsync(lz.data(), c->d_mclogz.p, sizeof(double) * B.ns, hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    std::vector<int> over, under;
    for (int k : *rest) ((lz[k] == lz[k] && lz[k] < first->h.s * c->n[k]) ? under : over).push_back(k);
    // the exponents to try: larger ones in ascending order for the overflows, smaller ones in descending order for the underflows
    // (model -1 = the default exponent, when the main pass ran on a rung)
    size_t n_larger = 0;
    const std::vector<int> tries = exponent_order(first_model, c->lin0.h.s, kRungS, rh_ctx::kRungs, &n_larger);
    for (size_t t = 0; t < tries.size(); t++) {
        const int rung = tries[t];
        std::vector<int>& F = t < n_larger ? over : under;
        if (F.empty()) continue;
        const SubBatch sub = gather(c, F, 1, B.lds);
        const int nsub = sub.nsub;
        McBatch S;
        if ((rc = stage_mc_sub(c, sub, &S))) return rc;
        // the tables (and packed operand tiles) the sub-batch reuses hold Inf / NaN of the failed pass: the fast path masks operands by
        // multiplying with 0 in places
        HIP_TRY(c, hipMemsetAsync(c->d_mctab.p, 0, sizeof(double) * B.seq_stride * nsub, c->s_mc));
        if (c->d_pk) HIP_TRY(c, hipMemsetAsync(c->d_pk.p, 0, sizeof(double) * B.pk_stride * kPkCopies * nsub, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));   // (the uploads of `sub`)
        // the sub-batch runs as it is, with plans of its own and without the per-sequence routing of launch_mc_lin;
        // its launches are not counted
        const LinSet* lin = rung < 0 ? &c->lin0 : &c->lin_r[rung];
        const int saved_nl[2] = {c->n_launch[0], c->n_launch[1]}, saved_nf[2] = {c->n_far[0], c->n_far[1]};
        rc = launch_mc_lin(c, mc_lin_args(c, 0, S, lin, false));
        if (!rc) rc = launch_mc_lin(c, mc_lin_args(c, 1, S, lin, false));
        if (!rc) rc = launch_mc_acc(c, S, lin, false);
        for (int q = 0; q < 2; q++) { c->n_launch[q] = saved_nl[q]; c->n_far[q] = saved_nf[q]; }
        if (rc) return rc;
        // flags and log Z of the sub-batch are the first nsub entries of d_bad / d_mclogz
        std::vector<int> sbad, still;
        std::vector<double> slz(nsub);
        HIP_TRY(c, hipMemcpyAsync(slz.data(), c->d_mclogz.p, sizeof(double) * nsub, hipMemcpyDeviceToHost, c->s_mc));
        if ((rc = flagged(c, c->d_bad.as<int>(), nsub, c->s_mc, &sbad))) return rc;
        size_t b = 0;
        for (int k = 0; k < nsub; k++) {
            if (b < sbad.size() && sbad[b] == k) { b++; still.push_back(F[k]); continue; }
            HIP_TRY(c, scatter_mc(c, k, F[k]));
            lz[F[k]] = slz[k];
            c->rescaled_mc.push_back(F[k]);
            rescued_by[rung + 1]++;
        }
        F.swap(still);
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_mclogz.p, lz.data(), sizeof(double) * B.ns, hipMemcpyHostToDevice, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));   // (lz dies with this scope)
    rest->clear();
    rest->insert(rest->end(), over.begin(), over.end());
    rest->insert(rest->end(), under.begin(), under.end());
    std::sort(rest->begin(), rest->end());
    std::sort(c->rescaled_mc.begin(), c->rescaled_mc.end());
    return RH_OK;
}

int recompute_dx_subset_log(rh_ctx* c, const std::vector<int>& F)
{
    const DxBatch& D = c->dx;
    const SubBatch sub = gather(c, F, 2, D.lds);
    const int nsub = sub.nsub;
    int rc;
    // own tables: the linear duplex image keeps zero pad columns between runs, which the log-space layout would overwrite
    if ((rc = stage_dx_sub(c, sub, sizeof(double) * (D.pair_stride + D.tab_stride + 1) * nsub))) return rc;   // tables, hp, log Z
    double* sub_hp = c->d_subdx.as<double>() + D.pair_stride * nsub;
    double* sub_logz = sub_hp + D.tab_stride * nsub;
    HIP_TRY(c, hipMemsetAsync(sub_hp, 0, sizeof(double) * D.tab_stride * nsub, c->s_dx));   // row 0 / column 0 stay zero
    HIP_TRY(c, hipStreamSynchronize(c->s_dx));   // (the uploads of `sub`)
    DxBatch S = D;
    S.np = nsub; S.n1max = sub.nmax[0]; S.n2max = sub.nmax[1];
    S.seq = c->d_subdseq.as<const uint8_t>(); S.n = c->d_subdn.as<const int>();
    S.tab = c->d_subdx.as<double>(); S.hp = sub_hp; S.logz = sub_logz;
    if ((rc = launch_dx_log(c, S))) return rc;
    for (int k = 0; k < nsub; k++) HIP_TRY(c, scatter_dx(c, sub_hp, sub_logz, k, F[k]));
    return RH_OK;
}

// ---- other scale exponents for the duplex sweeps before the log-space kernels (CONTRAfold model): the duplex counterpart of
// retry_mc_lin_rungs.  IN~ = IN * exp(-s (a+b)) with s = 0.65 per unit of a+b (random ACGU: log Z grows by 0.6 per unit); a pair of
// long complementary strands (1.0 - 1.5 per unit) leaves the double range.  The flagged pairs are recomputed as a compacted sub-batch on
// the SAME linear kernels with s = 1.3, then 2.2 (overflow), then 0.3, then 0 (underflow), with their own tables (zero pad columns),
// and only what no exponent holds goes to the log-space kernels.  An exponent costs dynamic range only, never accuracy.
constexpr int kDxRungs = 4;
constexpr double kDxRungS[kDxRungs] = {1.3, 2.2, 0.3, 0.0};

int retry_dx_lin_rungs(rh_ctx* c, std::vector<int>* rest)
{
    if (!c->scale_ladder || rest->empty() || !c->h_score) return RH_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const DxBatch& D = c->dx;
    int rc;
    if (!c->d_dxlin_r[0]) {
        for (int r = 0; r < kDxRungs; r++) {
            build_dx_lin_model(*c->h_score, kDxRungS[r], &c->h_dxlin_r[r]);
            HIP_TRY(c, c->d_dxlin_r[r].upload(&c->h_dxlin_r[r]));
        }
    }
    std::vector<int> F = *rest, bad;
    for (int r = 0; r < kDxRungs && !F.empty(); r++) {
        const SubBatch sub = gather(c, F, 2, D.lds);
        const int nsub = sub.nsub, n1max = sub.nmax[0], n2max = sub.nmax[1];
        DxLinArgs A = dx_lin_args(c);   // (d_zpart / d_zbar of the main batch: large enough, the sub-batch has no more chunks)
        DxLinBatch& X = A.X;   // lds, ldd, hp_stride as in the main batch: results scatter back row for row
        X = dxl_layout(nsub, n1max, n2max, X.lds, X.ldd, (int)DL_COUNT);
        X.hp_stride = D.tab_stride;
        const size_t tab_d = X.pair_stride * nsub, hp_d = D.tab_stride * nsub;
        const size_t own_bytes = sizeof(double) * (tab_d + hp_d + nsub + 1) + sizeof(int) * nsub;   // tables, hp, log Z, flags
        if ((rc = stage_dx_sub(c, sub, own_bytes))) return rc;
        double* sub_tab = c->d_subdx.as<double>();
        double* sub_hp = sub_tab + tab_d;
        double* sub_logz = sub_hp + hp_d;
        int* sub_bad = (int*)(sub_logz + nsub + 1);
        HIP_TRY(c, hipMemsetAsync(c->d_subdx.p, 0, own_bytes, c->s_dx));   // pad columns, row 0 / column 0 of hp
        HIP_TRY(c, hipStreamSynchronize(c->s_dx));   // (the uploads of `sub`)
        X.seq = c->d_subdseq.as<const uint8_t>(); X.n = c->d_subdn.as<const int>(); X.tab = sub_tab; X.hp = sub_hp;
        A.plan = plan_dx_lin(c, 4);   // (always the four-wavefront organisation, whatever RH_DX_W chose for the first pass: see ADVICE.md)
        A.dm = c->d_dxlin_r[r]; A.hm = &c->h_dxlin_r[r];
        A.lz_chunks = lz_chunks(n1max, n2max);
        A.logz = sub_logz; A.bad = sub_bad;
        if ((rc = launch_dx_lin(c, A))) return rc;
        if ((rc = flagged(c, sub_bad, nsub, c->s_dx, &bad))) return rc;
        std::vector<int> still;
        size_t b = 0;
        for (int k = 0; k < nsub; k++) {
            if (b < bad.size() && bad[b] == k) { b++; still.push_back(F[k]); continue; }
            HIP_TRY(c, scatter_dx(c, sub_hp, sub_logz, k, F[k]));
            c->rescaled_dx.push_back(F[k]);
        }
        HIP_TRY(c, hipStreamSynchronize(c->s_dx));   // the sub-batch buffers are reused by the next rung
        F.swap(still);
    }
    std::sort(c->rescaled_dx.begin(), c->rescaled_dx.end());
    *rest = F;
    return RH_OK;
}

// The flagged pairs P of a Vienna-BL batch, recomputed on the helper context and copied into this batch's result buffers (bp, up, hp and
// the three log partition functions of each pair); the layouts differ only in their strides.  Plain uploads only (compute()): every
// pair owns its two fold rows there.
int recompute_pairs_on_helper(rh_ctx* c, const std::vector<int>& P)
{
    if (!c->helper) {
        c->helper = make_ctx_for_helper(c->device, c->model, c->p_has_param ? c->p_param.c_str() : nullptr, c->p_has_defaults ? c->p_defaults.c_str() : nullptr,
                               c->p_use_bl, c->p_sem);
        if (!c->helper) return fail(c, RH_ERR_HIP, "helper context for the per-pair fallback could not be created");
        c->helper->is_helper = true;
    }
    rh_ctx* h = c->helper;
    h->max_w = c->max_w; h->hybrid = c->hybrid; h->mode = RH_MODE_AUTO; h->duplex_mode = c->duplex_mode; h->scale_ladder = c->scale_ladder; h->scale_memory = 0;
    h->vlin_primary = c->vlin_primary < 0 ? 0 : -1;   // the exponent of the first pass is known to fail for these pairs: start on the next one
    const int nsub = (int)P.size();
    const int lds = c->mc.lds;
    std::vector<std::string> text(2 * (size_t)nsub);
    std::vector<const char*> ptr(2 * (size_t)nsub);
    std::vector<int> lens(2 * (size_t)nsub);
    for (int k = 0; k < nsub; k++)
        for (int hh = 0; hh < 2; hh++) {
            const int sq = seq_of(c, P[k], hh), n = c->n[sq];
            std::string& t = text[2 * k + hh];
            t.resize(n);
            for (int i = 0; i < n; i++) t[i] = "NACGU"[c->h_codes[(size_t)sq * lds + 1 + i] <= 4 ? c->h_codes[(size_t)sq * lds + 1 + i] : 0];   // vienna_code^-1
            ptr[2 * k + hh] = t.c_str(); lens[2 * k + hh] = n;
        }
    int rc;
    BatchRequest r;
    r.ns = 2 * nsub; r.seqs = ptr.data(); r.lens = lens.data();
    r.with_mc = r.with_dx = true;
    if ((rc = stage(h, r))) return fail(c, rc, "helper upload: %s", h->err.c_str());
    if ((rc = compute(h))) return fail(c, rc, "helper compute: %s", h->err.c_str());
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_dx));
    const size_t up_c = (size_t)c->mc.ld * c->max_w, up_h = (size_t)h->mc.ld * h->max_w;
    for (int k = 0; k < nsub; k++) {
        for (int hh = 0; hh < 2; hh++) {
            const int sq = seq_of(c, P[k], hh), sh = 2 * k + hh, n = c->n[sq];
            HIP_TRY(c, hipMemcpyAsync(c->d_bp.as<double>() + (size_t)sq * c->mc.tri_stride, h->d_bp.as<const double>() + (size_t)sh * h->mc.tri_stride,
                                      sizeof(double) * tri_size(n), hipMemcpyDeviceToDevice, c->s_mc));
            HIP_TRY(c, hipMemcpyAsync(c->d_up.as<double>() + (size_t)sq * up_c, h->d_up.as<const double>() + (size_t)sh * up_h, sizeof(double) * (size_t)n * c->max_w,
                                      hipMemcpyDeviceToDevice, c->s_mc));
            HIP_TRY(c, hipMemcpyAsync(c->d_mclogz.as<double>() + sq, h->d_mclogz.as<const double>() + sh, sizeof(double), hipMemcpyDeviceToDevice, c->s_mc));
        }
        const int n1 = c->n[seq_of(c, P[k], 0)], n2 = c->n[seq_of(c, P[k], 1)];
        HIP_TRY(c, hipMemcpy2DAsync(c->d_hp.as<double>() + (size_t)P[k] * c->dx.tab_stride, sizeof(double) * c->dx.ldd,
                                    h->d_hp.as<const double>() + (size_t)k * h->dx.tab_stride, sizeof(double) * h->dx.ldd,
                                    sizeof(double) * (n2 + 1), (size_t)n1 + 1, hipMemcpyDeviceToDevice, c->s_mc));
        HIP_TRY(c, hipMemcpyAsync(c->d_logz.as<double>() + P[k], h->d_logz.as<const double>() + k, sizeof(double), hipMemcpyDeviceToDevice, c->s_mc));
    }
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    // what happened to them: held by another exponent on the helper's linear kernels (which = 2), or recomputed in log space (which = 0 / 1)
    c->last_path = 3;
    if (c->last_dx_path == 1 || c->last_dx_path == 0) c->last_dx_path = 3;
    c->rescaled_mc.clear(); c->fallback_mc.clear(); c->fallback_dx.clear();
    const bool h_log = h->last_went_log || h->last_path == 2 || (h->last_path == 3 && h->rescaled_mc.empty() && !h->fallback_mc.empty());
    for (int k = 0; k < nsub; k++) {
        const int sq1 = seq_of(c, P[k], 0), sq2 = seq_of(c, P[k], 1);
        if (h_log) { c->fallback_mc.push_back(sq1); c->fallback_mc.push_back(sq2); c->fallback_dx.push_back(P[k]); }
        else { c->rescaled_mc.push_back(sq1); c->rescaled_mc.push_back(sq2); }
    }
    c->tables_dirty = true;
    return RH_OK;
}

}  // namespace rh::host
