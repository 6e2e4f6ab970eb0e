// staging.hip -- the upload of a checked request (batch_request.h) and of its structure-constraint masks (allow_mask.hip): allocates
// every table the batch needs, sized by the layout functions of batch.h (buffers are kept and reused across batches of equal or
// smaller shape).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "kernels.h"

namespace rh::host {

// The masks [count][ld][ld] of one batch, built on the device from the per-letter values [count][lds]: H, the host pass over the
// batch's own strings (three small asynchronous copies), or, H == nullptr, the rows joint_cons_gather composes from the shares S of
// an indexed batch; then one launch on s_mc, in front of the sweeps.  d_n: the lengths on the device.  The kernel writes every
// byte of the image.
static int build_allow_masks(rh_ctx* c, const ConsPass* H, const JointShares* S, int count, int ld, int lds, const int* d_n, DevBuf& d_mask)
{
    int rc;
    const size_t cells = (size_t)count * lds;
    if ((rc = ensure(c, d_mask, (size_t)count * ld * ld, false))) return rc;
    if ((rc = ensure(c, c->d_cons, cells * (2 * sizeof(int) + 1), false))) return rc;
    int* d_P = c->d_cons.as<int>();
    int* d_enc = d_P + cells;
    uint8_t* d_ch = reinterpret_cast<uint8_t*>(d_enc + cells);
    if (H) {
        HIP_TRY(c, hipMemcpyAsync(d_P, H->P.data(), cells * sizeof(int), hipMemcpyHostToDevice, c->s_mc));
        HIP_TRY(c, hipMemcpyAsync(d_enc, H->enc.data(), cells * sizeof(int), hipMemcpyHostToDevice, c->s_mc));
        HIP_TRY(c, hipMemcpyAsync(d_ch, H->ch.data(), cells, hipMemcpyHostToDevice, c->s_mc));
    } else {
        hipLaunchKernelGGL(joint_cons_gather, dim3(count), dim3(kJointGatherThreads), 0, c->s_mc, *S, d_ch, d_P, d_enc);
        HIP_TRY(c, hipGetLastError());
    }
    const size_t lds_bytes = (size_t)lds * (2 * sizeof(int) + 1);
    const int in_lds = lds_bytes <= 64 * 1024;   // longer sequences: the kernel reads the three arrays from global memory
    hipLaunchKernelGGL(allow_mask_build, dim3(count, (ld + kAllowRows - 1) / kAllowRows), dim3(kAllowThreads), in_lds ? lds_bytes : 0, c->s_mc,
                       d_mask.as<uint8_t>(), d_n, d_ch, d_P, d_enc, ld, lds, in_lds);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));   // (the host arrays of the copies die with the caller's scope)
    return RH_OK;
}

// The codes, lengths and index of the request on the device, and the per-sequence routing of the CONTRAfold-model sweeps (the short
// sequences of a batch that runs in strips, the one-workgroup folds): all of it belongs to this upload and to nothing before it.
static int stage_sequences(rh_ctx* c, const BatchRequest& r, const BatchShape& S, bool vienna)
{
    const int ns = r.ns;
    const int* lens = r.lens;
    int rc;
    if ((rc = ensure(c, c->d_seq, S.codes.size(), false))) return rc;
    if ((rc = ensure(c, c->d_n, sizeof(int) * ns, false))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_seq.p, S.codes.data(), S.codes.size(), hipMemcpyHostToDevice, c->s_mc));
    HIP_TRY(c, hipMemcpyAsync(c->d_n.p, lens, sizeof(int) * ns, hipMemcpyHostToDevice, c->s_mc));
    if (r.with_dx && c->pair_seq_dev != S.pair_seq) {
        c->pair_seq_dev.clear();
        if ((rc = ensure(c, c->d_pidx, sizeof(int) * 2 * S.np, false))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_pidx.p, S.pair_seq.data(), sizeof(int) * 2 * S.np, hipMemcpyHostToDevice, c->s_mc));
        c->pair_seq_dev = S.pair_seq;
    }
    c->small_list.clear();
    c->nmax_sweep = S.nmax;
    c->n_short = 0; c->nmax_short = 0;
    std::vector<int> nsw, nsh;
    if (r.with_mc && !vienna && !S.has_fold) {
        nsw.assign(lens, lens + ns); nsh.assign(ns, 0);
        int nmax_rest = 0;
        for (int k = 0; k < ns; k++) {
            if (c->small_on && !(c->region_acc && c->max_w > 1) && lens[k] >= kSmallMin && lens[k] <= kSmallMax) { c->small_list.push_back(k); nsw[k] = 0; }
            else nmax_rest = std::max(nmax_rest, lens[k]);
        }
        if (nmax_rest >= kStripMinN)   // some sequence runs in strips: the ones below that length get their own pass
            for (int k = 0; k < ns; k++)
                if (nsw[k] > 0 && nsw[k] < kStripMinN) { nsh[k] = nsw[k]; nsw[k] = 0; c->n_short++; c->nmax_short = std::max(c->nmax_short, nsh[k]); }
        c->nmax_sweep = 0;
        for (int k = 0; k < ns; k++) c->nmax_sweep = std::max(c->nmax_sweep, nsw[k]);
        if (!c->small_list.empty() || c->n_short) {
            // longest first: one workgroup occupies a CU, and workgroups of alternating cost land on alternating CUs
            std::stable_sort(c->small_list.begin(), c->small_list.end(), [&](int a, int b) { return lens[a] > lens[b]; });
            if ((rc = ensure(c, c->d_small_list, sizeof(int) * ns, false))) return rc;
            if ((rc = ensure(c, c->d_n_sweep, sizeof(int) * ns, false))) return rc;
            if ((rc = ensure(c, c->d_n_short, sizeof(int) * ns, false))) return rc;
            if (!c->small_list.empty())
                HIP_TRY(c, hipMemcpyAsync(c->d_small_list.p, c->small_list.data(), sizeof(int) * c->small_list.size(), hipMemcpyHostToDevice, c->s_mc));
            HIP_TRY(c, hipMemcpyAsync(c->d_n_sweep.p, nsw.data(), sizeof(int) * ns, hipMemcpyHostToDevice, c->s_mc));
            HIP_TRY(c, hipMemcpyAsync(c->d_n_short.p, nsh.data(), sizeof(int) * ns, hipMemcpyHostToDevice, c->s_mc));
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));   // (the caller's arrays and the routing vectors are free again)
    return RH_OK;
}

// The single-molecule folds: c->mc, its tables and result buffers, the hairpin length weights and the masks of the fold constraints
static int stage_folds(rh_ctx* c, const BatchShape& S, int ns, bool vienna)
{
    int rc;
    McBatch& B = c->mc;
    B = mc_layout(ns, S.nmax, vienna ? (int)VM_COUNT : (int)T_COUNT);
    if ((rc = ensure(c, c->d_mctab, sizeof(double) * B.seq_stride * ns, false))) return rc;
    if ((rc = ensure(c, c->d_pk, sizeof(double) * B.pk_stride * kPkCopies * ns, false))) return rc;
    if ((rc = ensure(c, c->d_rowp, sizeof(double) * 4 * B.ld * ns, false))) return rc;
    if ((rc = ensure(c, c->d_f5, sizeof(double) * 2 * B.ld * ns, false))) return rc;
    if ((rc = ensure(c, c->d_up, sizeof(double) * B.ld * c->max_w * ns, false))) return rc;
    // gap probabilities [2 ns][32][ld] + the chunk sums of the gap lengths 1, 2 [8][2 ns][2][ld] (launch_mc_vlin)
    if (vienna && (rc = ensure(c, c->d_gaps, sizeof(double) * (2 * 32 + 8 * 2 * 2) * B.ld * ns, false))) return rc;
    if (vienna) {
        c->h_hplen.resize((size_t)B.ld);
        hairpin_length_weights(*c->h_vlin, B.ld, c->h_hplen.data());
        if ((rc = ensure(c, c->d_hplen, sizeof(double) * B.ld, false))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_hplen.p, c->h_hplen.data(), sizeof(double) * B.ld, hipMemcpyHostToDevice, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    }
    if ((rc = ensure(c, c->d_mclogz, sizeof(double) * ns, false))) return rc;
    if ((rc = ensure(c, c->d_bad, sizeof(int) * ns, false))) return rc;
    // bp entries outside 1<=i<j<=n are never written by the sweep: keep them zero
    const size_t bp_bytes = sizeof(double) * B.tri_stride * ns;
    if ((rc = ensure(c, c->d_bp, bp_bytes, false))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_bp.p, 0, bp_bytes, c->s_mc));
    if (S.has_fold) {
        if ((rc = build_allow_masks(c, &S.fold, nullptr, ns, B.ld, S.lds, c->d_n.as<const int>(), c->d_allow))) return rc;
        B.allow = c->d_allow.as<const uint8_t>();
    }
    if (c->tables_dirty) {
        // a problem of the previous batch overflowed: its tables hold Inf / NaN, which a later batch must never meet even in
        // cells it masks (0 x Inf).  One clear per such batch; ordinary batches reuse the tables as they are.
        HIP_TRY(c, hipMemsetAsync(c->d_mctab.p, 0, c->d_mctab.cap, c->s_mc));
        if (c->d_pk) HIP_TRY(c, hipMemsetAsync(c->d_pk.p, 0, c->d_pk.cap, c->s_mc));
        if (c->d_cotab) HIP_TRY(c, hipMemsetAsync(c->d_cotab.p, 0, c->d_cotab.cap, c->s_mc));
        if (c->d_copk) HIP_TRY(c, hipMemsetAsync(c->d_copk.p, 0, c->d_copk.cap, c->s_mc));
        c->tables_dirty = false;
    }
    B.seq = c->d_seq.as<const uint8_t>(); B.n = c->d_n.as<const int>();
    B.tab = c->d_mctab.as<double>(); B.pk = c->d_pk.as<double>(); B.rowp = c->d_rowp.as<double>();
    B.f5i = c->d_f5.as<double>(); B.f5o = c->d_f5.as<double>() + (size_t)B.ld * ns;
    B.bp = c->d_bp.as<double>(); B.up = c->d_up.as<double>();
    return RH_OK;
}

// The pairs: c->dx and c->dxl (log-space and anti-diagonal-major tables in one buffer, used one after the other), the result buffers,
// and the image *G that pair_gather fills -- launched by finish_pairs, behind stage_joint where there is one
static int stage_pairs(rh_ctx* c, const BatchShape& S, bool vienna, PairImage* G)
{
    int rc;
    const int np = S.np;
    c->co.allow = nullptr;   // (under RH_HYBRID_DUPLEX nothing rebuilds c->co: a joint mask of an earlier batch must not be seen)
    DxBatch& D = c->dx;
    D = dx_layout(np, S.n1max, S.n2max, S.lds, std::max((int)D_COUNT, (int)V_COUNT));   // 4 tables (CONTRAfold model) or 6 (Vienna model: IN/OUT + two decorated copies each)
    // Vienna-BL: raw + two decorated copies per direction; 2.x semantics: two more copies each (mismatch1nI, mismatch23I) -- sized
    // by the context, not by rh_set_duplex_mode, which may change between upload and compute: a 2.x context that stays on the
    // log-space kernels pays for it with a larger buffer and clear (10 linear tables against the 6 log-space ones, whichever is larger)
    DxLinBatch& X = c->dxl;
    X = dxl_layout(np, S.n1max, S.n2max, S.lds, D.ldd, !vienna ? (int)DL_COUNT : c->vienna_sem == kViennaSem20 ? (int)VD_COUNT20 : (int)VD_COUNT);
    const size_t dx_bytes = sizeof(double) * std::max(D.pair_stride, X.pair_stride) * np;
    void* before = c->d_dxtab.p;
    if ((rc = ensure(c, c->d_dxtab, dx_bytes, false))) return rc;
    const size_t layout = ((size_t)X.lda << 32) ^ ((size_t)S.n1max + S.n2max + 3) ^ ((size_t)np << 48);
    if (c->d_dxtab.p != before || layout != c->dxl_layout || c->last_dx_path != 1) {
        // pad columns must be zero and a different layout (or the log-space path) leaves arbitrary bytes there
        HIP_TRY(c, hipMemsetAsync(c->d_dxtab.p, 0, dx_bytes, c->s_dx));
        c->dxl_layout = layout;
        c->dxtab_log = false;
    }
    c->dx_bytes = dx_bytes;
    if ((rc = ensure(c, c->d_dxbad, sizeof(int) * np, false))) return rc;
    if ((rc = ensure(c, c->d_zbar, sizeof(double) * np, false))) return rc;
    c->lz_chunks = lz_chunks(S.n1max, S.n2max);
    if ((rc = ensure(c, c->d_zpart, (sizeof(double) + sizeof(int)) * (size_t)np * c->lz_chunks, false))) return rc;
    if ((rc = ensure(c, c->d_logz, sizeof(double) * np, false))) return rc;
    if ((rc = ensure(c, c->d_hp, sizeof(double) * D.tab_stride * np, false))) return rc;
    // the pair-major image the duplex kernels read: built on the device from the distinct sequences, which are on it once (the
    // copies of stage_sequences are complete)
    if ((rc = ensure(c, c->d_pseq, 2 * (size_t)np * S.lds, false))) return rc;
    if ((rc = ensure(c, c->d_pn, sizeof(int) * 2 * np, false))) return rc;
    G->seq = c->d_seq.as<const uint8_t>(); G->n = c->d_n.as<const int>(); G->idx = c->d_pidx.as<const int>();
    G->pseq = c->d_pseq.as<uint8_t>(); G->pn = c->d_pn.as<int>(); G->np = np; G->lds = S.lds;
    D.seq = c->d_pseq.as<const uint8_t>(); D.n = c->d_pn.as<const int>();
    D.tab = c->d_dxtab.as<double>(); D.hp = c->d_hp.as<double>(); D.logz = c->d_logz.as<double>();
    X.seq = D.seq; X.n = D.n; X.tab = D.tab; X.hp = D.hp; X.hp_stride = D.tab_stride;
    return RH_OK;
}

// The shares of an indexed batch on the device, in one copy: P, enc, the open lists, then the characters.  *blob is what the copy
// reads: it lives until the caller has synchronized s_mc (build_allow_masks does).
static int upload_shares(rh_ctx* c, const BatchShape& S, int ns, std::vector<int>* blob, JointShares* J)
{
    const SharePass& SH = S.share;
    const size_t cells = 2 * (size_t)ns * S.lds, ints = 2 * cells + SH.off.size() + SH.pos.size();
    blob->resize(ints + (cells + sizeof(int) - 1) / sizeof(int));
    std::copy(SH.L.P.begin(), SH.L.P.end(), blob->begin());
    std::copy(SH.L.enc.begin(), SH.L.enc.end(), blob->begin() + cells);
    std::copy(SH.off.begin(), SH.off.end(), blob->begin() + 2 * cells);
    std::copy(SH.pos.begin(), SH.pos.end(), blob->begin() + 2 * cells + SH.off.size());
    std::memcpy(blob->data() + ints, SH.L.ch.data(), cells);
    if (int rc = ensure(c, c->d_share, blob->size() * sizeof(int), false)) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_share.p, blob->data(), blob->size() * sizeof(int), hipMemcpyHostToDevice, c->s_mc));
    const int* d = c->d_share.as<const int>();
    J->P = d; J->enc = d + cells; J->open_off = d + 2 * cells; J->open_pos = J->open_off + SH.off.size();
    J->ch = reinterpret_cast<const uint8_t*>(d + ints);
    J->idx = c->d_pidx.as<const int>(); J->con = c->d_con.as<const int>();
    J->ns = ns; J->np = S.np; J->lds = S.lds; J->co_lds = S.co_lds;
    return RH_OK;
}

// The two-molecule ensemble (Vienna-BL, RH_HYBRID_COFOLD): c->co over the concatenations s1+s2, cut after s1, and the masks of the
// joint constraints -- from the per-pair strings of a plain batch or composed on the device from the shares of an indexed one.
// The masks read the joint lengths, so with them pair_gather runs here (*gathered) instead of in finish_pairs.
static int stage_joint(rh_ctx* c, const BatchShape& S, int ns, PairImage* G, bool* gathered)
{
    int rc;
    const int np = S.np;
    McBatch& C = c->co;
    C = mc_layout(np, S.n1max + S.n2max, (int)VM_COUNT);
    c->co_cut_min = S.cut_min; c->co_cut_max = S.cut_max;
    if ((rc = ensure(c, c->d_coseq, (size_t)np * C.lds, false))) return rc;
    if ((rc = ensure(c, c->d_con, sizeof(int) * 2 * np, false))) return rc;
    G->coseq = c->d_coseq.as<uint8_t>(); G->con = c->d_con.as<int>(); G->co_lds = C.lds;   // concatenated codes, lengths and cuts: pair_gather
    if ((rc = ensure(c, c->d_cotab, sizeof(double) * C.seq_stride * np, false))) return rc;
    if ((rc = ensure(c, c->d_copk, sizeof(double) * C.pk_stride * kPkCopies * np, false))) return rc;
    if ((rc = ensure(c, c->d_corowp, sizeof(double) * 4 * C.ld * np, false))) return rc;
    if ((rc = ensure(c, c->d_cof5, sizeof(double) * 6 * C.ld * np, false))) return rc;
    if ((rc = ensure(c, c->d_cobp, sizeof(double) * C.tri_stride * np, false))) return rc;
    if ((rc = ensure(c, c->d_cobad, sizeof(int) * np, false))) return rc;
    if ((int)c->h_hplen.size() < C.ld) {   // hairpin length weights up to the joint length (see the single-molecule batch)
        c->h_hplen.resize((size_t)C.ld);
        hairpin_length_weights(*c->h_vlin, C.ld, c->h_hplen.data());
    }
    C.seq = c->d_coseq.as<const uint8_t>(); C.n = c->d_con.as<const int>(); C.cut = c->d_con.as<const int>() + np;
    C.tab = c->d_cotab.as<double>(); C.pk = c->d_copk.as<double>(); C.rowp = c->d_corowp.as<double>();
    double* f = c->d_cof5.as<double>();
    const size_t fs = (size_t)C.ld * np;
    C.f5i = f; C.f5o = f + fs; C.xp = f + 2 * fs; C.xs = f + 3 * fs; C.xpo = f + 4 * fs; C.xso = f + 5 * fs;
    C.bp = c->d_cobp.as<double>();
    if (!S.has_joint && !S.has_shares) return RH_OK;
    JointShares J{};
    std::vector<int> blob;
    if (S.has_shares && (rc = upload_shares(c, S, ns, &blob, &J))) return rc;
    hipLaunchKernelGGL(pair_gather, dim3(np, 2), dim3(kPairGatherThreads), 0, c->s_dx, *G);   // (the kernels on s_mc read the joint lengths)
    HIP_TRY(c, hipStreamSynchronize(c->s_dx));
    *gathered = true;
    if ((rc = build_allow_masks(c, S.has_joint ? &S.joint : nullptr, &J, np, C.ld, S.co_lds, C.n, c->d_coallow))) return rc;
    C.allow = c->d_coallow.as<const uint8_t>();
    return RH_OK;
}

// pair_gather, unless stage_joint has run it, and the clear of hp behind it
static int finish_pairs(rh_ctx* c, const PairImage& G, bool gathered, bool vienna)
{
    const DxBatch& D = c->dx;
    if (!gathered) hipLaunchKernelGGL(pair_gather, dim3(D.np, 2), dim3(kPairGatherThreads), 0, c->s_dx, G);
    HIP_TRY(c, hipGetLastError());
    // row 0, column 0 and what lies beyond L1 / L2 stay zero.  CONTRAfold model: every path stores all of 1..L1 x 1..L2 (see
    // dx_hp_clear_rest), so only the rest is zeroed -- behind pair_gather, which writes the pair-major lengths that kernel reads.
    // Vienna-BL keeps the whole clear: its hp also comes from the two-molecule ensemble (cofold) and from the helper context, which
    // copy or store parts of the matrix only.
    if (vienna) HIP_TRY(c, hipMemsetAsync(c->d_hp.p, 0, sizeof(double) * D.tab_stride * D.np, c->s_dx));
    else hipLaunchKernelGGL(dx_hp_clear_rest, dim3(16, D.np), dim3(256), 0, c->s_dx, D);
    return RH_OK;
}

// Stage a request: check it (check_batch: nothing of the context is touched, a rejected request leaves the previous batch in place and
// fetchable), take the previous batch out of the context, allocate and fill what the request needs -- sequences, folds, pairs, the
// two-molecule ensemble -- and publish the new batch as the last statement.  In between the context holds no batch: a failure there
// (RH_ERR_OOM from ensure(), a HIP error) leaves ns = np = 0, and the next upload behaves as on a context that never failed.
int stage(rh_ctx* c, const BatchRequest& r)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const bool vienna = c->model == RH_MODEL_VIENNA_BL;
    BatchShape S;
    std::string why;
    int rc;
    if ((rc = check_batch(r, vienna, &S, &why))) return fail(c, rc, "%s", why.c_str());
    c->ns = c->np = 0;
    c->has_mc = c->has_dx = c->computed = false;
    if ((rc = stage_sequences(c, r, S, vienna))) return rc;
    if (r.with_mc && (rc = stage_folds(c, S, r.ns, vienna))) return rc;
    if (r.with_dx) {
        PairImage G{};
        bool gathered = false;
        if ((rc = stage_pairs(c, S, vienna, &G))) return rc;
        if (vienna && c->hybrid == RH_HYBRID_COFOLD && (rc = stage_joint(c, S, r.ns, &G, &gathered))) return rc;
        if ((rc = finish_pairs(c, G, gathered, vienna))) return rc;
    }
    c->n.assign(r.lens, r.lens + r.ns);
    c->h_codes.swap(S.codes);
    c->pair_seq.swap(S.pair_seq); c->indexed = S.indexed;
    c->has_mc = r.with_mc; c->has_dx = r.with_dx;
    c->ns = r.ns; c->np = S.np;
    return RH_OK;
}

}  // namespace rh::host

