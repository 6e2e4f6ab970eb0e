// staging.hip -- sequence encoding, the upload of a batch and of its structure-constraint masks (allow_mask.hip): sizes and allocates
// every table the batch needs (buffers are kept and reused across batches of equal or smaller shape).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "constraint_prepass.h"
#include "ctx.h"
#include "kernels.h"

namespace rh::host {

// The per-letter values of `count` constraint strings (constraint_prepass.h), [count][lds] each, as allow_mask_build reads them
struct ConsPass {
    std::vector<uint8_t> ch;
    std::vector<int> P, enc;
    ConsPass(int count, int lds) : ch((size_t)count * lds, '.'), P((size_t)count * lds, 0), enc((size_t)count * lds, 0) {}
};

// The shares of the ns distinct sequences of an indexed batch in both roles (share_prepass; share role * ns + k), the open brackets
// of each, and why a share cannot stand in its role ("" = it can): O(letters of the distinct sequences), whatever the pairs.
struct SharePass {
    ConsPass L;
    std::vector<int> off, pos;
    std::vector<std::string> why;
    SharePass(int ns, int lds) : L(2 * ns, lds), off(1, 0), why(2 * (size_t)ns) {}
};

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

// Stage `ns` sequences; with_dx: pair p is (first[p], second[p]) of them, npairs pairs -- or, first == nullptr, the ns / 2 pairs
// (2p, 2p+1).  Allocates what is needed.  cons: per-sequence structure constraints of
// the single-molecule folds, co_cons: per-pair constraints over s1+s2 of the two-molecule ensemble (Vienna-BL; either, or any entry,
// may be nullptr).  An indexed batch takes its joint constraints by shares instead: pair p's is co_first[first[p]] over s1 +
// co_second[second[p]] over s2 (constraint_prepass.h), and its masks are composed on the device from one pass per distinct sequence
// and role.  Every constraint is checked before the context changes: a rejected upload leaves the previous batch in place.
int stage(rh_ctx* c, int ns, const char* const* seqs, const int* lens, bool with_mc, bool with_dx, const char* const* cons, const char* const* co_cons,
          int npairs, const int* first, const int* second, const char* const* co_first, const char* const* co_second)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (ns <= 0) return fail(c, RH_ERR_ARG, "empty batch");
    int nmax = 0, n1max = 0, n2max = 0;
    for (int k = 0; k < ns; k++) {
        if (lens[k] < 1) return fail(c, RH_ERR_ARG, "sequence %d has length %d (must be >= 1)", k, lens[k]);
        if (!seqs[k]) return fail(c, RH_ERR_ARG, "sequence %d is NULL", k);
        nmax = std::max(nmax, lens[k]);
    }
    const bool indexed = with_dx && first && second;
    if (with_dx && !indexed && (ns & 1)) return fail(c, RH_ERR_ARG, "duplex batch needs an even number of sequences");
    if (!indexed) npairs = with_dx ? ns / 2 : 0;
    if (indexed && npairs < 1) return fail(c, RH_ERR_ARG, "indexed batch of %d pairs (must be >= 1)", npairs);
    std::vector<int> pair_seq(2 * (size_t)npairs);
    int cut_min = 0, cut_max = 0;
    for (int p = 0; p < npairs; p++) {   // lengths over the pairs, through the index
        const int a = indexed ? first[p] : 2 * p, b = indexed ? second[p] : 2 * p + 1;
        if (a < 0 || a >= ns || b < 0 || b >= ns) return fail(c, RH_ERR_ARG, "pair %d = (%d, %d): index outside [0, %d)", p, a, b, ns);
        pair_seq[2 * (size_t)p] = a; pair_seq[2 * (size_t)p + 1] = b;
        n1max = std::max(n1max, lens[a]); n2max = std::max(n2max, lens[b]);
        cut_min = p == 0 ? lens[a] : std::min(cut_min, lens[a]);
        cut_max = p == 0 ? lens[a] : std::max(cut_max, lens[a]);
    }
    const int lds = (nmax + 3 + 15) & ~15;  // codes 0..n+2 readable
    const int co_lds = (n1max + n2max + 3 + 15) & ~15;
    const bool vienna = c->model == RH_MODEL_VIENNA_BL;
    if (!with_mc) cons = nullptr;
    if (indexed) co_cons = nullptr;   // (an indexed batch has no per-pair strings: its joint constraints come as shares)
    if (!with_dx || !vienna) co_cons = nullptr;
    if (!indexed || !vienna) co_first = co_second = nullptr;
    const bool shares = co_first || co_second;
    ConsPass H(cons ? ns : 0, lds), CH(co_cons ? npairs : 0, co_lds);
    std::string why;
    for (int k = 0; cons && k < ns; k++)
        if (!constraint_prepass(seqs[k], lens[k], cons[k], &H.ch[(size_t)k * lds], &H.P[(size_t)k * lds], &H.enc[(size_t)k * lds], &why))
            return fail(c, RH_ERR_ARG, "sequence %d: %s", k, why.c_str());
    for (int p = 0; co_cons && p < npairs; p++) {   // over the concatenation s1+s2 (one string of n1+n2 characters per pair)
        const std::string joint = std::string(seqs[2 * p], lens[2 * p]) + std::string(seqs[2 * p + 1], lens[2 * p + 1]);
        if (!constraint_prepass(joint.c_str(), (int)joint.size(), co_cons[p], &CH.ch[(size_t)p * co_lds], &CH.P[(size_t)p * co_lds],
                                &CH.enc[(size_t)p * co_lds], &why))
            return fail(c, RH_ERR_ARG, "pair %d: %s", p, why.c_str());
    }
    SharePass SH(shares ? ns : 0, lds);
    for (int r = 0; shares && r < 2; r++)
        for (int k = 0; k < ns; k++) {
            const char* const* from = r ? co_second : co_first;
            const size_t sh = (size_t)r * ns + k;
            std::vector<int> open;
            if (from && from[k] &&
                !share_prepass(seqs[k], lens[k], from[k], r, &SH.L.ch[sh * lds], &SH.L.P[sh * lds], &SH.L.enc[sh * lds], &open, &SH.why[sh]))
                open.clear();   // (reported below if a pair puts the sequence in this role; its row is not read otherwise)
            SH.pos.insert(SH.pos.end(), open.begin(), open.end());
            SH.off.push_back((int)SH.pos.size());
        }
    for (int p = 0; shares && p < npairs; p++) {   // per pair only what the partner decides: O(open brackets)
        const int a = pair_seq[2 * (size_t)p], b = ns + pair_seq[2 * (size_t)p + 1];
        for (int sh : {a, b})
            if (!SH.why[sh].empty()) return fail(c, RH_ERR_ARG, "pair %d: %s", p, SH.why[sh].c_str());
        if (!joint_pair_check(seqs[a], SH.pos.data() + SH.off[a], SH.off[a + 1] - SH.off[a], seqs[b - ns], SH.pos.data() + SH.off[b], SH.off[b + 1] - SH.off[b], &why))
            return fail(c, RH_ERR_ARG, "pair %d: %s", p, why.c_str());
    }
    c->ns = ns; c->np = npairs;
    c->pair_seq.swap(pair_seq); c->indexed = indexed;
    c->has_mc = with_mc; c->has_dx = with_dx; c->computed = false;
    c->n.assign(lens, lens + ns);

    std::vector<uint8_t> codes((size_t)ns * lds, vienna ? 0 : 4);   // sentinel = the model's "no nucleotide" code
    for (int k = 0; k < ns; k++)
        for (int i = 0; i < lens[k]; i++) codes[(size_t)k * lds + 1 + i] = vienna ? vienna_code(seqs[k][i]) : nuc_code(seqs[k][i]);
    int rc;
    if ((rc = ensure(c, c->d_seq, codes.size(), false))) return rc;
    if ((rc = ensure(c, c->d_n, sizeof(int) * ns, false))) return rc;
    c->h_codes = codes;
    HIP_TRY(c, hipMemcpyAsync(c->d_seq.p, codes.data(), codes.size(), hipMemcpyHostToDevice, c->s_mc));
    HIP_TRY(c, hipMemcpyAsync(c->d_n.p, lens, sizeof(int) * ns, hipMemcpyHostToDevice, c->s_mc));
    if (with_dx && c->pair_seq_dev != c->pair_seq) {
        c->pair_seq_dev.clear();
        if ((rc = ensure(c, c->d_pidx, sizeof(int) * 2 * npairs, false))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_pidx.p, c->pair_seq.data(), sizeof(int) * 2 * npairs, hipMemcpyHostToDevice, c->s_mc));
        c->pair_seq_dev = c->pair_seq;
    }
    c->small_list.clear();
    c->nmax_sweep = nmax;
    c->n_short = 0; c->nmax_short = 0;
    if (with_mc && !vienna && !cons) {
        std::vector<int> nsw(lens, lens + ns), nsh(ns, 0);
        int nmax_rest = 0;
        for (int k = 0; k < ns; k++) {
            if (c->small_on && lens[k] >= kSmallMin && lens[k] <= kSmallMax) { c->small_list.push_back(k); nsw[k] = 0; }
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
            HIP_TRY(c, hipStreamSynchronize(c->s_mc));   // (the staging vectors die with this scope)
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));  // host staging buffers die with this scope

    if (with_mc) {
        McBatch& B = c->mc;
        B.ns = ns; B.nmax = nmax; B.lds = lds;
        B.ld = (nmax + 2 + 1) & ~1;
        B.tab_stride = (size_t)B.ld * B.ld;
        B.seq_stride = B.tab_stride * (vienna ? (int)VM_COUNT : (int)T_COUNT);
        B.tri_stride = (tri_size(nmax) + 1) & ~(size_t)1;
        if ((rc = ensure(c, c->d_mctab, sizeof(double) * B.seq_stride * ns, false))) return rc;
        B.nb = (nmax - 1) / 16 + 1;
        B.pk_stride = (size_t)B.nb * (B.nb + 1) / 2 * 256;
        if ((rc = ensure(c, c->d_pk, sizeof(double) * B.pk_stride * kPkCopies * ns, false))) return rc;
        B.pk = c->d_pk.as<double>();
        if ((rc = ensure(c, c->d_rowp, sizeof(double) * 4 * B.ld * ns, false))) return rc;
        B.rowp = c->d_rowp.as<double>();
        if ((rc = ensure(c, c->d_f5, sizeof(double) * 2 * B.ld * ns, false))) return rc;
        if ((rc = ensure(c, c->d_up, sizeof(double) * B.ld * c->max_w * ns, false))) return rc;
        // gap probabilities [2 ns][32][ld] + the chunk sums of the gap lengths 1, 2 [8][2 ns][2][ld] (launch_mc_vlin)
        if (vienna && (rc = ensure(c, c->d_gaps, sizeof(double) * (2 * 32 + 8 * 2 * 2) * B.ld * ns, false))) return rc;
        if (vienna) {
            const VLinModel& H = *c->h_vlin;
            c->h_hplen.resize((size_t)B.ld);
            for (int d = 0; d < B.ld; d++)   // hairpin of d unpaired letters: length weight (beyond 30 as part_func.c extrapolates) x lam^d
                c->h_hplen[d] = (d <= 30 ? H.E_hairpin[d] : std::exp(H.hairpin30 - H.lxc * std::log(d / 30.0))) * std::exp(-H.s * d);
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
        B.allow = nullptr;
        if (cons) {
            if ((rc = build_allow_masks(c, &H, nullptr, ns, B.ld, lds, c->d_n.as<const int>(), c->d_allow))) return rc;
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
        B.tab = c->d_mctab.as<double>();
        B.f5i = c->d_f5.as<double>(); B.f5o = c->d_f5.as<double>() + (size_t)B.ld * ns;
        B.bp = c->d_bp.as<double>(); B.up = c->d_up.as<double>();
    }
    if (with_dx) {
        DxBatch& D = c->dx;
        c->co.allow = nullptr;   // (under RH_HYBRID_DUPLEX nothing below rebuilds c->co: a joint mask of an earlier batch must not be seen)
        D.np = npairs; D.n1max = n1max; D.n2max = n2max; D.lds = lds;
        D.ldd = (n2max + 2 + 1) & ~1;
        D.tab_stride = (size_t)(n1max + 2) * D.ldd;
        D.pair_stride = D.tab_stride * std::max((int)D_COUNT, (int)V_COUNT);   // 4 tables (CONTRAfold model) or 6 (Vienna model: IN/OUT + two decorated copies each)
        // the linear path keeps anti-diagonal-major tables in the same buffer (sequential use)
        DxLinBatch& X = c->dxl;
        X.np = D.np; X.n1max = n1max; X.n2max = n2max; X.lds = lds; X.ldd = D.ldd;
        X.lda = (n1max + 2 + 2 * kDxPad + 1) & ~1;
        const size_t rows = (size_t)n1max + n2max + 3;
        X.tab_stride = rows * X.lda + 128;   // slack: the staged 96-column segments may run past the last row
        // Vienna-BL: raw + two decorated copies per direction; 2.x semantics: two more copies each (mismatch1nI, mismatch23I) -- sized
        // by the context, not by rh_set_duplex_mode, which may change between upload and compute: a 2.x context that stays on the
        // log-space kernels pays for it with a larger buffer and clear (10 linear tables against the 6 log-space ones, whichever is larger)
        X.pair_stride = X.tab_stride * (!vienna ? (int)DL_COUNT : c->vienna_sem == kViennaSem20 ? (int)VD_COUNT20 : (int)VD_COUNT);
        const size_t dx_bytes = sizeof(double) * std::max(D.pair_stride, X.pair_stride) * D.np;
        void* before = c->d_dxtab.p;
        if ((rc = ensure(c, c->d_dxtab, dx_bytes, false))) return rc;
        const size_t layout = ((size_t)X.lda << 32) ^ rows ^ ((size_t)D.np << 48);
        if (c->d_dxtab.p != before || layout != c->dxl_layout || c->last_dx_path != 1) {
            // pad columns must be zero and a different layout (or the log-space path) leaves arbitrary bytes there
            HIP_TRY(c, hipMemsetAsync(c->d_dxtab.p, 0, dx_bytes, c->s_dx));
            c->dxl_layout = layout;
            c->dxtab_log = false;
        }
        c->dx_bytes = dx_bytes;
        if ((rc = ensure(c, c->d_dxbad, sizeof(int) * D.np, false))) return rc;
        if ((rc = ensure(c, c->d_zbar, sizeof(double) * D.np, false))) return rc;
        c->lz_chunks = (n1max + n2max - 1 + 15) / 16;   // kLzRows anti-diagonals per chunk
        if ((rc = ensure(c, c->d_zpart, (sizeof(double) + sizeof(int)) * (size_t)D.np * c->lz_chunks, false))) return rc;
        if ((rc = ensure(c, c->d_logz, sizeof(double) * D.np, false))) return rc;
        const size_t hp_bytes = sizeof(double) * D.tab_stride * D.np;
        if ((rc = ensure(c, c->d_hp, hp_bytes, false))) return rc;
        // the pair-major image the duplex kernels read, and (below) the joint image of the two-molecule ensemble: built on the device
        // from the distinct sequences, which are on it once (the copies on s_mc above are complete)
        PairImage G{};
        bool gathered = false;
        if ((rc = ensure(c, c->d_pseq, 2 * (size_t)npairs * lds, false))) return rc;
        if ((rc = ensure(c, c->d_pn, sizeof(int) * 2 * npairs, false))) return rc;
        G.seq = c->d_seq.as<const uint8_t>(); G.n = c->d_n.as<const int>(); G.idx = c->d_pidx.as<const int>();
        G.pseq = c->d_pseq.as<uint8_t>(); G.pn = c->d_pn.as<int>(); G.np = npairs; G.lds = lds;
        D.seq = c->d_pseq.as<const uint8_t>(); D.n = c->d_pn.as<const int>();
        D.tab = c->d_dxtab.as<double>(); D.hp = c->d_hp.as<double>(); D.logz = c->d_logz.as<double>();
        if (vienna && c->hybrid == RH_HYBRID_COFOLD) {
            // concatenated sequences s1+s2, cut after s1
            McBatch& C = c->co;
            const int np = npairs, cmax = n1max + n2max;
            C = McBatch{};
            C.ns = np; C.nmax = cmax;
            C.lds = (cmax + 3 + 15) & ~15;
            C.ld = (cmax + 2 + 1) & ~1;
            C.tab_stride = (size_t)C.ld * C.ld;
            C.seq_stride = C.tab_stride * (int)VM_COUNT;
            C.tri_stride = (tri_size(cmax) + 1) & ~(size_t)1;
            c->co_cut_min = cut_min; c->co_cut_max = cut_max;
            if ((rc = ensure(c, c->d_coseq, (size_t)np * C.lds, false))) return rc;
            if ((rc = ensure(c, c->d_con, sizeof(int) * 2 * np, false))) return rc;
            G.coseq = c->d_coseq.as<uint8_t>(); G.con = c->d_con.as<int>(); G.co_lds = C.lds;   // concatenated codes, lengths and cuts: pair_gather
            if ((rc = ensure(c, c->d_cotab, sizeof(double) * C.seq_stride * np, false))) return rc;
            C.nb = (cmax - 1) / 16 + 1;
            C.pk_stride = (size_t)C.nb * (C.nb + 1) / 2 * 256;
            if ((rc = ensure(c, c->d_copk, sizeof(double) * C.pk_stride * kPkCopies * np, false))) return rc;
            C.pk = c->d_copk.as<double>();
            if ((rc = ensure(c, c->d_corowp, sizeof(double) * 4 * C.ld * np, false))) return rc;
            C.rowp = c->d_corowp.as<double>();
            if ((rc = ensure(c, c->d_cof5, sizeof(double) * 6 * C.ld * np, false))) return rc;
            if ((rc = ensure(c, c->d_cobp, sizeof(double) * C.tri_stride * np, false))) return rc;
            if ((rc = ensure(c, c->d_cobad, sizeof(int) * np, false))) return rc;
            if ((int)c->h_hplen.size() < C.ld) {   // hairpin length weights up to the joint length (see the single-molecule batch)
                const VLinModel& H = *c->h_vlin;
                c->h_hplen.resize((size_t)C.ld);
                for (int d = 0; d < C.ld; d++)
                    c->h_hplen[d] = (d <= 30 ? H.E_hairpin[d] : std::exp(H.hairpin30 - H.lxc * std::log(d / 30.0))) * std::exp(-H.s * d);
            }
            C.seq = c->d_coseq.as<const uint8_t>(); C.n = c->d_con.as<const int>(); C.cut = c->d_con.as<const int>() + np;
            C.tab = c->d_cotab.as<double>();
            double* f = c->d_cof5.as<double>();
            const size_t fs = (size_t)C.ld * np;
            C.f5i = f; C.f5o = f + fs; C.xp = f + 2 * fs; C.xs = f + 3 * fs; C.xpo = f + 4 * fs; C.xso = f + 5 * fs;
            C.bp = c->d_cobp.as<double>(); C.up = nullptr;
            JointShares S{};
            std::vector<int> blob;   // (dies with this scope: build_allow_masks synchronizes s_mc)
            if (shares) {
                // the shares go over once per distinct sequence and role, in one copy: P, enc, the open lists, then the characters
                const size_t cells = 2 * (size_t)ns * lds, ints = 2 * cells + SH.off.size() + SH.pos.size();
                blob.resize(ints + (cells + sizeof(int) - 1) / sizeof(int));
                std::copy(SH.L.P.begin(), SH.L.P.end(), blob.begin());
                std::copy(SH.L.enc.begin(), SH.L.enc.end(), blob.begin() + cells);
                std::copy(SH.off.begin(), SH.off.end(), blob.begin() + 2 * cells);
                std::copy(SH.pos.begin(), SH.pos.end(), blob.begin() + 2 * cells + SH.off.size());
                std::memcpy(blob.data() + ints, SH.L.ch.data(), cells);
                if ((rc = ensure(c, c->d_share, blob.size() * sizeof(int), false))) return rc;
                HIP_TRY(c, hipMemcpyAsync(c->d_share.p, blob.data(), blob.size() * sizeof(int), hipMemcpyHostToDevice, c->s_mc));
                const int* d = c->d_share.as<const int>();
                S.P = d; S.enc = d + cells; S.open_off = d + 2 * cells; S.open_pos = S.open_off + SH.off.size();
                S.ch = reinterpret_cast<const uint8_t*>(d + ints);
                S.idx = c->d_pidx.as<const int>(); S.con = c->d_con.as<const int>();
                S.ns = ns; S.np = np; S.lds = lds; S.co_lds = co_lds;
            }
            if (co_cons || shares) {
                hipLaunchKernelGGL(pair_gather, dim3(npairs, 2), dim3(kPairGatherThreads), 0, c->s_dx, G);   // (the kernels on s_mc read the joint lengths)
                HIP_TRY(c, hipStreamSynchronize(c->s_dx));
                gathered = true;
                if ((rc = build_allow_masks(c, co_cons ? &CH : nullptr, &S, np, C.ld, co_lds, C.n, c->d_coallow))) return rc;
                C.allow = c->d_coallow.as<const uint8_t>();
            }
        }
        if (!gathered) hipLaunchKernelGGL(pair_gather, dim3(npairs, 2), dim3(kPairGatherThreads), 0, c->s_dx, G);
        HIP_TRY(c, hipGetLastError());
        // row 0, column 0 and what lies beyond L1 / L2 stay zero.  CONTRAfold model: every path stores all of 1..L1 x 1..L2 (see
        // dx_hp_clear_rest), so only the rest is zeroed -- behind pair_gather, which writes the pair-major lengths that kernel reads.
        // Vienna-BL keeps the whole clear: its hp also comes from the two-molecule ensemble (cofold) and from the helper context, which
        // copy or store parts of the matrix only.
        if (vienna) HIP_TRY(c, hipMemsetAsync(c->d_hp.p, 0, hp_bytes, c->s_dx));
        else hipLaunchKernelGGL(dx_hp_clear_rest, dim3(16, D.np), dim3(256), 0, c->s_dx, D);
        X.seq = D.seq; X.n = D.n; X.tab = D.tab; X.hp = D.hp; X.hp_stride = D.tab_stride;
    }
    return RH_OK;
}

}  // namespace rh::host
