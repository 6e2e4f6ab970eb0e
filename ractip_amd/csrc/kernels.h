// kernels.h -- the one declaration of every __global__ kernel and cross-file launch helper of the library.
// Every .hip file that defines a kernel includes it, and so does every host unit that launches one: the compiler
// checks each definition (and each explicit instantiation) against the declaration here.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ractip_hot.h"
#include "batch.h"
#include "score_model.h"
#include "lin_model.h"
#include "vienna_model.h"

namespace rh {
__global__ void mc_init(McBatch B);
__global__ void mc_inside_diag(McBatch B, const ScoreModel* __restrict__ M, int d, int pin);
__global__ void mc_outside_diag(McBatch B, const ScoreModel* __restrict__ M, int d, int pin);
__global__ void mc_unpaired(McBatch B, int max_w);   // writes column 0 of up[.][max_w]
// mccaskill_acc.hip: region accessibility of the CONTRAfold model, widths 2..max_w, from the finished tables.  PATH 0: the scaled
// linear tables (A.lin), PATH 1: the log-space tables (A.score).  Scratch per sequence: three square tables and the gap weights.
struct AccArgs {
    const LinModel* lin;
    const ScoreModel* score;
    double* scratch;   // [ns][acc_scratch_doubles(ld)]
    int max_w, pad_;
};
constexpr int kAccTile = 64, kAccK = 16;   // cf_acc_link: output tile, K tile
constexpr size_t acc_scratch_doubles(int ld) { return 3 * (size_t)ld * ld + 2 * 31 * (size_t)ld; }
template <int PATH> __global__ void cf_acc_hrows(McBatch B, AccArgs A);
template <int PATH> __global__ void cf_acc_hcols(McBatch B, AccArgs A);
template <int PATH> __global__ void cf_acc_gaps(McBatch B, AccArgs A);
template <int PATH> __global__ void cf_acc_final(McBatch B, AccArgs A);
template <int PATH> __global__ void cf_acc_sbuild(McBatch B, AccArgs A);
template <int PATH> __global__ void cf_acc_seed(McBatch B, AccArgs A);
template <int PATH> __global__ void cf_acc_link(McBatch B, AccArgs A, int flip);
template <int PATH> __global__ void cf_acc_close(McBatch B, AccArgs A, int j, int flip);
__global__ void dx_sweep_diag(DxBatch B, const ScoreModel* __restrict__ M, int t);
__global__ void dx_logz(DxBatch B, const ScoreModel* __restrict__ M);
__global__ void dx_posterior(DxBatch B);
__global__ void dx_hp_clear_rest(DxBatch B);
__global__ void lin_init(McBatch B, const LinModel* __restrict__ L, int* __restrict__ bad);
template <int W, int BS, int MODE> __global__ void lin_inside_diag(McBatch B, const LinModel* __restrict__ L, int d, double lam_d, int pin);
template <int W, int BS> __global__ void lin_outside_diag(McBatch B, const LinModel* __restrict__ L, int d, int pin, int* __restrict__ bad);
template <int W, int BS> __global__ void lin_outside_pair(McBatch B, const LinModel* __restrict__ L, int d, int khi, int pin, int* __restrict__ bad);
template <int BS> __global__ void lin_far_inside(McBatch B, int D);
template <int BS> __global__ void lin_far_outside(McBatch B, int D);
__global__ void lin_far_inside_mfma(McBatch B, int D);
__global__ void lin_far_outside_mfma(McBatch B, int D);
template <int SWEEP> __global__ void lin_pack_tiles(McBatch B, int Dblk, int outside, int banded);
template <int KD, int W, int FILT> __global__ void lin_inside_strip(McBatch B, const LinModel* __restrict__ L, const double* __restrict__ wT, int d0, double lam_d0, int pin);
template <int KD, int W, int FILT> __global__ void lin_outside_strip(McBatch B, const LinModel* __restrict__ L, const double* __restrict__ wT, int d0, int pin, int* __restrict__ bad);
__global__ void lin_f5i_tail(McBatch B, const LinModel* __restrict__ L, int jlo);
__global__ void lin_f5i_pass(McBatch B, const LinModel* __restrict__ L, int jlo);
void launch_lin_small(const McBatch& B, const LinModel* L, const double* wpad, const int* list, int nlist, int* bad, hipStream_t stream);   // mccaskill_small.hip
__global__ void lin_f5o_head(McBatch B, const LinModel* __restrict__ L, int khi, int klo);
__global__ void lin_f5o_pass(McBatch B, const LinModel* __restrict__ L);
__global__ void lin_far_inside_pk(McBatch B, int D, int l2);
__global__ void lin_far_outside_pk(McBatch B, int D, int l2);
__global__ void lin_far_inside_pk4(McBatch B, int D, int l2);
__global__ void lin_far_outside_pk4(McBatch B, int D, int l2);
__global__ void lin_far2_inside(McBatch B, int D2, int l2);
__global__ void lin_far2_outside(McBatch B, int D2, int l2);
__global__ void lin_finish(McBatch B, const LinModel* __restrict__ L, double* __restrict__ logz, int* __restrict__ bad);
template <int W> __global__ void dxl_sweep(DxLinBatch B, const DxLinModel* __restrict__ L, int step, int groups);
__global__ void dxl_sweep4(DxLinBatch B, const DxLinModel* __restrict__ L, int step, int groups);
__global__ void dxl_strip8(DxLinBatch B, const DxLinModel* __restrict__ L, int step);
template <bool S20> __global__ void dxvl_sweep4(DxLinBatch B, const VLinModel* __restrict__ L, const VDxLin* __restrict__ D, int step);
template <bool S20> __global__ void dxvl_logz_part(DxLinBatch B, const VLinModel* __restrict__ L, const VDxLin* __restrict__ D, double* __restrict__ zpart,
                               int* __restrict__ cpart, int nchunk);
__global__ void dxvl_logz_final(DxLinBatch B, double s, const double* __restrict__ zpart, const int* __restrict__ cpart, int nchunk,
                                double* __restrict__ zbar, double* __restrict__ logz, int* __restrict__ bad);
constexpr int kLzThreads = 256;       // threads of a dxl_logz_part workgroup (its LDS staging is laid out for this count)
size_t dxl_logz_lds_bytes(int lds);   // duplex_lin.hip: dynamic LDS of a dxl_logz_part launch (weights and the letters of a pair); 0 = does not fit
__global__ void dxl_logz_part(DxLinBatch B, const DxLinModel* __restrict__ L, double* __restrict__ zpart, int* __restrict__ cpart, int nchunk);
__global__ void dxl_logz_final(DxLinBatch B, const DxLinModel* __restrict__ L, const double* __restrict__ zpart, const int* __restrict__ cpart, int nchunk,
                               double* __restrict__ zbar, double* __restrict__ logz, int* __restrict__ bad);
__global__ void dxl_posterior(DxLinBatch B, const double* __restrict__ zbar, int* __restrict__ bad);
__global__ void dxv_sweep_diag(DxBatch B, const ViennaDx* __restrict__ V, int t);
__global__ void dxv_logz(DxBatch B, const ViennaDx* __restrict__ V);
__global__ void dxv_posterior(DxBatch B);
__global__ void mcv_init(McBatch B);
__global__ void mcv_inside_diag(McBatch B, const ViennaDx* __restrict__ V, int d, int pin);
__global__ void mcv_outside_diag(McBatch B, const ViennaDx* __restrict__ V, int d, int pin);
__global__ void mcv_acc_prep(McBatch B, const ViennaDx* __restrict__ V);
__global__ void mcv_acc_hscan(McBatch B, int slot);
__global__ void vlin_acc_prep(McBatch B, const VLinModel* __restrict__ L, const double* __restrict__ hplen);
__global__ void vlin_acc_gaps(McBatch B, const VLinModel* __restrict__ L, double* __restrict__ gaps, int ng, int nchunk, double* __restrict__ part);
__global__ void vlin_acc_gsum(McBatch B, double* __restrict__ gaps, const double* __restrict__ part, int ng, int nchunk);
__global__ void vlin_acc_gaps_wide(McBatch B, const VLinModel* __restrict__ L, double* __restrict__ gaps);
__global__ void vlin_acc_final_t(McBatch B, const VLinModel* __restrict__ L, const double* __restrict__ gaps, int max_w);
__global__ void vlin_acc_hsum(McBatch B, int max_w);
__global__ void vlin_acc_gsuf(McBatch B, double* __restrict__ gaps);
__global__ void vlin_acc_final(McBatch B, const VLinModel* __restrict__ L, const double* __restrict__ gaps, int max_w);
__global__ void mcv_acc_gaps(McBatch B, const ViennaDx* __restrict__ V, double* __restrict__ gaps);
__global__ void mcv_acc_final(McBatch B, const ViennaDx* __restrict__ V, const double* __restrict__ gaps, int max_w);
__global__ void mcv_finish(McBatch B, double* __restrict__ logz);
__global__ void vlin_init(McBatch B, int* __restrict__ bad);
template <int W, int BS, bool CUT, int MODE> __global__ void vlin_inside_diag(McBatch B, const VLinModel* __restrict__ L, int d, double hp_d, int pin);
template <int W, int BS, bool CUT, int MODE> __global__ void vlin_outside_diag(McBatch B, const VLinModel* __restrict__ L, int d, int pin, int* __restrict__ bad);
__global__ void vlin_finish(McBatch B, const VLinModel* __restrict__ L, double* __restrict__ logz, int* __restrict__ bad);
__global__ void mcv_extract_hp(McBatch B, double* __restrict__ hp, size_t hp_stride, int ldd, double* __restrict__ logz, double lin_s, int* __restrict__ bad);
// allow_mask.hip: the structure-constraint masks [ns][ld][ld] from the per-letter values of constraint_prepass.h; grid (ns, tiles of
// kAllowRows rows), kAllowThreads threads, 9 * lds bytes of dynamic LDS when in_lds
constexpr int kAllowRows = 64, kAllowThreads = 256;
__global__ void allow_mask_build(uint8_t* __restrict__ allow, const int* __restrict__ n_of, const uint8_t* __restrict__ g_ch,
                                 const int* __restrict__ g_P, const int* __restrict__ g_enc, int ld, int lds, int in_lds);
// allow_mask.hip: the per-letter values of the joint constraints of an indexed batch, [np][co_lds] each as allow_mask_build reads
// them, composed from the shares of the distinct sequences (constraint_prepass.h: share_prepass, compose_joint_letter); grid (np),
// kJointGatherThreads threads.  Pair p = first share of sequence idx[2p] + second share of sequence idx[2p+1].
struct JointShares {
    const uint8_t* ch;     // [2][ns][lds]: role 0 = the sequence's share as s1, role 1 = as s2
    const int* P;          // [2][ns][lds]
    const int* enc;        // [2][ns][lds]
    const int* open_off;   // [2 ns + 1]: share role * ns + k owns open_pos[open_off[.] .. open_off[. + 1])
    const int* open_pos;   // positions of the open brackets, ascending per share
    const int* idx;        // [2 np]
    const int* con;        // [2][np]: joint lengths, cuts (pair_gather)
    int ns, np, lds, co_lds;
};
constexpr int kJointGatherThreads = 256;
__global__ void joint_cons_gather(JointShares S, uint8_t* __restrict__ ch, int* __restrict__ P, int* __restrict__ enc);
// pair_index.hip: the pair-major image of an upload, built from the distinct sequences and the index (pair p = sequences
// idx[2p], idx[2p+1]); grid (np, 2), kPairGatherThreads threads
struct PairImage {
    const uint8_t* seq;   // [ns][lds] codes of the distinct sequences (both sentinels included)
    const int* n;         // [ns]
    const int* idx;       // [2 np]
    uint8_t* pseq;        // [2 np][lds]: row 2p + side = the codes of idx[2p + side]
    int* pn;              // [2 np]
    uint8_t* coseq;       // two-molecule ensemble (or nullptr): [np][co_lds], s1 at 1..n1, s2 at n1+1..n1+n2, code 0 elsewhere
    int* con;             // [2][np]: joint lengths, cuts
    int np, lds, co_lds;
};
constexpr int kPairGatherThreads = 256;
__global__ void pair_gather(PairImage G);
__global__ void vlin_co_seed(McBatch B, McBatch S, const int* __restrict__ idx);
// pack_results.hip: the dense results of a computed batch narrowed to float into the packed image of packed_layout (batch.h); grid
// (blocks of the kinds asked for: bp, up, hp in this order; chunks of a block), kPackThreads threads.  A kind whose source is nullptr
// is left out of the grid.
struct PackArgs {
    const double* bp;      // [nseq][tri_stride]
    const double* up;      // [nseq][up_stride], n * max_w entries used
    const double* hp;      // [np][hp_stride], row pitch ldd
    const int* n;          // [nseq]
    const int* pn;         // [2 np]: the lengths of pair p's sequences
    const size_t* off;     // bp_off [nseq + 1], up_off [nseq + 1], hp_off [np + 1], one behind the other
    float* dst_bp;         // the three images (each 16-byte aligned)
    float* dst_up;
    float* dst_hp;
    size_t tri_stride, up_stride, hp_stride;
    int nseq, np, max_w, ldd;
};
constexpr int kPackThreads = 256, kPackGroupsPerThread = 4;
__global__ void pack_results_f32(PackArgs A);
}  // namespace rh

// defined by the host units (global namespace)
__global__ void collect_logz(const double* __restrict__ mc_logz, const int* __restrict__ idx, rh::DxBatch D, double* __restrict__ out);              // rh_api.hip
__global__ void log_finish(rh::McBatch B, double* __restrict__ logz);                                                       // launch_contrafold.hip
// candidates.hip
__global__ void cand_count(const double* __restrict__ base, int kind, int n, int n2, int ld, float th, int nrows, int* __restrict__ counts);
__global__ void cand_write(const double* __restrict__ base, int kind, int n, int n2, int ld, float th, int nrows, const int* __restrict__ counts,
                           const int* __restrict__ offsets, rh_cand* __restrict__ out, int cap);
__global__ void cand_count_all(const double* __restrict__ bp, const double* __restrict__ hp, const double* __restrict__ up, const int* __restrict__ nn,
                               const int* __restrict__ idx, int per, size_t tri_stride, size_t hp_stride, int up_ld, int hp_ld, int which, int rmax, float th, int* __restrict__ counts);
__global__ void cand_write_all(const double* __restrict__ bp, const double* __restrict__ hp, const double* __restrict__ up, const int* __restrict__ nn,
                               const int* __restrict__ idx, int per, size_t tri_stride, size_t hp_stride, int up_ld, int hp_ld, int which, int rmax, float th, const int* __restrict__ counts,
                               const int* __restrict__ offsets, rh_cand* __restrict__ out, int cap);
