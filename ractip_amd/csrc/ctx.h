// ctx.h -- the context behind the opaque rh_ctx of include/ractip_hot.h, its device buffers, and the host functions
// the units of the library share (namespace rh::host).
#pragma once
#include <hip/hip_runtime.h>

#include <cassert>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ractip_hot.h"
#include "batch.h"
#include "batch_request.h"
#include "local_windows.h"
#include "score_model.h"
#include "lin_model.h"
#include "vienna_model.h"
#include "scale_order.h"
#include "span_fold.h"

struct rh_ctx;

namespace rh::host {

// grow-only device buffer: freed by its destructor, grown by ensure() (free-then-malloc when too small)
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;   // bytes
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    explicit operator bool() const { return p != nullptr; }
};

// one model struct (or weight table) in HBM, allocated once at its exact size
template <class T>
struct DevObj : DevBuf {
    operator T*() const { return as<T>(); }
    hipError_t upload(const T* host, size_t count = 1)
    {
        hipError_t e = hipMalloc(&p, sizeof(T) * count);
        if (e != hipSuccess) return e;
        cap = sizeof(T) * count;
        return hipMemcpy(p, host, cap, hipMemcpyHostToDevice);
    }
};

// The hp result of a local hybridization (local_fold.hip): hp_loc [(n1+1)][(n2+1)] and log Z per window pair [nw1][nw2] on the device,
// grow-only.  A molecule that was not cut into windows (the query of rh_local_duplex) is the one window of its plan.
struct LocalHp {
    LocalDuplex2Plan D;            // of s1 and of s2
    int windowed = 0;              // rh_local_duplex: the molecule it cut, as rh_local_hp_layout reports it
    bool valid = false;
    DevBuf hp, logz;
    int tile[2] = {0, 0};          // rows, cols of the tile the call ran
    double ms[2] = {0, 0};         // rh_local_duplex2: the tiles' computes; gather + finish kernels and the scans since
};

// CONTRAfold linear path: the model at one scale exponent -- host copy, device copy and the transposed, zero-padded single-branch
// weights wT[l1][t+1] of the strip kernels.  McLinArgs::lin names the one a pass runs on.
struct LinSet {
    LinModel h;
    DevObj<LinModel> d;
    DevObj<double> wT;
};

// Vienna-BL linear path: the model at one scale exponent (built on first use, see select_vlin)
struct VLinSet {
    VLinModel* h = nullptr;
    DevObj<VLinModel> d;
    ~VLinSet() { delete h; }
};

struct GraphSlot {   // one captured launch sequence (see run_graphed)
    hipGraphExec_t exec = nullptr;
    size_t key = 0;   // hash of the argument(s) it was captured with
    int launches = 0, far = 0;
};

// The kernel organisation of one sweep (McCaskill inside, McCaskill outside, hybridization), decided once per compute from the
// context's switches and the batch shape by plan_mc_lin / plan_mc_vlin / plan_dx_lin / plan_dx_vlin.  The launchers run it and
// rh_batch_kernels reports it; nothing else reads the organisation switches.
struct SweepPlan {
    enum Org { kNone, kStrips, kPairs, kLookahead, kDiagonals, kDxStrip8, kDxSweep4, kDxSweepW };
    // block products: LDS/FMA kernel, MFMA with gathered operand tiles, MFMA on packed tiles with one wavefront per tile or (kFarPacked4)
    // split-K over the four wavefronts of a workgroup per tile
    enum Far { kFarNone, kFarLds, kFarGather, kFarPacked, kFarPacked4 };
    bool packed() const { return far == kFarPacked || far == kFarPacked4; }
    Org org = kNone;
    int W = 0;              // wavefronts per 64-cell group (strips: per workgroup)
    int BS = 0;             // block size of the far/near split of the O(n^3) terms (0: no block products)
    int filt = 0;           // strips: the factored single-branch filter
    Far far = kFarNone;
    int far2_from = 0;      // packed products: the length from which a sequence takes the two-level form (0: no sequence does)
    int banded = 0;         // packed products: block diagonal 2 of FM1 / FM is packed masked (the strips' banded near/far split)
    int repack2 = 0;        // outside sweep: the inside sweep left block diagonal 2 packed in the other form
    const char* fine = "";       // names rh_batch_kernels reports: the sweep kernel ...
    const char* far_name = "";   // ... and the block-product kernel
};

// ---- The argument of each captured launch sequence.  A launcher takes (rh_ctx*, const Args&), and everything that can differ between
// two computes on one context reaches it through the argument: run_graphed keys the captured graph by a hash of the argument's
// bytes, so a value a launcher took from anywhere else would be one a stale graph replays.  Inside a launcher the context serves
// only for the streams and events, the KLAUNCH timing state, the n_launch / n_far counters, fail(), and the objects that are fixed
// from rh_create* to rh_destroy (d_model, d_vienna, d_vdx, d_vdxl, d_dxlin).  The arguments are built outside the capture
// (mc_lin_args, mc_vlin_args, dx_lin_args), plans and variants decided.  Equal fields give equal bytes: an argument starts as zeroed
// storage, and what is copied into it whole has no padding of its own.
static_assert(std::has_unique_object_representations_v<SweepPlan> && std::has_unique_object_representations_v<McBatch>);
static_assert(sizeof(DxLinBatch) == 4 * sizeof(void*) + 6 * sizeof(int) + 3 * sizeof(size_t) + 16 * sizeof(double), "no padding");

struct McLinArgs {   // launch_mc_lin: one phase (0 inside, 1 outside) of the CONTRAfold-model sweeps on the scaled linear kernels
    McBatch B;                 // every sequence of the pass
    const LinSet* lin;         // the model at the scale exponent of this pass
    double* logz;              // per sequence of B
    int* bad;
    SweepPlan plan;            // of the pass over B as it is (not routed)
    // per-sequence routing (the batch as uploaded only; see launch_mc_lin): the sequences of the small list have a workgroup each,
    // the sweeps see the lengths n_sweep, the short pass n_short (0 hides a sequence), each with a plan of its own
    const int* small_list;     // device
    const int* n_sweep;
    const int* n_short;
    SweepPlan plan_sweep, plan_short;
    int routed, n_small, nmax_sweep, short_count, nmax_short;
    int phase, pin, strip_xcd;
    int f5_pass, f5_jlo;       // strips: the exterior sums by lin_f5i_pass / lin_f5o_pass (0: the serial kernels, same bits); the first F5i
                               // entry the bootstrap diagonals do not leave behind
    int up_w, pad_;            // row pitch of B.up (the context's max_w): mc_unpaired writes column 0
    McLinArgs() { std::memset(this, 0, sizeof *this); }
};

struct McVlinArgs {   // launch_mc_vlin: one phase of the Vienna-BL sweeps over the single-molecule batch or (co) the s1+s2 batch
    McBatch B;
    McBatch from;              // seeded two-molecule sweeps: the single-molecule batch whose inside tables they copy ...
    const int* pair_seq;       // ... and the index of the upload (device, [2 np]): pair p copies from sequences pair_seq[2p], pair_seq[2p+1]
    SweepPlan plan;
    const VLinModel* d_vlin;   // the model at the scale exponent of this pass, device and host (select_vlin) ...
    const VLinModel* h_vlin;
    const double* hplen;       // ... its hairpin length weights x lam^d: host (kernel argument of inside diagonal d) and device
    const double* d_hplen;
    int* bad;
    double* logz;              // single-molecule batch: log Z, the gap probabilities of the accessibility and its widths
    double* gaps;
    double* hp;                // two-molecule sweeps: where hp and its log Z go (DxBatch::hp, logz, tab_stride, ldd, n1max, n2max)
    double* hp_logz;
    size_t hp_stride;
    int hp_ldd, n1max, n2max;
    int window, cut_min, cut_max;   // ... and the window of groups around the cuts they launch
    int max_w, acc_wide, acc_final_t;   // accessibility variants: vlin_acc_gaps_wide, vlin_acc_final_t
    int phase, pin, co;
    McVlinArgs() { std::memset(this, 0, sizeof *this); }
};

struct DxLinArgs {   // launch_dx_lin (CONTRAfold model: dm, hm) and launch_dx_vlin (Vienna-BL: vdx_s)
    DxLinBatch X;              // the whole batch, or a compacted sub-batch of the scale-exponent ladder with its own tables
    SweepPlan plan;
    const DxLinModel* dm;      // the model at the scale exponent of this pass: device, host
    const DxLinModel* hm;
    double vdx_s;
    double* zpart;             // [lz_chunks][np] partial sums of Z~ (+ cell counts behind them)
    double* zbar;
    double* logz;              // per pair of X
    int* bad;
    int lz_chunks;
    int sem20;                 // Vienna-BL: the 2.x instantiations (dxvl_sweep4<true>, four more tables per pair)
    DxLinArgs() { std::memset(this, 0, sizeof *this); }
};
static_assert(std::is_trivially_copyable_v<McLinArgs> && std::is_trivially_copyable_v<McVlinArgs> && std::is_trivially_copyable_v<DxLinArgs>);

// the events of one compute (Ctx::ev): three phases on the McCaskill stream, one on the hybridization stream
enum Ev {
    kEvMcStart,     // s_mc: before the inside sweep
    kEvMcInside,    // s_mc: behind the inside sweep
    kEvMcEnd,       // s_mc: behind the outside sweep and the accessibility
    kEvDxStart,     // s_dx: before the hybridization sweeps
    kEvDxEnd,       // s_dx: behind them
    kEvMcOutside,   // s_mc: before the outside sweep, where something ran between the two sweeps (the seeded two-molecule sweeps)
    kEvCount
};

struct Ctx {   // (the fields of rh_ctx, below)
    int device = 0;
    int model = 0;
    std::string err;
    hipStream_t s_mc = nullptr, s_dx = nullptr;
    hipEvent_t ev[kEvCount] = {};
    DevObj<ScoreModel> d_model;
    // other scale exponents of the linear McCaskill path, tried on the problems that leave the double range before the log-space
    // kernels are (retry_mc_lin_rungs): built on first use from the host copy of the score model
    static constexpr int kRungs = 3;
    ScoreModel* h_score = nullptr;
    LinSet* lin_r = nullptr;                   // [kRungs]
    int scale_ladder = 1;                      // RH_SCALE_LADDER=0: flagged problems go straight to the log-space kernels
    int scale_memory = 0;                      // rh_set_scale_memory / RH_SCALE_MEMORY=1: the next batch starts on the exponent most of the last one needed
                                               // (off by default: a sequence's bits then depend on its own letters only, never on the context's history)
    // the default exponent's model and the exponent the NEXT batch starts with: -1 = default, k = rung k -- the one that held more
    // than half of the last batch (a stream of structured RNAs does not pay a failed first pass per batch)
    LinSet lin0;
    int lin_primary = -1;
    std::vector<int> rescaled_mc;              // sequences the last compute recomputed on the linear path with another exponent (rh_batch_fallbacks which = 2)
    DevObj<ViennaDx> d_vienna;     // RH_MODEL_VIENNA_BL only
    int vienna_sem = 0;            // kViennaSem18 / kViennaSem20 (0: CONTRAfold model)
    VLinModel* d_vlin = nullptr;   // the same model in scaled linear space: the selected entry of vlin_m (not owned)
    VLinModel* h_vlin = nullptr;
    // Vienna-BL: other scale exponents of the linear path, tried on the WHOLE batch (single-molecule folds and two-molecule sweeps
    // together: the latter are seeded from the former) before the log-space kernels; see compute().  Model -1 = the default exponent.
    static constexpr int kVRungs = 3;
    ViennaDx* h_vienna = nullptr;              // host copy of the energy tables the rung models are built from
    VLinSet vlin_m[kVRungs + 1];     // [0] = default, [k + 1] = rung k (owners)
    int vlin_cur = -1, vlin_primary = -1;      // model selected now / the one a batch starts with
    // Vienna-BL, per-pair route of the ladder (round 3): when at most half of the pairs of a batch are flagged, only THOSE pairs are recomputed --
    // on a helper context of the same model (its own tables, its own whole-batch ladder and log-space fallback) -- and their results are
    // copied into this batch's result buffers; every other pair keeps the result of the first pass bit for bit
    rh_ctx* helper = nullptr;
    bool is_helper = false;
    int pair_helper = 1;           // RH_PAIR_HELPER=0: the whole batch is run again (round-2 behaviour); 2: helper whenever at most half of the pairs are flagged
    std::string p_param, p_defaults;           // creation arguments, for the helper
    bool p_has_param = false, p_has_defaults = false;
    int p_use_bl = 1, p_sem = 0;
    DevObj<VLinModel> d_vdxl;      // the same tables at the duplex scale (duplex_vlin.hip)
    DevObj<VDxLin> d_vdx;
    double vdx_s = 0.27;           // log Z of pf_duplex per unit of a+b: 0.23 (random ACGU) .. 0.32 (70 % GC)
    DevObj<DxLinModel> d_dxlin;
    DxLinModel h_dxlin;
    DevObj<DxLinModel> d_dxlin_r[4];   // duplex scale-exponent ladder (retry_dx_lin_rungs), built on first use
    DxLinModel h_dxlin_r[4];
    std::vector<int> rescaled_dx;              // pairs the last compute recomputed on the linear duplex kernels with another exponent (rh_batch_fallbacks which = 3)
    DxLinBatch dxl = {};
    size_t dxl_layout = 0;         // (lda, rows) signature of the zero-padded table image currently in HBM
    size_t dx_bytes = 0;           // bytes of d_dxtab the staged batch uses
    bool dxtab_log = false;        // the log-space duplex kernels wrote d_dxtab since its last clear: the linear kernels, which share
                                   // the buffer and need zero pad columns, clear it first (a change of mode without a new upload)
    int co_seed = 1;               // Vienna-BL, hp from the two-molecule ensemble: copy the one-strand cells from the single folds (RH_CO_SEED=0: sweep them again)
    int dx_strip = 1;              // linear duplex: eight anti-diagonals per launch (dxl_strip8); RH_DX_STRIP=0: four (dxl_sweep4)
    int dx_quad = 1;               // linear duplex: four anti-diagonals per launch (dxl_sweep4, 4 wavefronts per group); RH_DX_QUAD=0: two (dxl_sweep<W>)
    int dx_w = 4;                  // wavefronts per 64-cell group of the linear duplex kernel
    int last_dx_path = 0;
    int far_mfma = 1;              // block products on v_mfma_f64_16x16x4_f64 (BS = 16); RH_FAR_MFMA=0: LDS/FMA kernel
    int lookahead = 2;             // inside sweep: 2 = two diagonals per launch (lin_inside_diag MODE 3), 1 = look-ahead pairs of launches
                                   // (MODE 1/2), 0 = one full launch per diagonal; RH_LOOKAHEAD
    int strip = 3;                 // CONTRAfold linear path: KD = 8 diagonals per launch (mccaskill_strip.hip) with the banded near/far split;
                                   // RH_STRIP=0: the per-diagonal-pair kernels of mccaskill_lin.hip.  Bit 0 = inside sweep, bit 1 = outside sweep
    int far2 = -1;                 // two-level block products: -1 = by size (sequences of n >= 384), 0 / 1 forced (RH_FAR2)
    int strip_w = 8;               // wavefronts per strip workgroup (RH_STRIP_W = 4 | 8)
    // short sequences (kSmallMin <= n <= kSmallMax, CONTRAfold model, scaled linear path): one workgroup per sequence, one launch
    // (mccaskill_small.hip); chosen per sequence by its length alone, so a result does not depend on the rest of the batch.  The sweeps
    // see these sequences with length 0 (d_n_sweep).  Opt-in (RH_SMALL=1): measured slower than the sweeps (6.1 against 4.9 ms per 1000 pairs of 109 + 53 letters).
    int small_on = 0;
    std::vector<int> small_list;
    DevBuf d_small_list;
    DevBuf d_n_sweep;
    int nmax_sweep = 0;
    // sequences shorter than 40 letters next to longer ones: the sweeps choose their launch organisation by the longest sequence they
    // see (strips of eight diagonals from 40 letters on), so these get a pass of their own with the organisation they would get alone
    // (d_n_short: their lengths, 0 for everyone else) -- a result then does not depend on what else is in the batch
    DevBuf d_n_short;
    int n_short = 0, nmax_short = 0;
    int strip_filt = 1;            // single-branch filter of the strip kernels: 1 = factored (A(t) B(|l1-l2|) + sparse residual), 0 = dense (RH_STRIP_FILT)
    bool strip_filt_ok = false;    // the model's weights have the factored form (strip_weights verifies it entry by entry)
    int co_cut_min = 0, co_cut_max = 0;   // smallest / largest cut (length of s1) of the two-molecule batch: bounds of the groups its sweeps launch
    int co_window = 1;             // two-molecule sweeps launch only the groups around the cut (RH_CO_WINDOW=0: all groups, most of which return at once)
    int acc_final_t = 1;           // Vienna-BL accessibility: vlin_acc_final_t (one thread per letter, all widths; RH_ACC_FINAL_T=0: one thread per letter and width)
    int acc_wide = 1;              // Vienna-BL accessibility: vlin_acc_gaps_wide for the gap lengths 3..30 (RH_ACC_WIDE=0: vlin_acc_gaps for all)
    int strip_xcd = 1;             // groups of one sequence consecutive on one XCD (RH_STRIP_XCD=0: sequence-major launch order only)
    int f5_pass = 1;               // exterior sums of the strip sweeps in one pass per direction; RH_F5_PASS=0: lin_f5i_tail / lin_f5o_head over the same
                                   // ranges, one entry at a time (slow, the same bits: the reference of tests/test_gpu_f5_pass.py)
    int far_pk = 1;                // ... on packed operand tiles (lin_pack_tiles + lin_far_*_pk); RH_FAR_PK=0: gather per product
    int far_wave = 1;              // 16-tile products on packed tiles: one wavefront per tile; RH_FAR_WAVE=0: lin_far_*_pk4, a workgroup per tile with
                                   // split-K over its four wavefronts (the same bits: the reference of tests/test_gpu_far_wave.py)
    int use_graphs = 1;            // RH_NO_GRAPH=1 launches every kernel from the host instead
    GraphSlot g_in, g_out, g_dx;
    int mode = RH_MODE_AUTO;       // which McCaskill path rh_batch_compute takes
    int duplex_mode = RH_MODE_INHERIT;   // rh_set_duplex_mode: the path of the pf_duplex sweeps alone (INHERIT: as `mode`)
    int lin_w = 4;                 // wavefronts per 64-cell group of the linear outside kernel (Vienna-BL kernels: 8)
    int lin_w_in = 4;              // ... of the inside kernel (fewer, longer wavefronts: less per-wavefront scalar overhead)
    int lin_bs = 16;               // block size of the far/near split of the O(n^3) terms (0 = off)
    int last_path = 0;             // 1 = linear, 2 = log-space, 3 = linear then log-space fallback
    bool last_went_log = false;    // Vienna-BL: the last compute ended with the folds or the two-molecule sweeps on the log-space kernels
                                   // (recompute_pairs_on_helper reads it from the helper context, to list its pairs under the right mechanism)
    SweepPlan plan[3];             // of the linear first pass over the batch as uploaded: inside, outside, hybridization (run_attempt)
    int max_w = 1;                 // accessibility widths 1..max_w (src/ractip.cpp:370-375); the CONTRAfold path has width 1 only ...
    int region_acc = 0;            // ... unless rh_set_region_accessibility turned the wider widths on (mccaskill_acc.hip, launch_mc_acc)
    DevBuf d_acc;                  // scratch of launch_mc_acc: [ns][acc_scratch_doubles(ld)], allocated by the first compute that needs it
    hipEvent_t acc_ev[2] = {nullptr, nullptr};   // around the accessibility kernels of the batch as uploaded (rh_batch_acc_time)
    bool acc_timed = false;

    // current batch (host mirror): published by stage() as its last step, all zero / false while it works and after it failed
    int np = 0, ns = 0;
    // the index of the upload: pair p = sequences pair_seq[2p] (s1) and pair_seq[2p+1] (s2) of the fold batch.  rh_batch_upload
    // stages the identity (2p, 2p+1); rh_batch_upload_indexed any pairs of the ns distinct sequences.  Read through seq_of().
    std::vector<int> pair_seq;
    std::vector<int> pair_seq_dev; // what d_pidx holds (a stream of uploads with one index, the identity of plain batches, copies it once)
    bool indexed = false;          // the batch came from rh_batch_upload_indexed
    bool has_mc = false, has_dx = false, computed = false;
    std::vector<int> n;  // [ns]
    McBatch mc = {};
    DxBatch dx = {};
    // owned device buffers
    DevBuf d_seq;
    DevBuf d_n;
    DevBuf d_pseq;    // pair-major image of the codes [2 np][lds] the duplex kernels read (pair_gather) ...
    DevBuf d_pn;      // ... its lengths [2 np] ...
    DevBuf d_pidx;    // ... and pair_seq on the device
    DevBuf d_mctab;
    DevBuf d_corowp;
    DevBuf d_rowp;    // look-ahead partial sums of the next inside diagonal
    DevBuf d_pk;        // operand tiles of the block products (single-molecule batch)
    DevBuf d_copk;    // ... of the s1+s2 batch
    DevBuf d_f5;
    DevBuf d_bp;
    DevBuf d_up;
    DevBuf d_dxtab;
    DevBuf d_hp;
    DevBuf d_logz;
    DevBuf d_scal;
    DevBuf d_mclogz;
    DevBuf d_bad;
    DevBuf d_cnt;
    DevBuf d_dxbad;
    DevBuf d_zbar;
    DevBuf d_zpart;   // per-chunk partial sums of Z~ (+ pairable-cell counts behind them)
    int lz_chunks = 0;
    DevBuf d_cand;
    // compacted sub-batches of the per-problem log-space fallback
    DevBuf d_subseq;
    DevBuf d_subn;
    DevBuf d_subbp;
    DevBuf d_subup;
    DevBuf d_subdseq;
    DevBuf d_subdn;
    DevBuf d_subdx;
    bool tables_dirty = false;      // the last compute met values outside the double range: clear the tables before the next batch
    std::vector<uint8_t> h_codes;   // host mirror of d_seq
    std::vector<int> fallback_mc, fallback_dx;   // problems the last compute recomputed in log space (rh_batch_fallbacks)
    DevBuf d_gaps;
    DevBuf d_allow;   // structure-constraint masks [ns][ld*ld] bytes (Vienna-BL, optional)
    DevBuf d_coallow;   // the same for the s1+s2 batch
    DevBuf d_cons;    // per-letter values of the constraint strings the masks are built from: P, enc [count][lds] ints, ch [count][lds] bytes
    DevBuf d_share;   // indexed batch under joint constraints: the shares of the distinct sequences in both roles (JointShares, kernels.h)
    // rh_batch_results_packed_f32 only (a context that never calls it allocates none of this): the staging buffer of the packed float
    // image (as large as the kinds asked for: about 0.5 GB per 256 pairs of n = 500), the offsets on the device with their host copy,
    // and the event pair around the pack kernel (rh_batch_pack_time)
    DevBuf d_pack;
    DevBuf d_packoff;
    std::vector<size_t> pack_off;
    hipEvent_t pack_ev[2] = {nullptr, nullptr};
    bool pack_timed = false;
    DevBuf d_hplen;   // lam^d x hairpin length weight, d = 0..nmax (linear Vienna path)
    std::vector<double> h_hplen;
    // two-molecule (co_pf_fold) form of the hybridization matrix: one concatenated sequence s1+s2 per pair
    int hybrid = RH_HYBRID_DUPLEX;
    McBatch co = {};
    DevBuf d_coseq;
    DevBuf d_con;     // [2][np]: lengths, cuts
    DevBuf d_cotab;
    DevBuf d_cof5;    // f5i, f5o, xp, xs, xpo, xso
    DevBuf d_cobp;
    DevBuf d_cobad;
    double ms[4] = {0, 0, 0, 0};
    int n_launch[3] = {0, 0, 0};
    int n_far[3] = {0, 0, 0};      // of which block-product launches (mccaskill_far.hip)
    bool overlap = true;           // false: duplex, inside and outside sweeps run one after the other (isolated phase timings)
    int time_cls = -1;             // rh_set_kernel_timing: sweep-kernel class whose launches are bracketed by event pairs (-1: none)
    // rh_local_fold only: the last local result -- its shape, the band bp_band [n][ld], up [n][loc_max_w] and log Z per window on the
    // device (grow-only, kept until the next rh_local_fold), and the device times rh_local_times reports
    LocalPlan loc;
    bool loc_valid = false;
    int loc_max_w = 1;
    int loc_chunk = 0;             // rh_set_local_chunk: windows per chunk (0: by kLocalChunkBytes)
    DevBuf d_loc_bp, d_loc_up, d_loc_logz;
    double loc_ms[2] = {0, 0};     // folds (sum of the chunks' computes); accumulate + finish + scans since
    // rh_local_duplex only: the hp part of the last local result, whose times are in loc_ms with the band's; dropped by the next
    // rh_local_fold, replaced by the next rh_local_duplex
    LocalHp loc_hp;
    // rh_local_duplex2 only: the last result of two windowed molecules, kept until the next rh_local_duplex2; the other local calls
    // neither read nor drop it
    LocalHp loc_hp2;
    int loc2_tile[2] = {0, 0};     // rh_set_local_tile: rows, cols of a tile (0, 0: local_tile_auto)
    DevBuf d_loc_rows;             // the row buffer of one row block of a walk with several windows on both sides (grow-only)
    // rh_span_fold only (mccaskill_span.hip): the band tables, the exterior logarithms with the hairpin length weights behind them, the
    // letters and the flag (grow-only); its result is the local result above.  span_ms: the sweeps; the exterior passes and the finish
    DevBuf d_span_tab, d_span_ext, d_span_seq, d_span_bad;
    double span_ms[2] = {0, 0};
    bool span_timed = false;       // a span fold has run on this context
    int span_cf = 0;               // rh_set_span_contrafold: a CONTRAfold context answers the span calls (mccaskill_span_cf.hip) instead of refusing them
    // rh_span_fold_acc at max_w > 1: the gap sums GL, GR [2][kSpanGapRows][ldn] (grow-only) and the device times of the last
    // accessibility stage: the hairpin part, the gap sums, the final kernel
    DevBuf d_span_gaps;
    double span_acc_ms[3] = {0, 0, 0};
    bool span_acc_timed = false;   // the last span fold ran the accessibility stage
    // every span fold: the per-item descriptors of the launches (grow-only)
    DevBuf d_span_desc;
    // span folds under a constraint: the per-letter records of the items of one chunk, laid out like the letters (grow-only)
    DevBuf d_span_cons;
    // rh_span_fold_batch only: the last batch result -- its plan, the status of every item, the bands, up tables and log Z of all
    // items one behind the other (grow-only, kept until the next rh_span_fold_batch), the chunk budget and the device times
    SpanBatchPlan sb;
    std::vector<int> sb_status;
    bool sb_valid = false;
    DevBuf d_sb_bp, d_sb_up, d_sb_logz;
    size_t sb_bytes = 0;           // rh_set_span_batch_bytes (0: kSpanBatchBytes)
    double sb_ms[3] = {0, 0, 0};   // sweeps; exterior passes + finish; accessibility stage
    double sb_scan_ms = 0;         // the scan kernels of rh_span_batch_candidates since
    std::vector<hipEvent_t> tev;   // event pool of the timed class (pairs), tev_n used by the last compute
    size_t tev_n = 0;
    Ctx() = default;
    Ctx(const Ctx&) = delete;
    ~Ctx() { delete[] lin_r; delete h_score; delete h_vienna; }   // (device buffers free themselves; rh_destroy has set the device)
};

}  // namespace rh::host

struct rh_ctx : rh::host::Ctx {};   // the opaque context of include/ractip_hot.h

#define HIP_TRY(c, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(c, e_ == hipErrorOutOfMemory ? RH_ERR_OOM : RH_ERR_HIP, "%s failed: %s", \
                        #call, hipGetErrorString(e_));                                           \
    } while (0)

// launch of one sweep kernel (class = 0 inside, 1 inside block products, 2 outside, 3 outside block products, 4 duplex)
// Measurement aid (rh_set_kernel_timing): launches of class `time_cls` are bracketed by a HIP event pair on their stream, so that
// bench.py can report the average duration of ONE kernel class live (what a kernel trace reports per kernel); off by default.
#define KLAUNCH(c, cls, kern, grid, block, stream, ...)                                                   \
    do {                                                                                                  \
        const bool timed_ = (c)->time_cls == (cls) && (c)->tev_n + 2 <= (c)->tev.size();                  \
        if (timed_) (void)hipEventRecord((c)->tev[(c)->tev_n++], stream);                                 \
        hipLaunchKernelGGL(kern, grid, block, 0, stream, __VA_ARGS__);                                    \
        if (timed_) (void)hipEventRecord((c)->tev[(c)->tev_n++], stream);                                 \
    } while (0)

namespace rh::host {

// rh_api.hip
int fail(rh_ctx* c, int code, const char* fmt, ...);
int ensure(rh_ctx* c, DevBuf& buf, size_t bytes, bool zero);
// staging.hip: check_batch (batch_request.h), then the tables of the request.  A request the checks reject leaves the previous
// batch in place; from the first change to the context until RH_OK the context holds no batch (ns = np = 0, nothing computed), so
// after a failure past the checks (RH_ERR_OOM, a HIP error) rh_batch_compute and the fetches answer "no ... batch".
int stage(rh_ctx* c, const BatchRequest& r);
// sequence of the fold batch that is strand `side` (0: s1, 1: s2) of pair p: the one place that knows how pairs map to sequences
inline int seq_of(const Ctx* c, int p, int side) { return c->pair_seq[2 * (size_t)p + side]; }
// the pairs that use sequence k, appended to *pairs (a flagged sequence flags every pair that references it)
inline void pairs_of_seq(const Ctx* c, int k, std::vector<int>* pairs)
{
    for (int p = 0; p < c->np; p++)
        if (seq_of(c, p, 0) == k || seq_of(c, p, 1) == k) pairs->push_back(p);
}
// a kernel on one line with the name reported for it
template <class K> struct Named { K kern; const char* name; };
#define NAMED(...) {__VA_ARGS__, #__VA_ARGS__}
template <class Row, size_t N, class Pred>
const Row& row_of(const Row (&rows)[N], Pred&& is)
{
    for (const Row& r : rows) if (is(r)) return r;
    assert(!"the plan names a kernel combination that has no row");
    return rows[0];
}
// sequence -> XCD affinity only when the batch spreads evenly over the 8 XCDs (speed only)
inline int xcd_pin(int ns) { return ns % 8 == 0 ? 1 : 0; }
// sequence-major launch order (sequence -> XCD affinity) or group-major
inline dim3 seq_grid(int pin, int ns, int groups) { return pin ? dim3(ns, groups) : dim3(groups, ns); }
// one pass of a McCaskill sweep on the scaled linear kernels: what the schedules and the block-product steps share
struct SweepPass {
    rh_ctx* c;
    const SweepPlan& P;
    const McBatch& B;    // the sequences of this pass
    hipStream_t st;
    int k;               // n_launch[k] / n_far[k] count it
    int far2_next = -1;  // outside: macro block diagonals whose 64-block products are still to be launched (descending)
    int last_block() const { return P.BS > 0 ? (B.nmax - 1) / P.BS : 0; }
};
// launch_contrafold.hip
int launch_mc_log(rh_ctx* c, int pin, const McBatch& B, double* logz_out);
SweepPlan plan_mc_lin(const rh_ctx* c, int phase, int nmax);
int launch_mc_lin(rh_ctx* c, const McLinArgs& A);
int launch_mc_acc(rh_ctx* c, const McBatch& B, const LinSet* lin, bool timed);
void far_products(const rh_ctx* c, int phase, int nmax, bool mfma, SweepPlan* P);
const char* far_name(SweepPlan::Far far, int BS, int phase);
void far_inside_after(const SweepPass& S, int done);
void far_outside_begin(SweepPass& S, int top);
void far_outside_before(SweepPass& S, int d);
std::vector<double> strip_weights(const LinModel& L, bool* ok_out = nullptr);
size_t f5_pass_lds(int ld, int phase);
bool f5_pass_fits(int ld);
// launch_vienna.hip
int launch_mc_vienna(rh_ctx* c, int pin);
SweepPlan plan_mc_vlin(const rh_ctx* c, int phase, bool co, int nmax);
int launch_mc_vlin(rh_ctx* c, const McVlinArgs& A);
int launch_cofold(rh_ctx* c);
int select_vlin(rh_ctx* c, int model);
extern const double kVRungS[Ctx::kVRungs];
// launch_duplex.hip
int launch_dx_log(rh_ctx* c, const DxBatch& D);
SweepPlan plan_dx_lin(const rh_ctx* c, int w);
SweepPlan plan_dx_vlin(bool sem20);
int launch_dx_lin(rh_ctx* c, const DxLinArgs& A);
int launch_dx_vlin(rh_ctx* c, const DxLinArgs& A);
int launch_dx_vlog(rh_ctx* c);
// fallbacks.hip
int ensure_rungs(rh_ctx* c);   // builds lin_r, the CONTRAfold models at the exponents kRungS, on first use
extern const double kRungS[Ctx::kRungs];
int retry_mc_lin_rungs(rh_ctx* c, int first_model, std::vector<int>* rest, int (&rescued_by)[Ctx::kRungs + 1]);
int recompute_mc_subset_log(rh_ctx* c, const std::vector<int>& F);
int retry_dx_lin_rungs(rh_ctx* c, std::vector<int>* rest);
int recompute_dx_subset_log(rh_ctx* c, const std::vector<int>& F);
int recompute_pairs_on_helper(rh_ctx* c, const std::vector<int>& P);
// compute.hip
int compute(rh_ctx* c);
McLinArgs mc_lin_args(const rh_ctx* c, int phase, const McBatch& B, const LinSet* lin, bool routed);
DxLinArgs dx_lin_args(const rh_ctx* c);
int flagged(rh_ctx* c, const int* d_flags, int n, hipStream_t st, std::vector<int>* set);
// local_fold.hip: the scan of rh_local_candidates (what = 0: a band [n][pitch]; 1: an up table [n][pitch]) on any such table
int local_scan_table(rh_ctx* c, const double* table, int n, int pitch, int what, float threshold, rh_cand* out, int cap, double* ms, const char* who);

}  // namespace rh::host

// = create_ctx of rh_api.hip, for the per-pair helper context (C++ linkage, not part of the C ABI)
rh_ctx* make_ctx_for_helper(int device, int model, const char* param_file, const char* defaults_file, int use_bl, int semantics);
