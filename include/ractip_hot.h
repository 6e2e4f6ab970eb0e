/* ractip_hot.h -- C ABI of the MI355X-native probability-matrix engine for RactIP.
 *
 * This is the drop-in boundary of SURVEY.md section 8(b): plain C, no C++ types,
 * no exceptions, caller-owned output buffers, one context per host thread / GPU.
 * Every entry point names the reference interface it replaces (paths relative
 * to /root/reference).  The C++ adapters that rebuild the reference's
 * VF/VI/VVF containers on top of this ABI live in ractip_amd/host/.
 *
 * Status codes: 0 = ok, negative = error (see rh_last_error).
 * Layouts (identical to the reference):
 *   bp  : T(n) = (n+1)(n+2)/2 doubles, element (i,j), 1 <= i < j <= n, at
 *         offset[i]+j with offset[i] = i*(2(n+1)-i-1)/2   (src/ractip.cpp:254-257,
 *         src/contrafold/InferenceEngine.ipp:316); all other entries 0.
 *   up  : n*max_w doubles row-major, up[i*max_w+w] = P(i..i+w unpaired), 0-based i
 *         (src/ractip.cpp:213-222 for max_w=1; src/ractip.cpp:370-375).
 *   hp  : (n1+1)*(n2+1) doubles row-major, 1-based, row 0 / column 0 zero
 *         (src/ractip.cpp:393-397, 236-244).
 */
#ifndef RACTIP_HOT_H
#define RACTIP_HOT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rh_ctx rh_ctx;

/* scoring model selector */
#define RH_MODEL_CONTRAFOLD 0 /* --contrafold path: src/ractip.cpp:195-246 */
#define RH_MODEL_VIENNA_BL 1  /* default CLI path: pf_fold bp + pf_unstru up (src/ractip.cpp:248-382) and the --duplex
                                 pf_duplex hp (src/ractip.cpp:390-398) with the BL* energies of src/boltzmann_param.c in
                                 ViennaRNA-1.8 semantics; PARITY UNPINNED (ViennaRNA is absent and unversioned) */

#define RH_OK 0
#define RH_ERR_ARG (-1)
#define RH_ERR_HIP (-2)
#define RH_ERR_OOM (-3)
#define RH_ERR_PARAM (-4)
#define RH_ERR_UNSUPPORTED (-5)

/* Create a context bound to HIP device `device`.  `param_file` = NULL loads the
 * bundled default weights (ractip_amd/data/contrafold_complementary.params, the
 * values of GetDefaultComplementaryValues, src/contrafold/Defaults.ipp:7-723; for
 * RH_MODEL_VIENNA_BL ractip_amd/data/vienna_bl_star.params, the BL* tables of
 * src/boltzmann_param.c).
 * Replaces the per-call engine construction of src/ractip.cpp:199-206, 229-234.
 * Returns NULL on failure; rh_last_error(NULL) then describes why. */
rh_ctx* rh_create(int device, int model, const char* param_file);
/* RH_MODEL_VIENNA_BL with the energy tables installed the way RactIP::run installs them (src/ractip.cpp:1563-1567):
 *   library defaults  ->  copy_boltzmann_parameters() unless --no-bl-param (use_bl_param)  ->  read_parameter_file(param_file).
 * defaults_file (or NULL): a ViennaRNA parameter file standing for the tables compiled into the user's RNAlib -- ViennaRNA is
 * not part of the reference, so its built-in Turner tables are not in this library; tables no source provides are ZERO.
 * param_file (or NULL): the -P file, ViennaRNA "## RNAfold parameter file" (1.x or v2.0 layout) or the flat dump format of
 * ractip_amd/data/vienna_bl_star.params.  rh_create(dev, RH_MODEL_VIENNA_BL, f) = rh_create_vienna(dev, NULL, 1, f, 0).
 * semantics: how the loop energies are evaluated --
 *   RH_VIENNA_SEM_18: ViennaRNA-1.8 LoopEnergy + dangle sums, the 1.8 branch of src/pf_duplex.c:209-433 (all kernels);
 *   RH_VIENNA_SEM_20: ViennaRNA-2.x E_IntLoop / E_ExtLoop / E_MLstem / E_Hairpin, the HAVE_VIENNA20 branch the reference's
 *     CMake selects (src/pf_duplex.c:128-206; CMakeLists.txt:28): mismatch_interior_1n / _23, mismatch_exterior / _multi,
 *     tri/tetra/hexaloop energies replacing the hairpin energy.  Log-space kernels, except pf_duplex on request:
 *     rh_set_mode(LINEAR) is refused, rh_set_duplex_mode(AUTO or LINEAR) moves the pf_duplex sweeps to the linear kernels;
 *   RH_VIENNA_SEM_AUTO: 2.x if defaults_file or param_file is a v2.0 parameter file, else 1.8.
 * PARITY UNPINNED in both semantics. */
#define RH_VIENNA_SEM_AUTO 0
#define RH_VIENNA_SEM_18 1
#define RH_VIENNA_SEM_20 2
rh_ctx* rh_create_vienna(int device, const char* defaults_file, int use_bl_param, const char* param_file, int semantics);
/* RH_VIENNA_SEM_18 / RH_VIENNA_SEM_20 of a RH_MODEL_VIENNA_BL context, 0 for the CONTRAfold model */
int rh_vienna_semantics(const rh_ctx* ctx);
void rh_destroy(rh_ctx* ctx);
const char* rh_last_error(const rh_ctx* ctx);

/* Arithmetic path of the McCaskill sweeps.  AUTO (default): scaled linear-space kernels,
 * and if any sequence of the batch leaves the double range (detected on device) the whole
 * batch is recomputed by the log-space kernels, which follow the reference's own
 * log-space arithmetic (src/contrafold/LogSpace.hpp).  LOG / LINEAR force one path
 * (LINEAR reports RH_OK even if values overflowed: testing only). */
#define RH_MODE_AUTO 0
#define RH_MODE_LOG 1
#define RH_MODE_LINEAR 2
int rh_set_mode(rh_ctx* ctx, int mode);
/* path taken by the last compute: 1 = linear, 2 = log-space, 3 = linear, then log-space fallback */
int rh_last_path(const rh_ctx* ctx);
/* the same for the sweeps that produced hp (duplex or two-molecule ensemble); 3 also where these sweeps left the double range on
 * the default scale exponent and another exponent on the linear kernels held them: CONTRAfold duplex pairs (rh_batch_fallbacks
 * which = 3), and a Vienna-BL two-molecule ensemble that leaves the range while every single fold of the batch stays inside (two
 * 1000-nt molecules with little structure: Z~ of each is 1e-114, Z~ of the pair 1e-220).  Two-molecule sweeps that only follow a
 * flagged fold to another exponent keep reporting 1. */
int rh_last_hybrid_path(const rh_ctx* ctx);
/* Arithmetic path of the pf_duplex sweeps alone: the sweeps that produce hp under RH_HYBRID_DUPLEX (rh_duplex, the batched
 * form, the pf_duplex shim), either model, either semantics, independently of the McCaskill sweeps.  RH_MODE_INHERIT
 * (default): as rh_set_mode says.  AUTO / LOG / LINEAR: as for rh_set_mode, for these sweeps only -- AUTO recomputes by the
 * log-space kernels what left the double range (rh_last_hybrid_path = 3, rh_batch_fallbacks which = 1), LINEAR never does.
 * Under RH_VIENNA_SEM_20 this is how pf_duplex (src/pf_duplex.c:128-206) reaches the scaled linear kernels: AUTO and LINEAR run
 * them, LOG and INHERIT stay on the log-space kernels.  Ignored under RH_HYBRID_COFOLD: the two-molecule sweeps follow
 * rh_set_mode.  Takes effect at the next compute, with or without a new upload (the linear and the log-space kernels share the
 * pair's tables; a compute that changes from one to the other clears them first).  A RH_VIENNA_SEM_20 context keeps ten
 * linear tables per pair instead of six whether or not it ever calls this. */
#define RH_MODE_INHERIT (-1)
int rh_set_duplex_mode(rh_ctx* ctx, int mode);
int rh_get_duplex_mode(const rh_ctx* ctx);

/* Base-pairing probabilities of one sequence.  Replaces the body of
 * RactIP::contrafold up to GetPosterior (src/ractip.cpp:199-211:
 * ComputeInside/ComputeOutside/ComputePosterior/GetPosterior(0,...)) and, for
 * RH_MODEL_VIENNA_BL, pf_fold + export_bppm of RactIP::rnafold
 * (src/ractip.cpp:288-304, 351-367).  `constraint` (RH_MODEL_VIENNA_BL only, or NULL): the string RactIP hands to
 * pf_fold when use_constraint_ is set (src/ractip.cpp:271-291), in ViennaRNA's fold_constrained alphabet:
 * 'x' never pairs, '<' / '>' pairs only with a later / earlier letter, matched '(' ')' keeps that pair and removes every
 * pair inconsistent with it, '|' and '.' do not restrict the partition function; shorter strings are padded with '.'.
 * A forced pair of non-complementary letters is rejected (RH_ERR_ARG). */
int rh_bpp(rh_ctx* ctx, const char* seq, int n, const char* constraint,
           double* bp_tri, double* logZ);

/* Accessibility, up[i*max_w+w] = P(letters i..i+w unpaired), n*max_w doubles.  RH_MODEL_CONTRAFOLD: max_w must be 1
 * (src/ractip.cpp:213-222, up[i] = max(0, 1 - sum_j bp(i,j))) unless rh_set_region_accessibility is on.  RH_MODEL_VIENNA_BL: any 1 <= max_w <= 64; replaces
 * pf_unstru and the H+I+M+E sum of src/ractip.cpp:370-375.  Sets the context's max_w (see rh_set_max_w). */
int rh_unpaired(rh_ctx* ctx, const char* seq, int n, int max_w, double* up);

/* Number of accessibility widths the batched / rh_fold forms compute (RactIP's --max-w, src/ractip.cpp:546-547:
 * rnafold(..., std::max(1, max_w_))).  Default 1 for RH_MODEL_CONTRAFOLD (only value allowed), 15 for
 * RH_MODEL_VIENNA_BL.  Takes effect at the next upload / single-sequence call. */
int rh_set_max_w(rh_ctx* ctx, int max_w);
int rh_get_max_w(const rh_ctx* ctx);

/* Region accessibility under RH_MODEL_CONTRAFOLD (an extension: the reference refuses widths with --contrafold,
 * src/ractip.cpp:1511-1517).  Off (the default): everything as described above, max_w must be 1.  On: rh_set_max_w and
 * rh_unpaired take 1..64, and rh_fold, the batched forms and their fetches carry n*max_w entries per sequence.
 *   up[i*max_w+w] = Z(letters i..i+w forbidden to pair) / Z, Z the sum over the derivations the CONTRAfold inside recurrences
 *   count (the quantity whose width-1 column is 1 - sum_j bp(i,j)); entries whose region runs past the end hold 0.
 * Column 0 keeps the width-1 arithmetic, max(0, 1 - sum_j bp(i,j)), bit for bit, and bp, hp and log Z do not change.
 * Turning it off sets max_w back to 1.  On a RH_MODEL_VIENNA_BL context the call is accepted and changes nothing. */
int rh_set_region_accessibility(rh_ctx* ctx, int on);
int rh_get_region_accessibility(const rh_ctx* ctx);
/* Measurement aid: device time (ms, one HIP event pair) of the region-accessibility kernels of the last rh_batch_compute, over the
 * batch as uploaded (sequences recomputed with another scale exponent or in log space are not in it). */
int rh_batch_acc_time(rh_ctx* ctx, double* ms);

/* Source of the hybridization matrix hp under RH_MODEL_VIENNA_BL (rh_duplex and the batched form):
 *   RH_HYBRID_DUPLEX (default): pf_duplex -- duplexes only, the --duplex branch (src/ractip.cpp:390-398);
 *   RH_HYBRID_COFOLD: the joint ensemble of both molecules, the default branch (src/ractip.cpp:400-458):
 *     co_pf_fold(s1+s2) with cut_point = n1+1, hp[i][j] = pr(i, n1+j).  The reference keeps only entries
 *     with p > th_hy (assign_plist_from_pr); this ABI returns the dense block and the adapter thresholds.
 *     logZ = log partition function of the two-molecule ensemble.  PARITY UNPINNED like the rest of this model. */
#define RH_HYBRID_DUPLEX 0
#define RH_HYBRID_COFOLD 1
int rh_set_hybrid(rh_ctx* ctx, int hybrid);

/* Both of the above from ONE inside/outside pass -- the whole of RactIP::contrafold (src/ractip.cpp:199-222) or of
 * the accessibility overload of RactIP::rnafold (src/ractip.cpp:308-382).  bp_tri, up (n*max_w doubles, max_w as set
 * by rh_set_max_w) or logZ may be NULL. */
int rh_fold(rh_ctx* ctx, const char* seq, int n, double* bp_tri, double* up, double* logZ);
/* rh_fold under a structure constraint (see rh_bpp): the whole accessibility overload of RactIP::rnafold with
 * use_constraint_ (src/ractip.cpp:308-382). */
int rh_fold_constrained(rh_ctx* ctx, const char* seq, int n, const char* constraint, double* bp_tri, double* up, double* logZ);

/* Hybridization probabilities of a pair.  Replaces RactIP::contraduplex
 * (src/ractip.cpp:225-245: DuplexEngine ComputeInside/Outside/Posterior) and, for
 * RH_MODEL_VIENNA_BL, pf_duplex + pr_duplex of RactIP::rnaduplex (src/ractip.cpp:390-398). */
int rh_duplex(rh_ctx* ctx, const char* s1, int n1, const char* s2, int n2,
              double* hp, double* logZ);

/* The two-molecule ensemble under a structure constraint: what the default branch of RactIP::rnaduplex hands to
 * co_pf_fold when use_constraint_ is set (src/ractip.cpp:405-447): `constraint` has n1+n2 characters over s1+s2 in the
 * fold_constrained alphabet of rh_bpp (RactIP writes '(' for '[' of s1, ')' for ']' of s2 and 'x' for every letter that
 * is paired inside its own molecule).  RH_MODEL_VIENNA_BL only; independent of rh_set_hybrid. */
int rh_cofold_constrained(rh_ctx* ctx, const char* s1, int n1, const char* s2, int n2, const char* constraint,
                          double* hp, double* logZ);

/* ---- batched, device-resident form (z-score loop src/ractip.cpp:1638-1657 and bench) ----
 * A batch is `npairs` independent (s1,s2) pairs; for each the engine computes
 * bp(s1), bp(s2), up(s1), up(s2) and hp(s1,s2) -- everything RactIP::solve needs
 * before the ILP (src/ractip.cpp:536-548).
 *   rh_batch_upload   : encode + copy the sequences to HBM, (re)allocate tables
 *   rh_batch_compute  : run all DP kernels (inputs already resident); blocks until done
 *   rh_batch_results  : copy dense results of pair `p` to caller buffers (any may be NULL)
 *   rh_batch_candidates: thresholded sparse results of pair `p` -- the scans of
 *                       src/ractip.cpp:557-568, 578-589, 598-608, 621-627 done on device.
 * An upload whose arguments are rejected (RH_ERR_ARG, RH_ERR_UNSUPPORTED) leaves the previous batch in place; one that fails
 * afterwards (RH_ERR_OOM, RH_ERR_HIP) leaves the context without a batch until the next successful upload.
 */
int rh_batch_upload(rh_ctx* ctx, int npairs,
                    const char* const* s1, const int* n1,
                    const char* const* s2, const int* n2);
/* rh_batch_upload under structure constraints (RactIP's -c / --use-constraint, src/ractip.cpp:271-291, 330-350, 405-447), one
 * per problem of the batch.  RH_MODEL_VIENNA_BL only (RH_ERR_UNSUPPORTED otherwise).
 *   cons1[p], cons2[p]: constraints of the two single-molecule folds of pair p (bp and up), in the fold_constrained alphabet of
 *     rh_bpp -- what RactIP::rnafold hands to pf_fold;
 *   co_cons[p]: n1+n2 characters over s1+s2 as in rh_cofold_constrained, for the two-molecule ensemble that produces hp under
 *     rh_set_hybrid(RH_HYBRID_COFOLD).  Under RH_HYBRID_DUPLEX it is checked and otherwise unused: the reference's --duplex branch
 *     (src/ractip.cpp:390-398) takes no constraint either.
 * Any of the three arrays, and any entry, may be NULL (no constraint); shorter strings are padded with '.'.  With no constraint at
 * all this is rh_batch_upload.  An unbalanced string or a forced pair of non-complementary letters is rejected (RH_ERR_ARG, the
 * message names the sequence 2p / 2p+1 or the pair p) before anything is staged: the previous batch stays in place.  The masks are
 * built on the device; everything downstream (results, candidates, log Z, fallbacks) works as on any batch. */
int rh_batch_upload_constrained(rh_ctx* ctx, int npairs,
                                const char* const* s1, const int* n1, const char* const* s2, const int* n2,
                                const char* const* cons1, const char* const* cons2, const char* const* co_cons);
/* ---- indexed batches: fold each distinct sequence once, pair by index ----
 * nseq distinct sequences, npairs pairs of them: pair p = (seqs[first[p]], seqs[second[p]]).
 * Every sequence is folded once (bp, up, log Z); every pair gets its hp.  A sequence may be used by any number of pairs, in
 * either role, or by none (it is folded all the same).  A 32 x 32 cross product is 1024 pairs over 64 folds, and its McCaskill
 * tables are those of 64 sequences; under RH_HYBRID_COFOLD the N + M folds seed the N x M two-molecule sweeps.
 * Both models; under RH_MODEL_VIENNA_BL both rh_set_hybrid sources.  Structure constraints on an indexed batch:
 * rh_batch_upload_indexed_constrained below.
 * An index outside [0, nseq), npairs < 1, nseq < 1, a NULL sequence or a length < 1 is RH_ERR_ARG.  All arguments are checked before
 * anything is staged: a rejected upload leaves the previous batch in place, as rh_batch_upload_constrained does.
 * rh_batch_upload IS the indexed upload with the identity index (nseq = 2*npairs, first[p] = 2p, second[p] = 2p+1), bit for bit:
 * both stage the distinct sequences once and build the pair-major image the duplex kernels read on the device, and a sequence's
 * result bits depend on its own letters only, so pair p of an indexed batch has the bits it has in the expanded batch.
 *
 * The batched entry points on an indexed batch:
 *   per pair, through the index: rh_batch_results(p, ...), rh_batch_candidates(p, which, ...), rh_batch_logz (out[3p..3p+2]) and
 *     rh_batch_candidates_all (which = 0..4: npairs+1 offsets, the lists of the expanded batch -- a sequence's list is repeated
 *     for every pair that uses it; rh_batch_candidates_seq_all is the form that does not replicate);
 *   per distinct sequence: rh_batch_layout, rh_batch_results_all and rh_batch_device_views describe bp [nseq][tri_stride],
 *     up [nseq][up_ld] and hp [npairs][hp_stride]; rh_batch_fallbacks which = 0 / 2 lists distinct-sequence indices, each once,
 *     which = 1 / 3 pair indices.  A sequence that leaves the double range flags every pair that references it.
 *   rh_debug_batch_allow_mask: which = 0, k = distinct sequence k; which = 1, k = pair k.  It returns 1 when that mask does not
 *     exist: always after rh_batch_upload_indexed, which takes no constraint. */
int rh_batch_upload_indexed(rh_ctx* ctx, int nseq, const char* const* seqs, const int* lens,
                            int npairs, const int* first, const int* second);
/* rh_batch_upload_indexed under structure constraints, given once per distinct sequence.  RH_MODEL_VIENNA_BL only: any other model
 * with at least one non-NULL constraint is RH_ERR_UNSUPPORTED.
 *   cons[k]: the constraint of the fold of sequence k, in the fold_constrained alphabet of rh_bpp.  The sequence is folded once,
 *     under it; every pair that uses k reads that fold.
 *   co_first[k], co_second[k]: sequence k's share of a joint constraint when it is s1 / s2 of a pair.  The joint constraint of
 *     pair p is pad(co_first[first[p]], n1) + pad(co_second[second[p]], n2), pad cutting a string at the sequence's length and
 *     filling it with '.', and means what co_cons[p] means to rh_batch_upload_constrained.  RactIP's translation (src/ractip.cpp:
 *     409-440) writes '(' for '[' in the share of s1, ')' for ']' in the share of s2 and 'x' for letters paired inside their own
 *     molecule; the whole alphabet is accepted: brackets matched inside one share stay pairs inside that molecule, and a '(' the
 *     first share leaves open pairs with a ')' the second share leaves open, the last one open with the first one closing.  Under
 *     RH_HYBRID_DUPLEX the shares are checked and otherwise unused, as co_cons is.
 * Any of the three arrays, and any entry, may be NULL (no constraint).  With no constraint at all this IS rh_batch_upload_indexed:
 * the same bits, no masks, the two-molecule sweeps seeded from the folds.  With masks the sweeps are not seeded.
 * Everything is checked before anything is staged (RH_ERR_ARG; the previous batch stays in place): indices, lengths and sequences
 * as rh_batch_upload_indexed does; a fold constraint as "sequence k: ..." with the text of rh_batch_upload_constrained; a joint
 * constraint as "pair p: ..." for the first pair p whose string is unbalanced -- a ')' left open in the share of s1, a '(' in the
 * share of s2, or different numbers left open by the two -- or forces a pair of non-complementary letters, inside a share or
 * across the cut.  A share that no pair uses in its role is not reported.
 * The fold masks come from one host pass per distinct sequence; the joint masks are composed on the device from one host pass per
 * distinct sequence and role, the host's work per pair being O(open brackets).  Everything downstream works as on any indexed
 * batch. */
int rh_batch_upload_indexed_constrained(rh_ctx* ctx, int nseq, const char* const* seqs, const int* lens,
                                        int npairs, const int* first, const int* second,
                                        const char* const* cons, const char* const* co_first, const char* const* co_second);
/* The index of the last upload (any pointer may be NULL; first / second hold npairs entries); for a plain rh_batch_upload:
 * nseq = 2*npairs, first[p] = 2p, second[p] = 2p+1. */
int rh_batch_index(rh_ctx* ctx, int* nseq, int* npairs, int* first, int* second);
int rh_batch_compute(rh_ctx* ctx);
int rh_batch_results(rh_ctx* ctx, int p,
                     double* bp1_tri, double* bp2_tri, double* up1, double* up2,
                     double* hp, double* logZ3 /* logZ(s1), logZ(s2), logZ(duplex) */);

/* Per-pair scalars of the whole batch in one copy: out[3p..3p+2] = logZ(s1), logZ(s2),
 * logZ(duplex) -- what a z-score shard gathers across GPUs (src/ractip.cpp:1655-1663). */
int rh_batch_logz(rh_ctx* ctx, double* out);

typedef struct rh_cand {
    int i, j; /* 1-based letters; for `up`: i = 0-based position, j = width index (region i..i+j, src/ractip.cpp:621-627) */
    float p;  /* probability narrowed to float exactly as the reference does (src/ractip.cpp:82-83) */
} rh_cand;
/* which: 0 = bp1 (p > th), 1 = bp2, 2 = hp, 3 = up1, 4 = up2.  Writes at most `cap`
 * entries in row-major scan order and returns the total number found (>= 0) or an error. */
int rh_batch_candidates(rh_ctx* ctx, int p, int which, float threshold, rh_cand* out, int cap);

/* The same scan for EVERY pair of the batch in two kernels and three copies (the z-score loop needs 5 scans
 * for each of 1000 pairs): out holds the concatenated lists, pair p owns out[first[p] .. first[p+1]) (first has
 * npairs+1 entries).  Returns the total number found (>= 0; only min(total, cap) entries are written) or an error. */
int rh_batch_candidates_all(rh_ctx* ctx, int which, float threshold, rh_cand* out, int cap, int* first);
/* Thresholded bp (what = 0) or up (what = 1) lists per DISTINCT sequence of the last upload: `first_out` has nseq+1 entries, sequence k
 * owns out[first_out[k] .. first_out[k+1]).  Records are those of rh_batch_candidates_all, which = 0 / 3.  On a plain
 * rh_batch_upload the sequences are 2p = s1, 2p+1 = s2 of pair p. */
int rh_batch_candidates_seq_all(rh_ctx* ctx, int what, float threshold, rh_cand* out, int cap, int* first_out);

/* Dense results of the whole batch in three copies, in the padded device layout described by rh_batch_layout:
 *   bp [nseq][tri_stride]      (rh_batch_upload: nseq = 2*npairs, sequence 2p = s1 of pair p; rh_batch_upload_indexed: the distinct
 *                               sequences; each table in the reference's triangular layout for ITS n)
 *   up [nseq][up_ld]           (n*max_w entries used, row-major position x width)
 *   hp [npairs][hp_stride] with row pitch hp_ld       logz [3*npairs]
 * Any pointer may be NULL. */
int rh_batch_layout(rh_ctx* ctx, size_t* tri_stride, int* up_ld, size_t* hp_stride, int* hp_ld);
int rh_batch_results_all(rh_ctx* ctx, double* bp, double* up, double* hp, double* logz);

/* ---- dense results at the width the reference stores them: packed float32, narrowed on the device ----
 * The reference keeps every probability as float (VF, VVF, pair_info::p: src/ractip.cpp:82-83).  The packed image is three arrays
 * of floats, each a row of blocks at their tight sizes in the layouts at the top of this file:
 *   bp: sequence k owns T(n_k) floats at bp_off[k];  up: n_k*max_w floats at up_off[k];  hp: pair p owns (n1+1)*(n2+1) floats at
 *   hp_off[p], row-major, 1-based, row 0 / column 0 zero -- what rh_batch_results hands back per pair, as floats.
 * Sequences are those of rh_batch_layout: 2p = s1, 2p+1 = s2 of pair p after rh_batch_upload, the distinct sequences after
 * rh_batch_upload_indexed (bp / up per distinct sequence, hp per pair).  Offsets count elements, are 64-bit (512 pairs of n = 2000
 * hold 2.05e9 hp entries, 8.2e9 bytes) and multiples of 4 (16 bytes); the floats between the end of one block and the start of the next
 * are padding and hold 0, so equal results give equal images byte for byte.  totals[k] (= the last entry of each offset array) is
 * the number of floats of the bp, up and hp image. */
/* element offsets of the packed float image of the last upload (known from the lengths: valid after the upload, before the compute) */
int rh_batch_packed_layout(rh_ctx* ctx, size_t* bp_off /*nseq+1*/, size_t* up_off /*nseq+1*/, size_t* hp_off /*npairs+1*/, size_t totals[3]);
/* bp, up, hp of the whole batch narrowed to float on the device, packed as rh_batch_packed_layout says; any pointer may be NULL; logz as rh_batch_results_all.
 * Element e of every block equals (float) of the corresponding double of rh_batch_results bit for bit (one IEEE conversion, round
 * to nearest, float subnormals kept), whichever path computed it.  Both models, both rh_set_hybrid sources, every kind of upload;
 * errors as rh_batch_results_all ("no computed pair batch").  Half the bytes of rh_batch_results_all cross the bus, and the host
 * narrows nothing.  The first call allocates a device staging buffer as large as the images asked for (about 0.5 GB per 256 pairs
 * of n = 500); it is kept, grows only, and goes with the context.  A table of 2^31 entries or more is RH_ERR_UNSUPPORTED. */
int rh_batch_results_packed_f32(rh_ctx* ctx, float* bp, float* up, float* hp, double* logz);
/* Measurement aid: device time (ms, one HIP event pair) of the pack kernel of the last rh_batch_results_packed_f32 that fetched a table. */
int rh_batch_pack_time(rh_ctx* ctx, double* ms);

/* Page-locked host memory for result buffers (hipHostMalloc): device-to-host copies into it run at the full DMA rate and,
 * issued from two contexts, overlap the other context's kernels (the reference's result containers are plain std::vector,
 * src/ractip.cpp:82-83; a host that wants the dense matrices at PCIe speed hands these buffers to rh_batch_results_all).
 * rh_host_alloc returns NULL on failure; any context's device is fine. */
void* rh_host_alloc(rh_ctx* ctx, size_t bytes);
void rh_host_free(rh_ctx* ctx, void* p);

/* Device time (ms, HIP events on the context's streams) spent by the last
 * rh_batch_compute in: [0] McCaskill inside sweep, [1] McCaskill outside sweep
 * (+posterior), [2] duplex sweeps, [3] whole compute.  Launch counts in n_launch[0..2]. */
int rh_batch_timings(rh_ctx* ctx, double ms[4], int n_launch[3]);

/* Names (as a kernel trace prints them) of the sweep kernels the last rh_batch_compute launched, per phase
 * [0] McCaskill inside, [1] outside (+posterior), [2] duplex: the per-diagonal kernel, the block-product kernel ("" if
 * none) and how many of the phase's n_launch were block-product launches. */
int rh_batch_kernels(rh_ctx* ctx, const char* fine[3], const char* far[3], int n_far[3]);

/* Measurement aid: rh_set_overlap(ctx, 0) makes rh_batch_compute run the duplex sweeps, the McCaskill inside sweep and
 * the outside sweep one after the other instead of overlapping the duplex stream with the McCaskill stream, so that
 * rh_batch_timings returns each phase's device time with nothing else on the GPU (what a kernel trace reports per
 * kernel).  Results are unchanged.  Default: overlap on. */
int rh_set_overlap(rh_ctx* ctx, int on);

/* Measurement aid: rh_set_kernel_timing(ctx, cls) brackets every launch of ONE class of sweep kernels by a HIP event pair on its
 * stream (cls 0 = McCaskill inside sweep kernel, 1 = its block products incl. operand packing, 2 = outside sweep kernel, 3 = its
 * block products, 4 = duplex sweep kernel; -1 = off, the default) -- launch graphs are bypassed meanwhile.  After rh_batch_compute,
 * rh_kernel_times returns how many launches of that class ran and the sum of their durations: the live counterpart of the
 * per-kernel average of a rocprofv3 kernel trace (bench.py: roofline.avg_launch_us).  Results are unchanged. */
int rh_set_kernel_timing(rh_ctx* ctx, int cls);
int rh_kernel_times(rh_ctx* ctx, int* n_launches, double* total_ms);

/* Which problems of the last rh_batch_compute left the double range on the scaled linear path and were recomputed by the
 * log-space kernels (rh_last_path / rh_last_hybrid_path == 3): which = 0: sequence indices (2p = s1 of pair p), 1: pair
 * indices of the duplex.  Only those problems are recomputed; every other problem keeps its linear-path result.  Writes at
 * most `cap` indices, returns how many there are.  (The reference's log-space arithmetic, LogSpace.hpp:232-244, never
 * leaves its range; this is how the fast path keeps that guarantee.)
 * which = 2: the sequence indices that left the range with the default scale exponent and were recomputed on the linear kernels
 * with another one (CONTRAfold model: 0.45, 1.5 or 0 per unit span instead of 0.12) -- they are NOT in the list of which = 0.
 * With rh_set_scale_memory(ctx, 1): when one exponent held more than half of a batch of at least eight sequences, the next
 * rh_batch_compute starts on it.
 * Vienna-BL model: the whole batch is run again with another exponent (0.7, 1.8 or 0 instead of 0.28); which = 2 then lists the
 * sequences that made it necessary.
 * which = 3: the pair indices whose DUPLEX sweeps left the range with the default exponent (0.65 per unit of i + (L2+1-j)) and were
 * recomputed on the linear duplex kernels with another one (1.3, 2.2, 0.3 or 0; CONTRAfold model) -- they are NOT in the list of
 * which = 1. */
int rh_batch_fallbacks(rh_ctx* ctx, int which, int* out, int cap);

/* Scale-exponent memory (default OFF).  Off: every rh_batch_compute starts on the default exponent, so a sequence's result bits
 * depend on its own letters only (the reference, src/ractip.cpp:195-245, is deterministic per input) and sharded + gathered
 * results equal single-context results bit for bit whatever each context computed before.  On: a stream of batches of one kind
 * (e.g. long, very stable RNAs) pays the failed first pass once instead of once per batch; results then differ by a few ulp
 * with the context's history, which voids the bit-for-bit shard guarantee.  Turning it off also forgets the remembered exponent. */
int rh_set_scale_memory(rh_ctx* ctx, int on);

/* Device pointers of the last batch (for callers that keep results on the GPU):
 * bp tables [nseq][tri_stride] (rh_batch_upload: sequence 2p = s1 of pair p, 2p+1 = s2; indexed: the distinct sequences),
 * hp tables [npairs][hp_stride]. */
int rh_batch_device_views(rh_ctx* ctx, const double** bp, size_t* tri_stride,
                          const double** hp, size_t* hp_stride, int* hp_ld);

/* ---- local folding: window-averaged bp and accessibility of a long sequence (the quantity RNAplfold defines; an extension, the
 * reference folds a sequence only as a whole) ----
 * A sequence of n letters, a window of W >= 2 letters and a step 1 <= S <= W; We = min(W, n).  n <= W: one window, start 0, n letters.
 * Otherwise m = ceil((n - W) / S) windows start at 0, S, .., (m-1) S and a last one at n - W, so that it ends at the last letter:
 * nw = m + 1 distinct, increasing starts.  Every window is folded as a sequence of its own (its end letters have no neighbour, as in
 * rh_fold) under the context's model, arithmetic mode, max_w and region-accessibility setting; no structure constraint applies.
 * Letters 0-based; a run of len letters from i lies in window k iff start[k] <= i and i + len <= start[k] + We.
 *   bp_loc(i, j), 1 <= j - i < We: the mean of bp_k(i - start[k], j - start[k]) over the windows that contain i..j; 0 if none does.
 *   up_loc[i][w]: the mean of up_k[i - start[k]][w] over the windows that contain i..i+w; 0 if none does or i + w >= n.
 *   logz_win[k]: log Z of window k.
 * A mean is a plain double sum in increasing window order followed by ONE division by the count: the order is part of the interface,
 * and the result bits do not depend on how the windows were chunked (each window's bits depend on its own letters only; under
 * RH_MODEL_VIENNA_BL that holds while no window leaves the double range on the default scale exponent, see rh_batch_fallbacks).
 * With S > 1 a run of more than We - S + 1 letters may lie in no window: its entry is 0, not a probability.
 * Layouts (offsets are size_t: n = 1e6, W = 1000 is 1e9 doubles):
 *   bp_band: n rows of ld = We doubles, bp_band[i*ld + d] = bp_loc(i, i + d); column 0 and every entry with i + d >= n hold 0;
 *   up: n * max_w doubles, up[i*max_w + w], as everywhere else;  logz_win: nw doubles.
 *
 * rh_local_fold checks its arguments first: a rejected call (RH_ERR_ARG) leaves the previous local result and the previous batch in
 * place.  Then it folds the windows in chunks of consecutive windows, each a fold-only batch, adds every chunk's tables into band
 * accumulators on the device and divides by the counts behind the last chunk; nothing but the letters crosses the bus.  Afterwards
 * the context's batch is the last chunk, a fold-only batch as after rh_fold (the pair fetches answer "no computed pair batch"); the
 * local result lives in buffers of its own, which grow only and go with the context, and stays valid until the next rh_local_fold.
 * A failure behind the checks (RH_ERR_OOM, RH_ERR_HIP) leaves no local result. */
int rh_local_fold(rh_ctx* ctx, const char* seq, int n, int window, int step);
/* shape of the last local result; any pointer may be NULL, starts receives nw entries */
int rh_local_layout(rh_ctx* ctx, int* n, int* ld, int* nw, int* max_w, int* starts);
/* the last local result in the layouts above; any pointer may be NULL */
int rh_local_results(rh_ctx* ctx, double* bp_band, double* up, double* logz_win);
/* Thresholded lists of the last local result, scanned on the device over the band: what = 0: bp_loc, records with 1-based letters
 * i < j of the long sequence; what = 1: up_loc, i = 0-based position, j = width index (all n * max_w entries).  Row-major order, the
 * float narrowing and the p > threshold comparison of rh_batch_candidates.  Writes at most `cap` records, returns the total found. */
int rh_local_candidates(rh_ctx* ctx, int what, float threshold, rh_cand* out, int cap);
/* Test and measurement aid: windows per chunk of rh_local_fold, 1..32768; 0 (default) = automatic, the largest chunk whose McCaskill
 * tables stay under the byte budget kLocalChunkBytes of ractip_amd/csrc/local_windows.h (4 GiB).  Under rh_local_duplex a window's
 * bytes also count its pair (hybridization tables, hp block, under RH_HYBRID_COFOLD the tables of query + window), the query's fold
 * counts once per chunk, and a chunk has at most 32767 windows.  Results are unchanged. */
int rh_set_local_chunk(rh_ctx* ctx, int windows);
/* Measurement aid: device time (ms, HIP event pairs) of the last rh_local_fold: ms[0] the folds (the computes of its chunks), ms[1]
 * the accumulate and finish kernels, plus the scan kernels of the rh_local_candidates calls since. */
int rh_local_times(rh_ctx* ctx, double ms[2]);

/* ---- span-limited folding: the whole long sequence, pairs within max_span letters ----
 * Inputs: n letters, max_span = L >= 2, Le = min(L, n).
 * Ensemble: that of rh_fold under the context's Vienna-BL model (1.8 semantics, BL* tables or a parameter file), the treatment of
 * unknown letters and of the end letters included.  Letters a < b (1-based) may pair only if b - a < L; nothing else changes.  With
 * L >= n it is the ensemble of rh_fold.  Unlike rh_local_fold, which averages windows folded as if the molecule ended at their
 * borders, this is one consistent ensemble of the whole molecule with one partition function (ViennaRNA's --maxBPspan; RNAplfold at
 * W = n), in O(n L) memory and O(n L^2) time.  The exterior sums are kept as logarithms, so the length of the sequence cannot take
 * the call out of the double range (ractip_amd/csrc/span_fold.h).
 * Results, in the local-fold layouts: bp_band[i*ld + d] = P(i, i+d), i 0-based, ld = Le, column 0 and every entry with i + d >= n
 * hold 0; up[i] (width 1) = 1 - sum_j P(i, j); logz_win[0] = log Z of the whole sequence.  They are fetched through rh_local_layout
 * (which reports nw = 1, starts = {0}, ld = Le, max_w = 1 whatever the context's max_w is), rh_local_results and
 * rh_local_candidates.  A span fold replaces the previous local-fold result exactly as an rh_local_fold would: it drops the hp part
 * of an rh_local_duplex and leaves the result of rh_local_duplex2 alone.  The context's batch is neither read nor changed.
 * Refusals.  RH_ERR_ARG: NULL sequence, n < 1, L < 2, sizes that overflow.  RH_ERR_UNSUPPORTED: CONTRAfold contexts, 2.x-semantics
 * contexts, contexts in RH_MODE_LOG (there is no log-space version).  Both leave the previous local result and the batch in place;
 * rh_last_error names the reason.  Structure constraints: rh_span_fold_constrained below.
 * A band cell that leaves the double range under the context's scale exponent sends the call through the exponent ladder (0.28 per
 * unit span, then 0.7, 1.8, 0): the closed value of a pair outside (1e-280, 1e280) or not a number, a multiloop sum above 1e280, an
 * outside value or a posterior above 1e300, an exterior logarithm that is not finite.  A closed value that underflows to exactly 0 is
 * not tested itself: it times the pair's outside value is the pair's probability, so the outside value passes 1e300 for every pair
 * with a probability above 5e-24.  When no exponent holds, the call returns RH_ERR_UNSUPPORTED ("no scale exponent of the ladder
 * ...") and leaves no local result, as RH_ERR_OOM does (buffers grow only and go with the context); everything else the context
 * holds stays.
 * The CONTRAfold model: rh_set_span_contrafold below; a CONTRAfold context that did not ask is refused. */
int rh_span_fold(rh_ctx* ctx, const char* seq, int n, int max_span);
/* Span folds under the CONTRAfold model, opt-in per context (default off: a CONTRAfold context refuses every span call as above).  On
 * a RH_MODEL_VIENNA_BL context the call is accepted and changes nothing.  On, for a RH_MODEL_CONTRAFOLD context, rh_span_fold,
 * rh_span_fold_acc and rh_span_fold_batch with max_w == 1 and their constrained forms with a NULL constraint (every entry NULL for a
 * batch) compute the span-limited ensemble under the context's CONTRAfold weights: the ensemble of rh_fold on that context (the
 * derivations the inside recurrences of InferenceEngine.ipp count) restricted to the derivations in which letters a < b pair only if
 * they are complementary and b - a < L; with L >= n it is the ensemble of rh_fold.  Unknown letters are encoded as in the batch path.
 * bp_band, up (width 1, max(0, 1 - sum_j bp(i, j))) and log Z come back through the same fetches, batches and candidates included.
 * The exponent ladder is the CONTRAfold one (0.12 per unit span, then 0.45, 1.5, 0); the context's batch, rh_fold's bits and the batch
 * path's state are untouched.  Still RH_ERR_UNSUPPORTED with the switch on, each leaving the previous result in place: max_w > 1
 * unless rh_set_region_accessibility is on as well (see rh_span_fold_acc), a constraint that is not NULL (the model takes none), a
 * context in RH_MODE_LOG. */
int rh_set_span_contrafold(rh_ctx* ctx, int on);
int rh_get_span_contrafold(const rh_ctx* ctx);
/* Measurement aid: device time (ms, HIP event pairs) of the last rh_span_fold: ms[0] the inside and outside sweeps (2 Le launches),
 * ms[1] the two exterior passes and the finish kernel. */
int rh_span_times(rh_ctx* ctx, double ms[2]);
/* The same ensemble with region accessibilities, what RactIP's integer programme takes under the default model:
 *   up[i*max_w + w] = P(letters i+1 .. i+1+w all unpaired), i 0-based, 0 <= w < max_w, and 0 where the run passes letter n.
 * max_w in 1..64 (the range of rh_set_max_w; anything else: RH_ERR_ARG, rh_last_error names it).  The context's own max_w setting is
 * neither read nor changed.  Checks, refusals and the exponent ladder are those of rh_span_fold; bp_band and logz_win[0] are its
 * bits.  rh_local_layout reports this max_w, rh_local_results and rh_local_candidates (what = 1: all n * max_w entries) serve the
 * result as after an rh_local_fold at that max_w.
 * max_w = 1 is rh_span_fold, bit for bit (1 - the row sums of the band).  For max_w > 1 EVERY column, column 0 included, is the sum
 * over where the run can lie -- the exterior, a hairpin loop, a gap of a loop with one enclosed pair, a run of a multiloop -- taken
 * on the band tables behind the outside sweep and clamped to at most 1, as rh_fold does for whole sequences at max_w > 1.  The
 * exterior part is a difference of the exterior logarithms.  The stage runs inside the ladder attempt that kept the band in range;
 * a value that is not finite sends the call to the next exponent.  Every sum has a fixed order: the bits depend on the letters, L,
 * max_w and the context's model only.
 * The CONTRAfold model.  A context with rh_set_span_contrafold AND rh_set_region_accessibility on answers max_w 1..64 (this call, the
 * batch, the constrained forms with NULL constraints); with region accessibility off max_w > 1 stays RH_ERR_UNSUPPORTED.  up is
 * Z(the run's letters forbidden to pair) / Z over the derivations of the span ensemble.  Column 0 has the bits of the max_w = 1 call
 * (1 - the row sums of the band), as rh_fold keeps it under this model; the columns w >= 1 are the sum of five terms on the band
 * tables -- the exterior, a hairpin loop, a gap of a loop with one enclosed pair, the leading letters of a multiloop branch, and the
 * trailing letters of a multiloop by the banded chain of products that counts every derivation -- clamped to at most
 * 1.  bp_band and log Z have the bits of the max_w = 1 call.  An item then takes four more band tables of scratch. */
int rh_span_fold_acc(rh_ctx* ctx, const char* seq, int n, int max_span, int max_w);
/* Measurement aid: device time (ms, HIP event pairs) of the accessibility stage of the last rh_span_fold_acc at max_w > 1: ms[0] the
 * hairpin part (suffix sums and their sums per run), ms[1] the gap sums of the loops with one enclosed pair, ms[2] the final kernel
 * (exterior, gap and multiloop parts).  On a CONTRAfold context the split is: ms[0] everything but the multiloop chain (hairpin
 * sums, gap sums, column 0, the kernel that adds the four direct terms), ms[1] the S build of the chain (one launch per diagonal),
 * ms[2] the max_w - 1 links of the chain with the kernels that add each width's term.  RH_ERR_ARG where the last span fold ran at
 * width 1. */
int rh_span_acc_times(rh_ctx* ctx, double ms[3]);
/* Span folds in batches: `count` sequences of ragged lengths n[k] through one set of launches, at one max_span and one max_w.
 * Item k is rh_span_fold_acc(ctx, seqs[k], n[k], max_span, max_w): the same ensemble, layouts (ld = min(max_span, n[k]),
 * up[i*max_w + w]) and clamping, and the bits of that single call made on this context.  The single calls run the same kernels as a
 * batch of one.  The item is a dimension of every launch: one launch per diagonal below the largest min(max_span, n[k]), and one
 * workgroup per item in the exterior passes.  The exponent ladder runs per item: the items of an attempt that stayed in range are
 * finished on that attempt's exponent, the others form the next attempt, so every item ends on the exponent its single call ends on.
 * An item for which no exponent holds gets status RH_ERR_UNSUPPORTED, which its fetches return; the call still returns RH_OK and
 * serves the other items.
 * The batch is cut into chunks of consecutive items whose band tables and gap sums fit rh_set_span_batch_bytes (0, the default: 16 GiB,
 * a setting that has not been tuned; a chunk holds at least one item); chunks run one after the other and change no bit.
 * The result lives in buffers of its own until the next rh_span_fold_batch: it neither reads nor changes the context's batch, the
 * local result (rh_local_*, the single span calls) or the result of rh_local_duplex2, and these calls leave it alone.
 * Refusals.  RH_ERR_ARG: count < 1, a NULL array, a NULL sequence, n[k] < 1, max_span < 2, max_w outside 1..64, sizes that overflow
 * (rh_last_error names the item).  RH_ERR_UNSUPPORTED: as rh_span_fold.  Both leave the previous batch result in place.
 * Structure constraints: rh_span_fold_batch_constrained below. */
int rh_span_fold_batch(rh_ctx* ctx, const char* const* seqs, const int* n, int count, int max_span, int max_w);
int rh_span_batch_layout(rh_ctx* ctx, int* count, int* max_span, int* max_w);
/* n, ld = min(max_span, n) and the status of one item; RH_ERR_ARG for an item outside the batch */
int rh_span_batch_item(rh_ctx* ctx, int item, int* n, int* ld, int* status);
/* bp_band [n][ld], up [n][max_w] and log Z (one double) of one item; any pointer may be NULL */
int rh_span_batch_results(rh_ctx* ctx, int item, double* bp_band, double* up, double* logz);
/* Thresholded list of one item, by the scan kernels of rh_local_candidates: what = 0 the band, 1 up; same records, order and return */
int rh_span_batch_candidates(rh_ctx* ctx, int item, int what, float threshold, rh_cand* out, int cap);
/* Table memory (band tables + gap sums, bytes) one chunk of a span batch may take; 0: the default */
int rh_set_span_batch_bytes(rh_ctx* ctx, size_t bytes);
/* Measurement aid: device time (ms, HIP event pairs) of the last rh_span_fold_batch, summed over its chunks and ladder attempts: ms[0]
 * the inside and outside sweeps, ms[1] the exterior passes and the finish kernels, ms[2] the accessibility stage. */
int rh_span_batch_times(rh_ctx* ctx, double ms[3]);
/* Span folds under a structure constraint.  `constraint`: a string in the fold_constrained alphabet of rh_bpp (or NULL); shorter than
 * n it is padded with '.', longer the surplus is ignored.  The ensemble is that of rh_span_fold_acc with one more restriction: letters
 * a < b may pair only if b - a < max_span AND the constraint allows the pair, by the rule of rh_fold_constrained -- 'x' never pairs,
 * '<' only with a later letter, '>' only with an earlier one, a matched '(' ')' removes every pair that conflicts with it (it does not
 * force the pair itself), '|' and '.' restrict nothing.  With max_span >= n it is the ensemble of rh_fold_constrained.  Model, unknown
 * letters, end letters, layouts, the exponent ladder and the local-result slots are those of rh_span_fold_acc; a NULL constraint, or
 * one that restricts nothing, gives rh_span_fold_acc bit for bit.  No n x n mask is built: the constraint costs 8 bytes per letter.
 * Refusals, each leaving the previous local result in place.  RH_ERR_ARG: those of rh_span_fold_acc; unbalanced brackets or a bracket
 * pair of non-complementary letters, with the reason rh_fold_constrained gives; a matched bracket pair (a, b) with b - a >= max_span
 * (rh_last_error names a, b and max_span); a constraint over 2^30 letters or more.  RH_ERR_UNSUPPORTED: as rh_span_fold. */
int rh_span_fold_constrained(rh_ctx* ctx, const char* seq, int n, const char* constraint, int max_span, int max_w);
/* rh_span_fold_batch under constraints: item k is rh_span_fold_constrained(ctx, seqs[k], n[k], constraints[k], max_span, max_w), bit
 * for bit.  `constraints`, and any entry of it, may be NULL.  The result goes to the span-batch slots (rh_span_batch_*).  The per-letter
 * records are not counted in the chunk budget, so the chunks do not depend on the constraints.  Refusals: those of rh_span_fold_batch
 * and, per item, of rh_span_fold_constrained (rh_last_error names the item); every check of every item runs before anything is
 * staged, and a refused call leaves the previous batch result in place. */
int rh_span_fold_batch_constrained(rh_ctx* ctx, const char* const* seqs, const int* n, int count, const char* const* constraints, int max_span, int max_w);

/* ---- local hybridization: window-averaged hp of a query on a long target ----
 * Two molecules s1 (n1 letters) and s2 (n2 letters).  `windowed` (1 or 2) names the one that is cut into the windows of rh_local_fold
 * (same W, S, We, starts); the other one, the query, is always whole.  For window k the engine computes hp_k of the pair
 * (query, window k) if windowed = 2, (window k, query) if windowed = 1, under the context's model, arithmetic mode, rh_set_hybrid and
 * rh_set_duplex_mode settings, without constraints.
 *   hp_loc(i, j), 1-based letters of s1 and s2: the mean of hp_k at the translated coordinates over the windows that contain the
 *     windowed molecule's letter -- a plain double sum in increasing window order, then ONE division by the count, the rule of bp_loc;
 *     the order is part of the interface and the bits do not depend on the chunking.  Every letter lies in a window: no holes.
 *   logz_pair[k]: log Z of the two-molecule or duplex ensemble of window k.
 * Layout of hp: (n1+1) * (n2+1) doubles, row-major, 1-based, row 0 and column 0 zero -- what rh_duplex returns; offsets are size_t.
 * WHAT THE MEAN MEANS depends on the hybridization source.  Under the duplex-only sources (the CONTRAfold DuplexEngine, Vienna
 * pf_duplex) each window's ensemble is normalized over the duplexes inside that window: a window without the true site still spends
 * its whole probability somewhere, and the mean is a probability GIVEN THAT THE QUERY BINDS IN THE WINDOW.  Under RH_HYBRID_COFOLD
 * the ensemble of a window includes the unbound state, and the mean is a probability in RNAplfold's sense.  No Z-weighted
 * combination of the windows is offered for the duplex sources.
 *
 * rh_local_duplex checks its arguments first ("local duplex: ..."): a rejected call (RH_ERR_ARG) leaves the previous local result,
 * the previous local hp result and the previous batch in place.  Then it runs chunks of consecutive windows, each an indexed batch
 * (rh_batch_upload_indexed) whose sequence 0 is the query and whose sequences 1..c are windows, paired (0, k) or (k, 0).  For the
 * windowed molecule the call is also rh_local_fold: bp_band, up and logz_win of that molecule carry the bits a plain rh_local_fold
 * gives and are served by rh_local_layout / rh_local_results / rh_local_candidates / rh_local_times (whose accumulate time then
 * includes the hp kernels).  The query's own bp / up are not part of the local result (rh_fold).  Afterwards the context's batch is
 * the last chunk, an ordinary computed indexed batch.
 * One window (W >= the windowed molecule): hp and logz_pair[0] have the bits of rh_duplex(s1, s2) under the same settings.  Under
 * RH_HYBRID_COFOLD that call's two-molecule sweeps are not seeded from folds (it has none), so the one compute of a one-window call
 * is not either; with two windows or more the chunks are seeded like every batch with folds, whose hp differs from the unseeded
 * one in the last bits on the scaled linear path. */
int rh_local_duplex(rh_ctx* ctx, const char* s1, int n1, const char* s2, int n2, int windowed, int window, int step);
/* shape of the last local hp result; any pointer may be NULL.  "no local hybridization result" before the first rh_local_duplex and
 * after a later rh_local_fold, which replaces the fold part and drops the hp part. */
int rh_local_hp_layout(rh_ctx* ctx, int* n1, int* n2, int* windowed, int* nw);
/* hp_loc and logz_pair (nw doubles) in the layout above; any pointer may be NULL.  rh_local_candidates(what = 2) scans hp_loc on the
 * device: records (i, j) 1-based over 1..n1 x 1..n2 in row-major order, narrowed to float before p > threshold. */
int rh_local_hp_results(rh_ctx* ctx, double* hp, double* logz_pair);

/* ---- local hybridization of two long molecules: both cut into windows ----
 * s1 (n1 letters) is cut into the windows of rh_local_fold with (window1, step1): We1 = min(window1, n1), starts a_0 < .. < a_{nw1-1};
 * s2 (n2 letters) with (window2, step2): We2, starts b_0 < .. < b_{nw2-1}.  For every (k, l) the engine computes h_kl, the hp matrix of
 * the pair (window k of s1, window l of s2), under the context's model, arithmetic mode, rh_set_hybrid and rh_set_duplex_mode
 * settings, without constraints; logz_pair[k*nw2 + l] is that pair's log Z.
 *   hp_loc2(i, j), 1-based letters of s1 and s2, is a SUM OF ROW SUMS followed by one division:
 *     acc = 0
 *     for k in increasing order over the windows of s1 that contain letter i:
 *         r = 0
 *         for l in increasing order over the windows of s2 that contain letter j:  r += h_kl(i - a_k, j - b_l)
 *         acc += r
 *     hp_loc2(i, j) = acc / (c1(i) * c2(j))        c1, c2: the numbers of containing windows; their product is exact in double
 * All sums are plain double sums.  The association -- row sums first, not one running sum over (k, l) -- is part of the interface: it
 * lets the grid of window pairs be cut into rectangular tiles (a per-k row buffer is carried across the column tiles of a row block,
 * then added in increasing k), so that rows x cols pairs cost rows + cols folds and the result bits do not depend on the tiling.
 * Every letter lies in a window: no holes.  Layout of hp: (n1+1) * (n2+1) doubles, row-major, 1-based, row 0 and column 0 zero;
 * offsets are size_t (n1 = n2 = 1e5 is 1e10 doubles).  nw1 * nw2 must fit an int.
 * WHAT THE MEAN MEANS, as for rh_local_duplex: under the duplex-only sources each window pair's ensemble is normalized inside that
 * pair, so the mean is a probability GIVEN THAT THE MOLECULES BIND IN THAT PAIR OF WINDOWS; under RH_HYBRID_COFOLD each pair's
 * ensemble contains the unbound state.  Under every source the sum of a letter's row over the whole other molecule is NOT bounded by
 * 1: different columns are averaged over different window pairs, whose ensembles are separate (the letters of a planted site reach
 * 1.06 under cofold when computed on the CPU).  The values are evidence for the ILP, not a distribution over partners.
 *
 * rh_local_duplex2 checks its arguments first ("local duplex2: ..."): a rejected call (RH_ERR_ARG) leaves every previous result and
 * the previous batch in place.  Then it walks tiles of `rows` consecutive k by `cols` consecutive l -- row blocks in increasing k,
 * inside a row block column tiles in increasing l -- each one indexed batch WITH folds (rh_batch_upload_indexed): sequences
 * 0..rows-1 the windows of s1, rows..rows+cols-1 those of s2, pair a*cols + b = (a, rows + b).  A pair so has the bits it has in any
 * indexed batch with folds (under RH_HYBRID_COFOLD the two-molecule sweeps are seeded from the folds); only a call with one window
 * pair (nw1 * nw2 == 1) runs its one compute unseeded and answers with the bits of rh_duplex, as rh_local_duplex does.  The folds of
 * the windows are not part of the result (rh_local_fold).  The result lives in buffers of its own, which grow only and go with the
 * context, and stays valid until the next rh_local_duplex2: rh_local_fold and rh_local_duplex neither read nor drop it, and it
 * leaves theirs alone.  Afterwards the context's batch is the last tile, an ordinary computed indexed batch.  A failure behind the
 * checks (RH_ERR_OOM, RH_ERR_HIP) leaves no result of this kind. */
int rh_local_duplex2(rh_ctx* ctx, const char* s1, int n1, const char* s2, int n2, int window1, int step1, int window2, int step2);
/* shape of the last rh_local_duplex2; any pointer may be NULL, starts1 / starts2 receive nw1 / nw2 entries.  "no local hybridization
 * result of two windowed molecules" before the first call. */
int rh_local_hp2_layout(rh_ctx* ctx, int* n1, int* n2, int* nw1, int* nw2, int* starts1, int* starts2);
/* hp_loc2 and logz_pair (nw1 * nw2 doubles, row-major) in the layout above; any pointer may be NULL */
int rh_local_hp2_results(rh_ctx* ctx, double* hp, double* logz_pair);
/* Thresholded list of hp_loc2, scanned on the device: records (i, j) 1-based over 1..n1 x 1..n2 in row-major order, narrowed to float
 * before p > threshold, as rh_local_candidates(what = 2).  Writes at most `cap` records, returns the total found. */
int rh_local_hp2_candidates(rh_ctx* ctx, float threshold, rh_cand* out, int cap);
/* Test and measurement aid: the tile of rh_local_duplex2, rows x cols windows; (0, 0) (default) = automatic: the largest t with
 * 2t fold + t^2 pair + t rowbuf bytes under kLocalChunkBytes of ractip_amd/csrc/local_windows.h (rowbuf = (We1+1) * (n2+1) doubles,
 * the row buffer of one k), rows = min(t, nw1), cols = min(t, nw2), the unclipped side grown while the sum still fits.  Otherwise
 * rows, cols >= 1, rows + cols <= 32768 and rows * cols <= 32767; each is clipped to nw1 / nw2 at run time.  Results are unchanged.
 * rh_set_local_chunk does not apply to rh_local_duplex2.  rh_local_hp2_tile: the tile the last call ran, clipped. */
int rh_set_local_tile(rh_ctx* ctx, int rows, int cols);
int rh_local_hp2_tile(rh_ctx* ctx, int* rows, int* cols);
/* Measurement aid: device time (ms, HIP event pairs) of the last rh_local_duplex2: ms[0] the computes of its tiles, ms[1] the row, add
 * and finish kernels with the log Z copies, plus the scan kernels of the rh_local_hp2_candidates calls since. */
int rh_local_hp2_times(rh_ctx* ctx, double ms[2]);

/* ---- loader inspection (host only, no GPU, no context) ----
 * What the parameter loader holds after binding its sources, for checks of the binding itself (tests/test_bl_cells.py,
 * tests/test_vienna_par.py); not needed by a caller of the probability path.  Return 0, -1 (bad index / NULL) or
 * RH_ERR_PARAM (-4: the files could not be loaded).
 * rh_debug_vienna_cell: energy in the file's 10 cal/mol units of one cell of table 0 = stack[i][j], 1 = int11[i][j][k][l],
 * 2 = int21[i][j][k][l][m], 3 = int22[i][j][k][l][m][n] (pair types 0..7, nucleotides 0..4) of a flat BL* dump or
 * ViennaRNA parameter file (the conventions of src/boltzmann_param.c:5908-5971).
 * rh_debug_vienna_value: one entry (log Boltzmann weight) of the model built from (defaults_file, use_bl_param, bl_path,
 * param_file, semantics) in the install order of src/ractip.cpp:1563-1567; `table` codes 10..27 are listed next to the
 * function in ractip_amd/csrc/vienna_loader.cpp. */
int rh_debug_vienna_cell(const char* param_file, int table, int i, int j, int k, int l, int m, int n, double* energy);
int rh_debug_vienna_value(const char* defaults_file, int use_bl_param, const char* bl_path, const char* param_file, int semantics,
                          int table, int i, int j, int k, int l, double* out);

/* The allowed-pair mask of the last upload as the kernels read it: which = 0, sequence k (2p = s1 of pair p; of an indexed batch:
 * distinct sequence k), or which = 1, the concatenation s1+s2 of pair k.  *ld receives the row pitch; out (or NULL, to ask for ld first) receives ld*ld bytes, byte
 * [a*ld + b] != 0 iff letters a < b (1-based) may pair.  Returns 0, 1 if that batch has no mask, or an error. */
int rh_debug_batch_allow_mask(rh_ctx* ctx, int which, int k, unsigned char* out, int* ld);

/* ---- source-compatible pf_duplex surface (src/pf_duplex.h:25-28) ----
 * double pf_duplex(const char*, const char*); extern double** pr_duplex; void free_pf_duplex();
 * are provided by libractip_pfduplex (ractip_amd/csrc/pf_duplex_shim.cpp) on top of rh_duplex. */

#ifdef __cplusplus
}
#endif
#endif /* RACTIP_HOT_H */
