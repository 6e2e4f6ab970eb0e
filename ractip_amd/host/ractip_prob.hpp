// ractip_prob.hpp -- C++17 mirror of RactIP's probability-layer members on top of the
// C ABI (include/ractip_hot.h).  Same names, argument meaning, container layouts and
// error behaviour as the reference's private members (/root/reference/src/ractip.cpp):
//
//   void contrafold(const std::string& seq, VF& bp, VI& offset, VVF& up) const;   // :195-223
//   void contrafold(const std::string& seq, VF& bp, VI& offset, VVF& up, uint max_w) const;   // (no counterpart: region accessibility)
//   void contraduplex(const std::string& s1, const std::string& s2, VVF& hp) const; // :225-245
//   void rnaduplex(const std::string& s1, const std::string& s2, VVF& hp) const;  // :384-399 (--duplex branch)
//   void rnafold(const std::string& seq, VF& bp, VI& offset) const;                // :248-306  (Fasta::seq() of the original)
//   void rnafold(const std::string& seq, VF& bp, VI& offset, VVF& up, uint max_w) const;  // :308-382
//
// so that RactIP::solve (:536-548) can call them unchanged; see INTEGRATION.md for the
// two-line patch.  Failures surface as std::logic_error, which RactIP's main() already
// catches (:1684-1691).
#pragma once
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

struct rh_ctx;

namespace ractip_amd {

typedef unsigned int uint;
typedef std::vector<float> VF;   // src/ractip.cpp:82
typedef std::vector<VF> VVF;     // src/ractip.cpp:83
typedef std::vector<int> VI;

struct PairProbabilities {  // everything RactIP::solve consumes for one (s1,s2) pair
    VF bp1, bp2;
    VI offset1, offset2;
    VVF up1, up2, hp;
    double logZ1 = 0, logZ2 = 0, logZd = 0;
};

class ProbabilityEngine {
public:
    // th_hy: RactIP's hybridization threshold th_hy_ (contraduplex keeps hp >= th_hy, :237)
    explicit ProbabilityEngine(int device = 0, float th_hy = 0.1f, const char* param_file = nullptr);
    // the z-score shard inside ONE process (src/ractip.cpp:1636-1663): one rh_ctx and one host thread per listed
    // device.  The batched forms split their pairs into contiguous blocks, one per device, and return the results in
    // iteration order, so the float accumulation of the caller (:1655-1663) sees the same sequence of values as on one
    // GPU.  A device may be listed more than once (two contexts on one GPU: one's copies overlap the other's kernels).
    // The single-problem members use the first device.
    explicit ProbabilityEngine(const std::vector<int>& devices, float th_hy = 0.1f, const char* param_file = nullptr);
    ~ProbabilityEngine();
    ProbabilityEngine(const ProbabilityEngine&) = delete;
    ProbabilityEngine& operator=(const ProbabilityEngine&) = delete;

    void contrafold(const std::string& seq, VF& bp, VI& offset, VVF& up) const;
    // an extension (the reference refuses widths with --contrafold, :1511-1517): the same with region accessibility
    // up[i][w] = P(letters i..i+w unpaired), w < max_w, under the CONTRAfold model (rh_set_region_accessibility), in the layout
    // of the rnafold overload below.  The option is turned on for this call only: every other member sees width 1 as before.
    void contrafold(const std::string& seq, VF& bp, VI& offset, VVF& up, uint max_w) const;
    void contraduplex(const std::string& seq1, const std::string& seq2, VVF& hp) const;
    // the --duplex branch of RactIP::rnaduplex: pf_duplex() + pr_duplex copy (:390-398)
    void rnaduplex(const std::string& seq1, const std::string& seq2, VVF& hp) const;

    // the default CLI path: pf_fold + export_bppm (:288-304, 351-367) and pf_unstru's H+I+M+E (:370-375) with the BL*
    // energies, ViennaRNA-1.8 semantics -- PARITY UNPINNED (ViennaRNA is absent and unversioned); structure
    // constraints (use_constraint_, :271-291) are not supported.  A second context (RH_MODEL_VIENNA_BL) is created on
    // first use.
    void rnafold(const std::string& seq, VF& bp, VI& offset) const;
    void rnafold(const std::string& seq, VF& bp, VI& offset, VVF& up, uint max_w) const;
    // the same with use_constraint_ (:271-291): `str` is the FASTA structure line (Fasta::str()); '[' ']' 'e' become 'x',
    // everything else is handed to pf_fold's fold_constrained unchanged
    void rnafold(const std::string& seq, const std::string& str, VF& bp, VI& offset, VVF& up, uint max_w) const;
    // the DEFAULT branch of RactIP::rnaduplex (:400-458): co_pf_fold on s1+s2 with cut_point = |s1|+1, plist entries with
    // i < cut_point <= j and p > th_hy copied to hp[i][j-cut_point+1], everything else 0 (same model and caveats)
    void rnaduplex_cofold(const std::string& seq1, const std::string& seq2, VVF& hp) const;
    // ... with use_constraint_ (:409-440): str1 / str2 are the FASTA structure lines; '[' of s1 becomes '(' and ']' of s2
    // becomes ')' (the interaction is forced), and '(' ')' 'l' 'x' become 'x' (letters paired inside their own molecule)
    void rnaduplex_cofold(const std::string& seq1, const std::string& str1, const std::string& seq2, const std::string& str2, VVF& hp) const;

    // batched form for the z-score loop (:1638-1657): all DPs of all pairs in one device pass.  The batched members fetch the dense
    // tables as floats, narrowed on the device (rh_batch_results_packed_f32: the bits of (float)x on the host, half the bytes),
    // into page-locked buffers the engine keeps per context, and copy the blocks into the members
    std::vector<PairProbabilities> solve_probabilities(const std::vector<std::pair<std::string, std::string>>& pairs) const;
    // the same for the DEFAULT path (:544-548): rnafold(fa, bp, offset, up, max(1, max_w)) x2 + the co_pf_fold branch of
    // rnaduplex (hp entries with p > th_hy, :451-454) for every pair, Vienna-BL model; duplex = true: the --duplex branch
    std::vector<PairProbabilities> solve_probabilities_default(const std::vector<std::pair<std::string, std::string>>& pairs,
                                                               uint max_w = 15, bool duplex = false) const;

    // ... with use_constraint_: structures[p] = (str1, str2) are the FASTA structure lines of pair p, translated as rnafold(seq, str, ...)
    // and rnaduplex_cofold(seq1, str1, seq2, str2, ...) translate them (fold_constraint / joint_constraint below) and handed to one
    // constrained batch (rh_batch_upload_constrained); device shards split the structures with the pairs.  duplex = true: the folds
    // are constrained, hp is not (the --duplex branch takes no constraint, :390-398)
    std::vector<PairProbabilities> solve_probabilities_default(const std::vector<std::pair<std::string, std::string>>& pairs,
                                                               const std::vector<std::pair<std::string, std::string>>& structures,
                                                               uint max_w = 15, bool duplex = false) const;

    // Indexed batches (rh_batch_upload_indexed): every string of `seqs` is folded once, pair p = (seqs[i], seqs[j]) for (i, j) =
    // index_pairs[p] -- a screen of queries against targets, or a z-score loop that shuffles one molecule only.  The same
    // PairProbabilities per pair as the members above return for the expanded pairs.  Device shards split the pairs into the usual
    // contiguous blocks; each shard uploads only the sequences its block references.  (The members above do not dedupe: they fold
    // what they are given.)
    std::vector<PairProbabilities> solve_probabilities_indexed(const std::vector<std::string>& seqs,
                                                               const std::vector<std::pair<int, int>>& index_pairs) const;
    std::vector<PairProbabilities> solve_probabilities_default_indexed(const std::vector<std::string>& seqs,
                                                                       const std::vector<std::pair<int, int>>& index_pairs,
                                                                       uint max_w = 15, bool duplex = false) const;

    // the Vienna energy tables as RactIP::run installs them (:1563-1567): copy_boltzmann_parameters() unless use_bl_param_ is
    // off, then read_parameter_file(param_file_).  defaults_file stands for the tables built into the user's RNAlib (a ViennaRNA
    // parameter file; ViennaRNA is no part of the reference, so this library has none of its own); semantics: 0 = by the files
    // (a v2.0 file selects the 2.x loop energies of the HAVE_VIENNA20 build), 1 = ViennaRNA-1.8, 2 = ViennaRNA-2.x (include/
    // ractip_hot.h, rh_create_vienna).  Takes effect for the Vienna-model members; existing Vienna contexts are rebuilt.
    void set_vienna_parameters(const std::string& defaults_file, bool use_bl_param, const std::string& param_file, int semantics = 0);
    // arithmetic path of the pf_duplex sweeps alone (rh_set_duplex_mode: RH_MODE_INHERIT, AUTO, LOG, LINEAR), on every context of
    // this engine, those created later included.  With the 2.x loop energies, RH_MODE_AUTO moves the --duplex branch
    // (rnaduplex, solve_probabilities_default(..., duplex = true)) from the log-space kernels to the scaled linear ones
    void set_duplex_mode(int mode);

    rh_ctx* raw() const { return ctx_; }
    int device_count() const { return (int)devices_.size(); }
    // [lo, hi) of `num` units owned by shard `k` of `parts`: contiguous, sizes differ by at most one (ractip_amd/shard.py)
    static std::pair<int, int> shard_bounds(int num, int k, int parts);

private:
    [[noreturn]] void raise(const char* where) const;
    rh_ctx* vienna() const;
    std::vector<PairProbabilities> batch(rh_ctx* ctx, const std::vector<std::pair<std::string, std::string>>& pairs, uint max_w,
                                         bool threshold_hp, const std::vector<std::pair<std::string, std::string>>* structures = nullptr) const;
    std::vector<PairProbabilities> batch_one(rh_ctx* ctx, const std::vector<std::pair<std::string, std::string>>& pairs, int lo, int hi,
                                             uint max_w, bool threshold_hp,
                                             const std::vector<std::pair<std::string, std::string>>* structures = nullptr) const;
    std::vector<PairProbabilities> batch_indexed(rh_ctx* ctx, const std::vector<std::string>& seqs, const std::vector<std::pair<int, int>>& index_pairs,
                                                 uint max_w, bool threshold_hp) const;
    std::vector<PairProbabilities> compute_and_unpack(rh_ctx* ctx, int nseq, const std::vector<int>& first, const std::vector<int>& second,
                                                      const std::vector<int>& n1, const std::vector<int>& n2, uint max_w, bool threshold_hp) const;
    // page-locked float buffers of the batched members (rh_host_alloc), one set per context: bp, up, hp images of
    // rh_batch_results_packed_f32.  Grow-only; released before their context is destroyed.
    struct PackedBuffers {
        float* p[3] = {nullptr, nullptr, nullptr};
        size_t cap[3] = {0, 0, 0};   // floats
    };
    PackedBuffers& packed_buffers(rh_ctx* ctx, const size_t totals[3]) const;
    void release_buffers(rh_ctx* ctx) const;
    mutable std::map<rh_ctx*, PackedBuffers> packed_;
    mutable std::mutex packed_lock_;       // (the shards of one call look their sets up from their own threads)
    rh_ctx* ctx_;                          // first device's CONTRAfold context
    mutable rh_ctx* vctx_ = nullptr;       // first device's Vienna-BL context (created on first use)
    std::vector<int> devices_;
    std::vector<rh_ctx*> ctxs_;            // one CONTRAfold context per listed device (ctxs_[0] == ctx_)
    mutable std::vector<rh_ctx*> vctxs_;   // Vienna-BL contexts, same order
    int device_;
    float th_hy_;
    std::string v_defaults_, v_param_;     // set_vienna_parameters
    bool v_use_bl_ = true;
    int v_semantics_ = 0;
    int duplex_mode_ = -1;                 // RH_MODE_INHERIT
};

// The FASTA structure line of one sequence of L letters as RactIP::rnafold hands it to pf_fold (src/ractip.cpp:275-287): '[' ']' 'e'
// become 'x', everything else is kept, missing positions are '.'
std::string fold_constraint(const std::string& str, uint L);
// The structure lines of a pair as the default branch of RactIP::rnaduplex hands them to co_pf_fold over s1+s2 (:409-440): '[' of s1
// becomes '(' and ']' of s2 becomes ')', '(' ')' 'l' 'x' become 'x', everything else '.'
std::string joint_constraint(const std::string& str1, uint n1, const std::string& str2, uint n2);

// offset[i] = i*(2(L+1)-i-1)/2, size L+1  (src/ractip.cpp:254-257; InferenceEngine.ipp:316)
VI make_offsets(uint L);

}  // namespace ractip_amd
