// batch_request.h -- what an upload asks for, as a value, and the host-only checks of it (batch_request.cpp: no HIP, no context).
// Every path to the GPU -- the one-shot folds and pair calls, the four rh_batch_upload* entry points, the helper context of the
// per-pair fallback -- fills a BatchRequest and hands it to stage() (staging.hip), which begins with check_batch.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace rh::host {

struct BatchRequest {
    int ns = 0;                                // the distinct sequences ...
    const char* const* seqs = nullptr;         // ... [ns], lens[k] letters each
    const int* lens = nullptr;
    bool with_mc = false;                      // fold every sequence
    bool with_dx = false;                      // hybridize the pairs
    const char* const* fold_cons = nullptr;    // [ns] structure constraints of the single-molecule folds
    const char* const* joint_cons = nullptr;   // [ns / 2] per pair, over s1+s2 of the two-molecule ensemble: plain batches only
    int npairs = 0;                            // pair p = (first[p], second[p]); first == nullptr: the ns / 2 pairs (2p, 2p+1), a
    const int* first = nullptr;                // plain batch, whatever npairs says
    const int* second = nullptr;
    const char* const* share_first = nullptr;  // [ns] indexed batches only: pair p's joint constraint is share_first[first[p]]
    const char* const* share_second = nullptr; // over s1 + share_second[second[p]] over s2 (constraint_prepass.h)
    // Any constraint array, or any entry, may be nullptr; an array whose entries are all nullptr is no constraint.
};

// The per-letter values of `count` constraint strings (constraint_prepass.h), [count][lds] each, as allow_mask_build reads them
struct ConsPass {
    std::vector<uint8_t> ch;
    std::vector<int> P, enc;
    ConsPass(int count = 0, int lds = 0) : ch((size_t)count * lds, '.'), P((size_t)count * lds, 0), enc((size_t)count * lds, 0) {}
};

// The shares of the ns distinct sequences of an indexed batch in both roles (share_prepass; share role * ns + k), the open brackets
// of each, and why a share cannot stand in its role ("" = it can): O(letters of the distinct sequences), whatever the pairs.
struct SharePass {
    ConsPass L;
    std::vector<int> off, pos;
    std::vector<std::string> why;
    SharePass(int ns = 0, int lds = 0) : L(2 * ns, lds), off(1, 0), why(2 * (size_t)ns) {}
};

// What check_batch derives from an accepted request: everything stage() sizes and fills the tables from.
struct BatchShape {
    bool indexed = false;
    int np = 0;                          // pairs (0 without with_dx)
    int nmax = 0, n1max = 0, n2max = 0;  // longest sequence, longest s1, longest s2
    int cut_min = 0, cut_max = 0;        // shortest / longest s1
    int lds = 0, co_lds = 0;             // row pitch of the codes of a sequence / of a concatenation s1+s2
    std::vector<int> pair_seq;           // [2 np] pair p = sequences pair_seq[2p], pair_seq[2p+1]
    std::vector<uint8_t> codes;          // [ns][lds] letter codes of the model, sentinels around each sequence
    bool has_fold = false, has_joint = false, has_shares = false;   // which constraints apply, and their pre-passes:
    ConsPass fold, joint;                // [ns][lds], [np][co_lds]
    SharePass share;                     // [2 ns][lds]
};

// RH_ERR_UNSUPPORTED, with the reason in *why, for a request that carries a constraint (a non-null entry of any of its arrays) under
// another model than Vienna-BL; RH_OK otherwise.  Reads the constraint arrays only.
int check_model(const BatchRequest& r, bool vienna, std::string* why);

// Everything that can be said about a request without a device: lengths, NULLs, the even count of a plain batch, the index range;
// which constraint arrays apply; their pre-passes (per sequence, per joined pair, per share and pair); the shape.  Returns RH_OK
// with *shape filled, or the error code with the message in *why.  vienna: the model (letter codes, and whether constraints apply).
int check_batch(const BatchRequest& r, bool vienna, BatchShape* shape, std::string* why);

}  // namespace rh::host
