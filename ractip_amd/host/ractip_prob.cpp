// ractip_prob.cpp -- see ractip_prob.hpp.  Pure host code above the C ABI.
#include "ractip_prob.hpp"

#include <algorithm>
#include <thread>

#include "../../include/ractip_hot.h"

namespace ractip_amd {

VI make_offsets(uint L)
{
    VI off(L + 1);
    for (uint i = 0; i <= L; ++i) off[i] = (int)(i * ((L + 1) + (L + 1) - i - 1) / 2);
    return off;
}

ProbabilityEngine::ProbabilityEngine(int device, float th_hy, const char* param_file)
    : ProbabilityEngine(std::vector<int>(1, device), th_hy, param_file) {}

ProbabilityEngine::ProbabilityEngine(const std::vector<int>& devices, float th_hy, const char* param_file)
    : ctx_(nullptr), devices_(devices.empty() ? std::vector<int>(1, 0) : devices), device_(devices_[0]), th_hy_(th_hy)
{
    for (int d : devices_) {
        rh_ctx* c = rh_create(d, RH_MODEL_CONTRAFOLD, param_file);
        if (!c) {
            const std::string why = rh_last_error(nullptr);
            for (rh_ctx* k : ctxs_) rh_destroy(k);
            throw std::logic_error("ractip_amd: " + why);
        }
        ctxs_.push_back(c);
    }
    ctx_ = ctxs_[0];
    vctxs_.assign(devices_.size(), nullptr);
}

ProbabilityEngine::~ProbabilityEngine()
{
    for (rh_ctx* c : ctxs_) { release_buffers(c); rh_destroy(c); }
    for (rh_ctx* c : vctxs_) { release_buffers(c); rh_destroy(c); }
}

// this context's page-locked buffers, grown to hold `totals` floats of bp, up and hp
ProbabilityEngine::PackedBuffers& ProbabilityEngine::packed_buffers(rh_ctx* ctx, const size_t totals[3]) const
{
    PackedBuffers* b;
    {
        std::lock_guard<std::mutex> hold(packed_lock_);
        b = &packed_[ctx];   // (a map keeps its entries in place; a context is driven by one thread at a time)
    }
    for (int k = 0; k < 3; ++k) {
        if (totals[k] <= b->cap[k]) continue;
        if (b->p[k]) rh_host_free(ctx, b->p[k]);
        b->cap[k] = 0;
        b->p[k] = static_cast<float*>(rh_host_alloc(ctx, sizeof(float) * totals[k]));
        if (!b->p[k]) throw std::logic_error(std::string("ractip_amd::solve_probabilities: ") + rh_last_error(ctx));
        b->cap[k] = totals[k];
    }
    return *b;
}

void ProbabilityEngine::release_buffers(rh_ctx* ctx) const
{
    if (!ctx) return;
    std::lock_guard<std::mutex> hold(packed_lock_);
    const auto it = packed_.find(ctx);
    if (it == packed_.end()) return;
    for (float* p : it->second.p) if (p) rh_host_free(ctx, p);
    packed_.erase(it);
}

rh_ctx* ProbabilityEngine::vienna() const
{
    if (!vctx_) {
        for (size_t k = 0; k < devices_.size(); ++k) {
            if (!vctxs_[k])
                vctxs_[k] = rh_create_vienna(devices_[k], v_defaults_.empty() ? nullptr : v_defaults_.c_str(), v_use_bl_ ? 1 : 0,
                                             v_param_.empty() ? nullptr : v_param_.c_str(), v_semantics_);
            if (!vctxs_[k]) throw std::logic_error(std::string("ractip_amd: ") + rh_last_error(nullptr));
            rh_set_duplex_mode(vctxs_[k], duplex_mode_);
        }
        vctx_ = vctxs_[0];
    }
    return vctx_;
}

void ProbabilityEngine::set_vienna_parameters(const std::string& defaults_file, bool use_bl_param, const std::string& param_file, int semantics)
{
    v_defaults_ = defaults_file; v_use_bl_ = use_bl_param; v_param_ = param_file; v_semantics_ = semantics;
    for (rh_ctx*& c : vctxs_) { if (c) { release_buffers(c); rh_destroy(c); } c = nullptr; }
    vctx_ = nullptr;
}

void ProbabilityEngine::set_duplex_mode(int mode)
{
    if (mode < RH_MODE_INHERIT || mode > RH_MODE_LINEAR) throw std::logic_error("ractip_amd::set_duplex_mode: unknown mode");
    duplex_mode_ = mode;
    for (rh_ctx* c : ctxs_) rh_set_duplex_mode(c, mode);
    for (rh_ctx* c : vctxs_) if (c) rh_set_duplex_mode(c, mode);
}

std::pair<int, int> ProbabilityEngine::shard_bounds(int num, int k, int parts)
{
    const int base = num / parts, extra = num % parts;
    const int lo = k * base + std::min(k, extra);
    return {lo, lo + base + (k < extra ? 1 : 0)};
}

void ProbabilityEngine::raise(const char* where) const
{
    throw std::logic_error(std::string("ractip_amd::") + where + ": " + rh_last_error(ctx_));
}

std::string fold_constraint(const std::string& str, uint L)
{
    std::string c(L, '.');   // src/ractip.cpp:275-287
    for (uint i = 0; i != str.size() && i != L; ++i) c[i] = (str[i] == '[' || str[i] == ']' || str[i] == 'e') ? 'x' : str[i];
    return c;
}

std::string joint_constraint(const std::string& str1, uint n1, const std::string& str2, uint n2)
{
    std::string c(n1 + n2, '.');   // src/ractip.cpp:409-440
    for (uint i = 0; i != str1.size() && i != n1; ++i)
        switch (str1[i]) {
            case '[': c[i] = '('; break;
            case '(': case ')': case 'l': case 'x': c[i] = 'x'; break;
            default: break;
        }
    for (uint i = 0; i != str2.size() && i != n2; ++i)
        switch (str2[i]) {
            case ']': c[n1 + i] = ')'; break;
            case '(': case ')': case 'l': case 'x': c[n1 + i] = 'x'; break;
            default: break;
        }
    return c;
}

namespace {
// narrow to float exactly where the reference does (VF containers, src/ractip.cpp:82-83)
void narrow_bp(const std::vector<double>& d, VF& bp)
{
    bp.resize(d.size());
    std::transform(d.begin(), d.end(), bp.begin(), [](double v) { return (float)v; });
}
void narrow_up(const std::vector<double>& d, VVF& up)
{
    up.assign(d.size(), VF(1));
    for (size_t i = 0; i < d.size(); ++i) up[i][0] = (float)d[i];
}
}  // namespace

void ProbabilityEngine::contrafold(const std::string& seq, VF& bp, VI& offset, VVF& up) const
{
    const uint L = seq.size();
    std::vector<double> dbp((size_t)(L + 1) * (L + 2) / 2, 0.0), dup(L, 1.0);
    offset = make_offsets(L);
    if (L > 0 && rh_fold(ctx_, seq.c_str(), (int)L, dbp.data(), dup.data(), nullptr) != RH_OK) raise("contrafold");
    narrow_bp(dbp, bp);
    narrow_up(dup, up);
}

void ProbabilityEngine::contrafold(const std::string& seq, VF& bp, VI& offset, VVF& up, uint max_w) const
{
    const uint L = seq.size();
    if (max_w < 1) max_w = 1;
    std::vector<double> dbp((size_t)(L + 1) * (L + 2) / 2, 0.0), dup((size_t)L * max_w, 0.0);
    offset = make_offsets(L);
    if (L > 0) {
        const bool ok = rh_set_region_accessibility(ctx_, 1) == RH_OK && rh_set_max_w(ctx_, (int)max_w) == RH_OK &&
                        rh_fold(ctx_, seq.c_str(), (int)L, dbp.data(), dup.data(), nullptr) == RH_OK;
        const std::string why = ok ? "" : rh_last_error(ctx_);
        rh_set_region_accessibility(ctx_, 0);   // (max_w goes back to 1 with it)
        if (!ok) throw std::logic_error("ractip_amd::contrafold: " + why);
    }
    narrow_bp(dbp, bp);
    up.assign(L, VF(max_w));
    for (uint i = 0; i < L; ++i)
        for (uint w = 0; w < max_w; ++w) up[i][w] = (float)dup[(size_t)i * max_w + w];
}

void ProbabilityEngine::rnafold(const std::string& seq, VF& bp, VI& offset) const
{
    const uint L = seq.size();
    std::vector<double> dbp((size_t)(L + 1) * (L + 2) / 2, 0.0);
    offset = make_offsets(L);
    rh_ctx* v = vienna();
    if (L > 0 && rh_bpp(v, seq.c_str(), (int)L, nullptr, dbp.data(), nullptr) != RH_OK)
        throw std::logic_error(std::string("ractip_amd::rnafold: ") + rh_last_error(v));
    narrow_bp(dbp, bp);
}

void ProbabilityEngine::rnafold(const std::string& seq, VF& bp, VI& offset, VVF& up, uint max_w) const
{
    const uint L = seq.size();
    std::vector<double> dbp((size_t)(L + 1) * (L + 2) / 2, 0.0), dup((size_t)L * max_w, 0.0);
    offset = make_offsets(L);
    rh_ctx* v = vienna();
    if (L > 0 && (rh_set_max_w(v, (int)max_w) != RH_OK || rh_fold(v, seq.c_str(), (int)L, dbp.data(), dup.data(), nullptr) != RH_OK))
        throw std::logic_error(std::string("ractip_amd::rnafold: ") + rh_last_error(v));
    narrow_bp(dbp, bp);
    up.assign(L, VF(max_w));   // up.resize(L, VF(max_w)), :370
    for (uint i = 0; i < L; ++i)
        for (uint w = 0; w < max_w; ++w) up[i][w] = (float)dup[(size_t)i * max_w + w];
}

void ProbabilityEngine::rnafold(const std::string& seq, const std::string& str, VF& bp, VI& offset, VVF& up, uint max_w) const
{
    const uint L = seq.size();
    const std::string c = fold_constraint(str, L);
    std::vector<double> dbp((size_t)(L + 1) * (L + 2) / 2, 0.0), dup((size_t)L * max_w, 0.0);
    offset = make_offsets(L);
    rh_ctx* v = vienna();
    if (L > 0 && (rh_set_max_w(v, (int)max_w) != RH_OK ||
                  rh_fold_constrained(v, seq.c_str(), (int)L, c.c_str(), dbp.data(), dup.data(), nullptr) != RH_OK))
        throw std::logic_error(std::string("ractip_amd::rnafold: ") + rh_last_error(v));
    narrow_bp(dbp, bp);
    up.assign(L, VF(max_w));
    for (uint i = 0; i < L; ++i)
        for (uint w = 0; w < max_w; ++w) up[i][w] = (float)dup[(size_t)i * max_w + w];
}

void ProbabilityEngine::rnaduplex_cofold(const std::string& seq1, const std::string& seq2, VVF& hp) const
{
    const uint n1 = seq1.size(), n2 = seq2.size();
    hp.assign(n1 + 1, VF(n2 + 1, 0.0f));   // hp.resize(s1.size()+1, VF(s2.size()+1, 0.0)), :403-404
    if (n1 == 0 || n2 == 0) return;
    rh_ctx* v = vienna();
    std::vector<double> d((size_t)(n1 + 1) * (n2 + 1));
    bool ok = rh_set_hybrid(v, RH_HYBRID_COFOLD) == RH_OK &&
              rh_duplex(v, seq1.c_str(), (int)n1, seq2.c_str(), (int)n2, d.data(), nullptr) == RH_OK;
    const std::string why = ok ? "" : rh_last_error(v);
    rh_set_hybrid(v, RH_HYBRID_DUPLEX);
    if (!ok) throw std::logic_error("ractip_amd::rnaduplex: " + why);
    for (uint i = 1; i <= n1; ++i)
        for (uint j = 1; j <= n2; ++j) {
            const float p = (float)d[(size_t)i * (n2 + 1) + j];   // pair_info::p is a float
            if (p > th_hy_) hp[i][j] = p;                          // :451-454
        }
}

void ProbabilityEngine::rnaduplex_cofold(const std::string& seq1, const std::string& str1, const std::string& seq2,
                                         const std::string& str2, VVF& hp) const
{
    const uint n1 = seq1.size(), n2 = seq2.size();
    hp.assign(n1 + 1, VF(n2 + 1, 0.0f));
    if (n1 == 0 || n2 == 0) return;
    const std::string c = joint_constraint(str1, n1, str2, n2);
    rh_ctx* v = vienna();
    std::vector<double> d((size_t)(n1 + 1) * (n2 + 1));
    if (rh_cofold_constrained(v, seq1.c_str(), (int)n1, seq2.c_str(), (int)n2, c.c_str(), d.data(), nullptr) != RH_OK)
        throw std::logic_error(std::string("ractip_amd::rnaduplex: ") + rh_last_error(v));
    for (uint i = 1; i <= n1; ++i)
        for (uint j = 1; j <= n2; ++j) {
            const float p = (float)d[(size_t)i * (n2 + 1) + j];
            if (p > th_hy_) hp[i][j] = p;
        }
}

void ProbabilityEngine::contraduplex(const std::string& seq1, const std::string& seq2, VVF& hp) const
{
    const uint n1 = seq1.size(), n2 = seq2.size();
    hp.assign(n1 + 1, VF(n2 + 1, 0.0f));
    if (n1 == 0 || n2 == 0) return;
    std::vector<double> d((size_t)(n1 + 1) * (n2 + 1));
    if (rh_duplex(ctx_, seq1.c_str(), (int)n1, seq2.c_str(), (int)n2, d.data(), nullptr) != RH_OK) raise("contraduplex");
    for (uint i = 1; i <= n1; ++i)
        for (uint j = 1; j <= n2; ++j) {
            const float p = (float)d[(size_t)i * (n2 + 1) + j];
            hp[i][j] = p >= th_hy_ ? p : 0.0f;  // GetPosterior(th_hy_, ip), DuplexEngine.ipp:1189-1196
        }
}

void ProbabilityEngine::rnaduplex(const std::string& seq1, const std::string& seq2, VVF& hp) const
{
    // the --duplex branch (src/ractip.cpp:390-398): pf_duplex() with the BL* energies, i.e. the Vienna-BL context with hp from
    // the duplex-only ensemble -- the same numbers the pf_duplex shim and solve_probabilities_default(duplex = true) return
    const uint n1 = seq1.size(), n2 = seq2.size();
    hp.assign(n1 + 1, VF(n2 + 1, 0.0f));  // hp.resize(s1.size()+1, VF(s2.size()+1)), :393
    if (n1 == 0 || n2 == 0) return;
    rh_ctx* v = vienna();
    std::vector<double> d((size_t)(n1 + 1) * (n2 + 1));
    if (rh_set_hybrid(v, RH_HYBRID_DUPLEX) != RH_OK || rh_duplex(v, seq1.c_str(), (int)n1, seq2.c_str(), (int)n2, d.data(), nullptr) != RH_OK)
        throw std::logic_error(std::string("ractip_amd::rnaduplex: ") + rh_last_error(v));
    for (uint i = 1; i <= n1; ++i)
        for (uint j = 1; j <= n2; ++j) hp[i][j] = (float)d[(size_t)i * (n2 + 1) + j];  // :395-397, no threshold
}

std::vector<PairProbabilities> ProbabilityEngine::solve_probabilities(
    const std::vector<std::pair<std::string, std::string>>& pairs) const
{
    return batch(ctx_, pairs, 1, false);
}

std::vector<PairProbabilities> ProbabilityEngine::solve_probabilities_default(
    const std::vector<std::pair<std::string, std::string>>& pairs, uint max_w, bool duplex) const
{
    vienna();
    for (rh_ctx* v : vctxs_)
        if (rh_set_max_w(v, (int)std::max(1u, max_w)) != RH_OK || rh_set_hybrid(v, duplex ? RH_HYBRID_DUPLEX : RH_HYBRID_COFOLD) != RH_OK)
            throw std::logic_error(std::string("ractip_amd::solve_probabilities_default: ") + rh_last_error(v));
    std::vector<PairProbabilities> out = batch(vctx_, pairs, std::max(1u, max_w), !duplex);
    for (rh_ctx* v : vctxs_) rh_set_hybrid(v, RH_HYBRID_DUPLEX);
    return out;
}

std::vector<PairProbabilities> ProbabilityEngine::solve_probabilities_default(
    const std::vector<std::pair<std::string, std::string>>& pairs, const std::vector<std::pair<std::string, std::string>>& structures,
    uint max_w, bool duplex) const
{
    if (structures.size() != pairs.size()) throw std::logic_error("ractip_amd::solve_probabilities_default: one (str1, str2) per pair");
    vienna();
    for (rh_ctx* v : vctxs_)
        if (rh_set_max_w(v, (int)std::max(1u, max_w)) != RH_OK || rh_set_hybrid(v, duplex ? RH_HYBRID_DUPLEX : RH_HYBRID_COFOLD) != RH_OK)
            throw std::logic_error(std::string("ractip_amd::solve_probabilities_default: ") + rh_last_error(v));
    std::vector<PairProbabilities> out;
    std::string error;
    try { out = batch(vctx_, pairs, std::max(1u, max_w), !duplex, &structures); } catch (const std::logic_error& e) { error = e.what(); }
    for (rh_ctx* v : vctxs_) rh_set_hybrid(v, RH_HYBRID_DUPLEX);
    if (!error.empty()) throw std::logic_error(error);
    return out;
}

std::vector<PairProbabilities> ProbabilityEngine::solve_probabilities_indexed(const std::vector<std::string>& seqs,
                                                                              const std::vector<std::pair<int, int>>& index_pairs) const
{
    return batch_indexed(ctx_, seqs, index_pairs, 1, false);
}

std::vector<PairProbabilities> ProbabilityEngine::solve_probabilities_default_indexed(const std::vector<std::string>& seqs,
                                                                                      const std::vector<std::pair<int, int>>& index_pairs,
                                                                                      uint max_w, bool duplex) const
{
    vienna();
    for (rh_ctx* v : vctxs_)
        if (rh_set_max_w(v, (int)std::max(1u, max_w)) != RH_OK || rh_set_hybrid(v, duplex ? RH_HYBRID_DUPLEX : RH_HYBRID_COFOLD) != RH_OK)
            throw std::logic_error(std::string("ractip_amd::solve_probabilities_default_indexed: ") + rh_last_error(v));
    std::vector<PairProbabilities> out;
    std::string error;
    try { out = batch_indexed(vctx_, seqs, index_pairs, std::max(1u, max_w), !duplex); } catch (const std::logic_error& e) { error = e.what(); }
    for (rh_ctx* v : vctxs_) rh_set_hybrid(v, RH_HYBRID_DUPLEX);
    if (!error.empty()) throw std::logic_error(error);
    return out;
}

// The indexed counterpart of batch(): the same contiguous blocks of the pairs, one per listed device; each shard uploads only the
// sequences its block references, re-indexed in the order of their first appearance in the block
std::vector<PairProbabilities> ProbabilityEngine::batch_indexed(rh_ctx* ctx, const std::vector<std::string>& seqs,
                                                                const std::vector<std::pair<int, int>>& index_pairs, uint max_w,
                                                                bool threshold_hp) const
{
    const int np = (int)index_pairs.size(), ns = (int)seqs.size();
    for (const std::pair<int, int>& ip : index_pairs)
        if (ip.first < 0 || ip.first >= ns || ip.second < 0 || ip.second >= ns)
            throw std::logic_error("ractip_amd::solve_probabilities_indexed: index outside the sequences");
    if (np == 0) return {};
    const std::vector<rh_ctx*>& all = (ctx == ctx_) ? ctxs_ : vctxs_;
    const int parts = std::min<int>((int)all.size(), np);
    const auto one = [&](rh_ctx* c, int lo, int hi) {
        std::vector<int> slot(ns, -1), first(hi - lo), second(hi - lo), lens, na(hi - lo), nb(hi - lo);
        std::vector<const char*> ptr;
        const auto use = [&](int k) {
            if (slot[k] < 0) { slot[k] = (int)ptr.size(); ptr.push_back(seqs[k].c_str()); lens.push_back((int)seqs[k].size()); }
            return slot[k];
        };
        for (int p = lo; p < hi; ++p) {
            first[p - lo] = use(index_pairs[p].first); second[p - lo] = use(index_pairs[p].second);
            na[p - lo] = (int)seqs[index_pairs[p].first].size(); nb[p - lo] = (int)seqs[index_pairs[p].second].size();
        }
        if (rh_batch_upload_indexed(c, (int)ptr.size(), ptr.data(), lens.data(), hi - lo, first.data(), second.data()) != RH_OK)
            throw std::logic_error(std::string("ractip_amd::solve_probabilities_indexed: ") + rh_last_error(c));
        return compute_and_unpack(c, (int)ptr.size(), first, second, na, nb, max_w, threshold_hp);
    };
    if (parts <= 1) return one(ctx, 0, np);
    std::vector<std::vector<PairProbabilities>> part(parts);
    std::vector<std::string> errors(parts);
    std::vector<std::thread> workers;
    for (int k = 0; k < parts; ++k)
        workers.emplace_back([&, k] {
            try {
                const auto b = shard_bounds(np, k, parts);
                part[k] = one(all[k], b.first, b.second);
            } catch (const std::exception& e) { errors[k] = e.what(); }
        });
    for (std::thread& t : workers) t.join();
    std::vector<PairProbabilities> out;
    out.reserve(np);
    for (int k = 0; k < parts; ++k) {
        if (!errors[k].empty()) throw std::logic_error(errors[k]);
        for (PairProbabilities& r : part[k]) out.push_back(std::move(r));
    }
    return out;
}

// contiguous blocks of the pairs, one per listed device, each on its own context and host thread; results in iteration order
std::vector<PairProbabilities> ProbabilityEngine::batch(rh_ctx* ctx, const std::vector<std::pair<std::string, std::string>>& pairs,
                                                        uint max_w, bool threshold_hp,
                                                        const std::vector<std::pair<std::string, std::string>>* structures) const
{
    const int np = (int)pairs.size();
    const std::vector<rh_ctx*>& all = (ctx == ctx_) ? ctxs_ : vctxs_;
    const int parts = std::min<int>((int)all.size(), std::max(1, np));
    if (parts <= 1) return batch_one(ctx, pairs, 0, np, max_w, threshold_hp, structures);
    std::vector<std::vector<PairProbabilities>> part(parts);
    std::vector<std::string> errors(parts);
    std::vector<std::thread> workers;
    for (int k = 0; k < parts; ++k)
        workers.emplace_back([&, k] {
            try {
                const auto b = shard_bounds(np, k, parts);
                part[k] = batch_one(all[k], pairs, b.first, b.second, max_w, threshold_hp, structures);
            } catch (const std::exception& e) { errors[k] = e.what(); }
        });
    for (std::thread& t : workers) t.join();
    std::vector<PairProbabilities> out;
    out.reserve(np);
    for (int k = 0; k < parts; ++k) {
        if (!errors[k].empty()) throw std::logic_error(errors[k]);
        for (PairProbabilities& r : part[k]) out.push_back(std::move(r));
    }
    return out;
}

std::vector<PairProbabilities> ProbabilityEngine::batch_one(rh_ctx* ctx, const std::vector<std::pair<std::string, std::string>>& all_pairs,
                                                            int lo, int hi, uint max_w, bool threshold_hp,
                                                            const std::vector<std::pair<std::string, std::string>>* structures) const
{
    const std::vector<std::pair<std::string, std::string>> pairs(all_pairs.begin() + lo, all_pairs.begin() + hi);
    const int np = (int)pairs.size();
    if (np == 0) return {};
    std::vector<const char*> a(np), b(np);
    std::vector<int> na(np), nb(np);
    for (int p = 0; p < np; ++p) {
        a[p] = pairs[p].first.c_str(); b[p] = pairs[p].second.c_str();
        na[p] = (int)pairs[p].first.size(); nb[p] = (int)pairs[p].second.size();
    }
    auto raise_ctx = [&](const char* where) { throw std::logic_error(std::string("ractip_amd::") + where + ": " + rh_last_error(ctx)); };
    if (structures) {   // this shard's structure lines, translated as the single-problem members translate them
        std::vector<std::string> c1(np), c2(np), cj(np);
        std::vector<const char*> p1(np), p2(np), pj(np);
        for (int p = 0; p < np; ++p) {
            const std::pair<std::string, std::string>& st = (*structures)[lo + p];
            c1[p] = fold_constraint(st.first, na[p]); c2[p] = fold_constraint(st.second, nb[p]);
            cj[p] = joint_constraint(st.first, na[p], st.second, nb[p]);
            p1[p] = c1[p].c_str(); p2[p] = c2[p].c_str(); pj[p] = cj[p].c_str();
        }
        if (rh_batch_upload_constrained(ctx, np, a.data(), na.data(), b.data(), nb.data(), p1.data(), p2.data(), pj.data()) != RH_OK)
            raise_ctx("solve_probabilities");
    } else if (rh_batch_upload(ctx, np, a.data(), na.data(), b.data(), nb.data()) != RH_OK) raise_ctx("solve_probabilities");
    std::vector<int> first(np), second(np);
    for (int p = 0; p < np; ++p) { first[p] = 2 * p; second[p] = 2 * p + 1; }
    return compute_and_unpack(ctx, 2 * np, first, second, na, nb, max_w, threshold_hp);
}

// the staged batch computed and unpacked: pair p = sequences first[p], second[p] of the nseq fold rows, of n1[p] and n2[p] letters
std::vector<PairProbabilities> ProbabilityEngine::compute_and_unpack(rh_ctx* ctx, int nseq, const std::vector<int>& first, const std::vector<int>& second,
                                                                     const std::vector<int>& na, const std::vector<int>& nb, uint max_w,
                                                                     bool threshold_hp) const
{
    const int np = (int)first.size();
    std::vector<PairProbabilities> out(np);
    auto raise_ctx = [&](const char* where) { throw std::logic_error(std::string("ractip_amd::") + where + ": " + rh_last_error(ctx)); };
    if (rh_batch_compute(ctx) != RH_OK) raise_ctx("solve_probabilities");
    // the whole batch at the width the containers store (VF / VVF are float): narrowed and packed on the device, three copies into this
    // context's page-locked buffers, then block copies into the members
    std::vector<size_t> bp_off((size_t)nseq + 1), up_off((size_t)nseq + 1), hp_off((size_t)np + 1);
    size_t totals[3];
    if (rh_batch_packed_layout(ctx, bp_off.data(), up_off.data(), hp_off.data(), totals) != RH_OK) raise_ctx("solve_probabilities");
    const PackedBuffers& buf = packed_buffers(ctx, totals);
    std::vector<double> z((size_t)3 * np);
    if (rh_batch_results_packed_f32(ctx, buf.p[0], buf.p[1], buf.p[2], z.data()) != RH_OK) raise_ctx("solve_probabilities");
    const auto rows = [max_w](const float* u, uint n, VVF& up) {
        up.resize(n);
        for (uint i = 0; i < n; ++i) up[i].assign(u + (size_t)i * max_w, u + (size_t)(i + 1) * max_w);
    };
    for (int p = 0; p < np; ++p) {
        const uint n1 = na[p], n2 = nb[p];
        PairProbabilities& r = out[p];
        const float* b1 = buf.p[0] + bp_off[first[p]];
        const float* b2 = buf.p[0] + bp_off[second[p]];
        r.bp1.assign(b1, b1 + (size_t)(n1 + 1) * (n1 + 2) / 2);
        r.bp2.assign(b2, b2 + (size_t)(n2 + 1) * (n2 + 2) / 2);
        rows(buf.p[1] + up_off[first[p]], n1, r.up1);
        rows(buf.p[1] + up_off[second[p]], n2, r.up2);
        r.offset1 = make_offsets(n1); r.offset2 = make_offsets(n2);
        const float* h = buf.p[2] + hp_off[p];
        r.hp.resize(n1 + 1);
        for (uint i = 0; i <= n1; ++i) {
            VF& row = r.hp[i];
            row.assign(h + (size_t)i * (n2 + 1), h + (size_t)(i + 1) * (n2 + 1));
            if (threshold_hp)
                for (float& v : row) if (!(v > th_hy_)) v = 0.0f;   // plist entries with p > th_hy (:451-454)
        }
        r.logZ1 = z[3 * p]; r.logZ2 = z[3 * p + 1]; r.logZd = z[3 * p + 2];
    }
    return out;
}

}  // namespace ractip_amd
