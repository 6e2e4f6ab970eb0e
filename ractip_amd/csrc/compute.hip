// compute.hip -- one batch from staged to computed: hipGraph capture / replay of the launch sequences, the two streams
// and their events, and the decision which fallback a flagged problem takes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "kernels.h"

namespace rh::host {

// ---- hipGraph replay of the fast path.  A launch sequence depends only on its argument(s) (ctx.h), so it is captured once per
// value of them and replayed: the ~1000 launches per sweep then cost the GPU-side ~1.5 us boundary instead of a host launch each.
// The key of slot g is a hash of the arguments' bytes; k: the n_launch / n_far entry that counts the sequence.
template <class L, class... Args>
int run_graphed(rh_ctx* c, GraphSlot& g, hipStream_t stream, int k, L launcher, const Args&... args)
{
    const auto launch = [&] { int rc = RH_OK; ((rc = rc ? rc : launcher(c, args)), ...); return rc; };
    if (!c->use_graphs || c->time_cls >= 0) return launch();   // (timed launches are host launches: events between graph nodes would be captured)
    size_t key = 1469598103934665603ull + (sizeof(Args) + ...);
    const auto mix = [&](const void* p, size_t n) { for (size_t q = 0; q < n; q++) key = (key ^ ((const unsigned char*)p)[q]) * 0x100000001b3ull; };
    (mix(&args, sizeof(Args)), ...);
    int *launch_counter = &c->n_launch[k], *far_counter = &c->n_far[k];
    if (!g.exec || g.key != key) {
        if (g.exec) { HIP_TRY(c, hipGraphExecDestroy(g.exec)); g.exec = nullptr; }
        hipGraph_t graph = nullptr;
        const int before = *launch_counter, far_before = *far_counter;
        HIP_TRY(c, hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        const int rc = launch();
        hipError_t e = hipStreamEndCapture(stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }   // (the captured graph is not leaked on the error paths)
        if (e != hipSuccess) { if (graph) (void)hipGraphDestroy(graph); return fail(c, RH_ERR_HIP, "graph capture failed: %s", hipGetErrorString(e)); }
        e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { g.exec = nullptr; return fail(c, RH_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e)); }
        g.key = key;
        g.launches = *launch_counter - before;
        g.far = *far_counter - far_before;
        *launch_counter = before;
        *far_counter = far_before;
    }
    HIP_TRY(c, hipGraphLaunch(g.exec, stream));
    *launch_counter += g.launches;
    *far_counter += g.far;
    return RH_OK;
}

// ---- the arguments of the launchers, from the context
// One phase over the sequences B on the model `lin`.  routed: B is the batch as uploaded, whose short and small sequences have passes
// of their own (stage() has written their lists and length arrays).
McLinArgs mc_lin_args(const rh_ctx* c, int phase, const McBatch& B, const LinSet* lin, bool routed)
{
    McLinArgs A;
    A.B = B; A.lin = lin; A.phase = phase;
    A.logz = c->d_mclogz.as<double>(); A.bad = c->d_bad.as<int>();
    A.plan = plan_mc_lin(c, phase, B.nmax);
    if (routed && (!c->small_list.empty() || c->n_short > 0)) {
        A.routed = 1;
        A.small_list = c->d_small_list.as<const int>(); A.n_small = (int)c->small_list.size();
        A.n_sweep = c->d_n_sweep.as<const int>(); A.nmax_sweep = c->nmax_sweep;
        A.n_short = c->d_n_short.as<const int>(); A.nmax_short = c->nmax_short; A.short_count = c->n_short;
        A.plan_sweep = plan_mc_lin(c, phase, A.nmax_sweep);
        A.plan_short = plan_mc_lin(c, phase, A.nmax_short);
    }
    A.pin = B.ns % 8 == 0 ? 1 : 0;   // sequence -> XCD affinity only when the batch spreads evenly over the 8 XCDs (speed only)
    A.strip_xcd = c->strip_xcd;
    return A;
}

// One phase over the staged single-molecule batch or (co) the s1+s2 batch, on the model select_vlin selected last
static McVlinArgs mc_vlin_args(const rh_ctx* c, int phase, bool co)
{
    McVlinArgs A;
    A.B = co ? c->co : c->mc; A.phase = phase; A.co = co;
    A.pin = A.B.ns % 8 == 0 ? 1 : 0;
    A.plan = plan_mc_vlin(c, phase, co, A.B.nmax);
    A.d_vlin = c->d_vlin; A.h_vlin = c->h_vlin; A.hplen = c->h_hplen.data(); A.d_hplen = c->d_hplen.as<const double>();
    A.bad = co ? c->d_cobad.as<int>() : c->d_bad.as<int>();
    if (co) {
        const DxBatch& D = c->dx;
        if (A.B.seeded) A.from = c->mc;
        A.hp = D.hp; A.hp_logz = D.logz; A.hp_stride = D.tab_stride; A.hp_ldd = D.ldd; A.n1max = D.n1max; A.n2max = D.n2max;
        A.cut_min = c->co_cut_min; A.cut_max = c->co_cut_max;
        A.window = c->co_window && c->co_cut_min >= 1 && (phase == 1 || A.B.seeded);   // (an unseeded inside sweep computes every group)
    } else {
        A.logz = c->d_mclogz.as<double>(); A.gaps = c->d_gaps.as<double>(); A.max_w = c->max_w;
        // (vlin_acc_gaps_wide addresses a sequence's tables with 32-bit offsets; vlin_acc_final_t has up to fifteen widths)
        A.acc_wide = c->acc_wide && (size_t)kViennaMcTables * A.B.tab_stride * sizeof(double) < ((size_t)1 << 32);
        A.acc_final_t = c->acc_final_t && c->max_w <= 15;
    }
    return A;
}

// The hybridization sweeps over the staged batch of pairs, either model
DxLinArgs dx_lin_args(const rh_ctx* c)
{
    DxLinArgs A;
    A.X = c->dxl; A.plan = c->plan[2]; A.lz_chunks = c->lz_chunks;
    if (c->model == RH_MODEL_VIENNA_BL) { A.vdx_s = c->vdx_s; A.sem20 = c->vienna_sem == kViennaSem20; }
    else { A.dm = c->d_dxlin; A.hm = &c->h_dxlin; }
    A.zpart = c->d_zpart.as<double>(); A.zbar = c->d_zbar.as<double>();
    A.logz = c->d_logz.as<double>(); A.bad = c->d_dxbad.as<int>();
    return A;
}

// the indices of the set ones among the n flags at d_flags, read behind everything `st` holds
int flagged(rh_ctx* c, const int* d_flags, int n, hipStream_t st, std::vector<int>* set)
{
    std::vector<int> flags(n);
    HIP_TRY(c, hipMemcpyAsync(flags.data(), d_flags, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    set->clear();
    for (int k = 0; k < n; k++) if (flags[k]) set->push_back(k);
    return RH_OK;
}

int compute_once(rh_ctx* c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    c->deferred = false;
    c->went_log = false;
    c->tev_n = 0;
    c->n_launch[0] = c->n_launch[1] = c->n_launch[2] = 0;
    c->n_far[0] = c->n_far[1] = c->n_far[2] = 0;
    c->last_path = 0;
    c->fallback_mc.clear(); c->fallback_dx.clear(); c->rescaled_mc.clear(); c->rescaled_dx.clear();
    // the organisation of each sweep's linear first pass: decided here, on every compute (a replayed graph does not call its launcher);
    // the arguments below carry the same plans to the launchers
    const bool vienna = c->model == RH_MODEL_VIENNA_BL;
    for (int phase = 0; phase < 2; phase++) c->plan[phase] = vienna ? plan_mc_vlin(c, phase, false, c->mc.nmax) : plan_mc_lin(c, phase, c->mc.nmax);
    c->plan[2] = !vienna ? plan_dx_lin(c, c->dx_w) : c->hybrid == RH_HYBRID_COFOLD ? plan_mc_vlin(c, 0, true, c->co.nmax) : plan_dx_vlin(c->vienna_sem == kViennaSem20);
    const int pin = (c->has_mc && c->mc.ns % 8 == 0) ? 1 : 0;   // (of the log-space sweeps; the linear ones: see their arguments)
    // the path of the pf_duplex sweeps (RH_HYBRID_DUPLEX): rh_set_duplex_mode, or what rh_set_mode says
    const int dx_mode = c->duplex_mode == RH_MODE_INHERIT ? c->mode : c->duplex_mode;
    int rc;
    std::vector<int> bad;
    // the linear duplex kernels share d_dxtab with the log-space ones and read zero pad columns: after a log-space compute on this
    // upload (another mode since, or a fallback) the image stage() left is gone
    if (c->has_dx && c->dxtab_log && dx_mode != RH_MODE_LOG && !(c->model == RH_MODEL_VIENNA_BL && c->hybrid == RH_HYBRID_COFOLD)) {
        HIP_TRY(c, hipMemsetAsync(c->d_dxtab.p, 0, c->dx_bytes, c->s_dx));
        c->dxtab_log = false;
    }
    // duplex first on its own stream: it is independent of the McCaskill sweeps and overlaps them
    HIP_TRY(c, hipEventRecord(c->ev[3], c->s_dx));
    bool dx_lin_launched = false, co_lin_launched = false, co_seed_bad = false, out_from_ev5 = false;
    // two-molecule sweeps in linear space next to the single-molecule folds of the same pairs (no structure constraints): the cells
    // on one strand are copied from those folds (vlin_co_seed), so the sweeps over s1+s2 start when their inside tables are final
    const bool co_seed = c->has_dx && c->has_mc && c->model == RH_MODEL_VIENNA_BL && c->hybrid == RH_HYBRID_COFOLD && c->mode != RH_MODE_LOG &&
                         c->co_seed && !c->mc.allow && !c->co.allow && c->mc.ns == 2 * c->co.ns;
    c->co.seeded = co_seed ? 1 : 0;
    auto launch_co_lin = [&]() -> int {   // scaled linear sweeps over s1+s2; out-of-range values send the batch to the log-space kernels
        return run_graphed(c, c->g_dx, c->s_dx, 2, launch_mc_vlin, mc_vlin_args(c, 0, true), mc_vlin_args(c, 1, true));   // (one graph of both)
    };
    if (c->has_dx && c->model == RH_MODEL_VIENNA_BL && c->hybrid == RH_HYBRID_COFOLD) {
        HIP_TRY(c, hipMemsetAsync(c->d_cobp.p, 0, sizeof(double) * c->co.tri_stride * c->co.ns, c->s_dx));
        bool co_log = c->mode == RH_MODE_LOG;
        if (!co_log && !co_seed) {
            if ((rc = launch_co_lin())) return rc;
            c->last_dx_path = 1;
            co_lin_launched = true;   // its overflow flags are read after the McCaskill stream has been fed (the two overlap)
        }
        if (co_log) {
            if ((rc = launch_cofold(c))) return rc;
            if (c->last_dx_path != 3) c->last_dx_path = 2;
        }
    } else if (c->has_dx && c->model == RH_MODEL_VIENNA_BL) {
        if (dx_mode != RH_MODE_LOG) {   // scaled linear sweeps; pairs outside the double range send the batch to the log-space kernels
            if ((rc = run_graphed(c, c->g_dx, c->s_dx, 2, launch_dx_vlin, dx_lin_args(c)))) return rc;
            dx_lin_launched = true;
        } else {
            if ((rc = launch_dx_vlog(c))) return rc;
            c->dxtab_log = true;
            c->last_dx_path = 2;
        }
    } else if (c->has_dx) {
        if (dx_mode != RH_MODE_LOG) {
            if ((rc = run_graphed(c, c->g_dx, c->s_dx, 2, launch_dx_lin, dx_lin_args(c)))) return rc;
            dx_lin_launched = true;
        } else {
            if ((rc = launch_dx_log(c, c->dx))) return rc;
            c->dxtab_log = true;
            c->last_dx_path = 2;
        }
    }
    HIP_TRY(c, hipEventRecord(c->ev[4], c->s_dx));
    if (!c->overlap) HIP_TRY(c, hipStreamSynchronize(c->s_dx));   // isolated phase timings: nothing else on the device

    HIP_TRY(c, hipEventRecord(c->ev[0], c->s_mc));
    bool need_log = c->has_mc && c->mode == RH_MODE_LOG && c->model != RH_MODEL_VIENNA_BL;
    if (c->has_mc && c->model == RH_MODEL_VIENNA_BL) {
        bool log_path = c->mode == RH_MODE_LOG;
        if (!log_path) {   // scaled linear sweeps; a sequence that leaves the double range sends the batch to the log-space kernels
            if ((rc = run_graphed(c, c->g_in, c->s_mc, 0, launch_mc_vlin, mc_vlin_args(c, 0, false)))) return rc;
            HIP_TRY(c, hipEventRecord(c->ev[1], c->s_mc));
            if (co_seed) {   // the inside tables of both molecules are final behind ev[1]
                HIP_TRY(c, hipStreamWaitEvent(c->s_dx, c->ev[1], 0));
                HIP_TRY(c, hipEventRecord(c->ev[3], c->s_dx));
                if ((rc = launch_co_lin())) return rc;
                HIP_TRY(c, hipEventRecord(c->ev[4], c->s_dx));
                c->last_dx_path = 1;
                co_lin_launched = true;
                if (!c->overlap) HIP_TRY(c, hipStreamSynchronize(c->s_dx));   // isolated phase timings: nothing else on the device
            }
            HIP_TRY(c, hipEventRecord(c->ev[5], c->s_mc));   // start of the outside phase (= ev[1] unless the seeded sweeps ran in between)
            out_from_ev5 = true;
            if ((rc = run_graphed(c, c->g_out, c->s_mc, 1, launch_mc_vlin, mc_vlin_args(c, 1, false)))) return rc;
            c->last_path = 1;
            if (c->mode == RH_MODE_AUTO) {
                if ((rc = flagged(c, c->d_bad.as<int>(), c->mc.ns, c->s_mc, &bad))) return rc;
                log_path = !bad.empty();
                if (log_path) { c->last_path = 3; c->tables_dirty = true; co_seed_bad = co_seed; }
                if (log_path && c->defer_log) {   // another exponent first (compute): this attempt ends here
                    for (int k : bad) { c->flagged_mc.push_back(k); if (c->has_dx) c->flagged_pairs.push_back(k / 2); }
                    c->deferred = true;
                    log_path = false;
                }
            }
        }
        if (log_path) {
            c->went_log = true;
            out_from_ev5 = false;
            c->n_launch[0] = c->n_launch[1] = 0;
            c->n_far[0] = c->n_far[1] = 0;
            HIP_TRY(c, hipEventRecord(c->ev[0], c->s_mc));
            HIP_TRY(c, hipMemsetAsync(c->d_bp.p, 0, sizeof(double) * c->mc.tri_stride * c->mc.ns, c->s_mc));
            if ((rc = launch_mc_vienna(c, pin))) return rc;
            if (c->last_path == 0) c->last_path = 2;
        }
    } else if (c->has_mc && c->mode != RH_MODE_LOG) {
        // on the exponent most of the last batch needed (scale-exponent ladder), or the default one
        const bool on_rung = c->mode == RH_MODE_AUTO && c->scale_ladder && c->lin_primary >= 0 && c->lin_r;
        const LinSet* lin = on_rung ? &c->lin_r[c->lin_primary] : &c->lin0;
        if ((rc = run_graphed(c, c->g_in, c->s_mc, 0, launch_mc_lin, mc_lin_args(c, 0, c->mc, lin, true)))) return rc;
        HIP_TRY(c, hipEventRecord(c->ev[1], c->s_mc));
        if ((rc = run_graphed(c, c->g_out, c->s_mc, 1, launch_mc_lin, mc_lin_args(c, 1, c->mc, lin, true)))) return rc;
        c->last_path = 1;
        if (c->mode == RH_MODE_AUTO) {  // did every sequence stay inside the double range?
            if ((rc = flagged(c, c->d_bad.as<int>(), c->mc.ns, c->s_mc, &c->fallback_mc))) return rc;
            if (!c->fallback_mc.empty()) {
                c->last_path = 3;
                c->tables_dirty = true;
                if ((rc = retry_mc_lin_rungs(c, lin, &c->fallback_mc))) return rc;   // another exponent first; what is left goes to log space
                for (int q = 0; q <= rh_ctx::kRungs; q++)   // more than half of the batch on one exponent: the next batch starts there
                    if (c->scale_memory && c->mc.ns >= 8 && 2 * c->rescued_by[q] > c->mc.ns) c->lin_primary = q - 1;   // (a batch, not a single call)
                if (c->fallback_mc.empty()) { }
                else if (2 * c->fallback_mc.size() > (size_t)c->mc.ns) need_log = true;   // most of the batch: redo it whole
                else if ((rc = recompute_mc_subset_log(c, c->fallback_mc))) return rc;
            }
        }
    } else {
        HIP_TRY(c, hipEventRecord(c->ev[1], c->s_mc));
    }
    if (need_log) {
        c->n_launch[0] = c->n_launch[1] = 0;
        c->n_far[0] = c->n_far[1] = 0;
        HIP_TRY(c, hipEventRecord(c->ev[0], c->s_mc));
        HIP_TRY(c, hipMemsetAsync(c->d_bp.p, 0, sizeof(double) * c->mc.tri_stride * c->mc.ns, c->s_mc));
        if ((rc = launch_mc_log(c, pin, c->mc, c->d_mclogz.as<double>()))) return rc;
        if (c->last_path == 0) c->last_path = 2;
    }
    HIP_TRY(c, hipEventRecord(c->ev[2], c->s_mc));
    if (co_lin_launched && c->mode == RH_MODE_AUTO) {
        if ((rc = flagged(c, c->d_cobad.as<int>(), c->co.ns, c->s_dx, &bad))) return rc;
        const bool redo = co_seed_bad || !bad.empty();   // (a molecule left the double range on its own: what was copied from its fold is not usable)
        if (redo && c->defer_log) {
            c->tables_dirty = true; c->deferred = true;
            c->flagged_pairs.insert(c->flagged_pairs.end(), bad.begin(), bad.end());
        }
        else if (redo) {   // some pair left the double range: recompute the two-molecule sweeps in log space
            c->went_log = true;
            c->tables_dirty = true;
            c->n_launch[2] = 0; c->n_far[2] = 0;
            HIP_TRY(c, hipEventRecord(c->ev[3], c->s_dx));
            HIP_TRY(c, hipMemsetAsync(c->d_cobp.p, 0, sizeof(double) * c->co.tri_stride * c->co.ns, c->s_dx));
            if ((rc = launch_cofold(c))) return rc;
            HIP_TRY(c, hipEventRecord(c->ev[4], c->s_dx));
            c->last_dx_path = 3;
        }
    }
    if (dx_lin_launched) {
        c->last_dx_path = 1;
        if (dx_mode == RH_MODE_AUTO) {
            if ((rc = flagged(c, c->d_dxbad.as<int>(), c->dx.np, c->s_dx, &c->fallback_dx))) return rc;
            const bool redo = !c->fallback_dx.empty();
            if (redo && c->model != RH_MODEL_VIENNA_BL && 2 * c->fallback_dx.size() <= (size_t)c->dx.np) {
                // only the flagged pairs, as a compacted sub-batch with its own tables: another scale exponent on the linear kernels
                // first (retry_dx_lin_rungs), the log-space kernels for what is left
                if ((rc = retry_dx_lin_rungs(c, &c->fallback_dx))) return rc;
                if (!c->fallback_dx.empty() && (rc = recompute_dx_subset_log(c, c->fallback_dx))) return rc;
                HIP_TRY(c, hipEventRecord(c->ev[4], c->s_dx));
                c->last_dx_path = 3;
            } else if (redo && c->model == RH_MODEL_VIENNA_BL && c->defer_log) {   // (compute: the flagged pairs go to the helper context)
                c->tables_dirty = true; c->deferred = true;
                c->flagged_pairs.insert(c->flagged_pairs.end(), c->fallback_dx.begin(), c->fallback_dx.end());
                c->fallback_dx.clear();
            } else if (redo) {  // most pairs (or the Vienna-BL model): recompute the batch with the log-space kernels
                c->n_launch[2] = 0;
                HIP_TRY(c, hipEventRecord(c->ev[3], c->s_dx));
                if ((rc = (c->model == RH_MODEL_VIENNA_BL ? launch_dx_vlog(c) : launch_dx_log(c, c->dx)))) return rc;
                c->dxtab_log = true;
                HIP_TRY(c, hipEventRecord(c->ev[4], c->s_dx));
                c->last_dx_path = 3;
            }
        }
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_dx));
    float t01 = 0, t12 = 0, t34 = 0, t02 = 0;
    HIP_TRY(c, hipEventElapsedTime(&t01, c->ev[0], c->ev[1]));
    HIP_TRY(c, hipEventElapsedTime(&t12, c->ev[out_from_ev5 && !c->overlap ? 5 : 1], c->ev[2]));
    HIP_TRY(c, hipEventElapsedTime(&t02, c->ev[0], c->ev[2]));
    HIP_TRY(c, hipEventElapsedTime(&t34, c->ev[3], c->ev[4]));
    c->ms[0] = t01; c->ms[1] = t12; c->ms[2] = t34; c->ms[3] = std::max(t02, t34);
    c->computed = true;
    return RH_OK;
}

int compute(rh_ctx* c)
{
    c->defer_log = false;
    c->flagged_mc.clear();
    const bool ladder = c->model == RH_MODEL_VIENNA_BL && c->mode == RH_MODE_AUTO && c->scale_ladder && c->has_mc && c->h_vienna &&
                        c->vienna_sem != kViennaSem20 && !std::getenv("RH_VLIN_S");
    if (!ladder) return compute_once(c);
    HIP_TRY(c, hipSetDevice(c->device));
    // the exponent the batch starts with, then the others: larger ones ascending, smaller ones descending
    std::vector<int> order = {c->vlin_primary};
    {
        std::vector<std::pair<double, int>> all = {{c->vlin_m[0].h->s, -1}};
        for (int r = 0; r < rh_ctx::kVRungs; r++) all.push_back({kVRungS[r], r});
        std::sort(all.begin(), all.end());
        const double s0 = c->vlin_primary < 0 ? c->vlin_m[0].h->s : kVRungS[c->vlin_primary];
        for (const auto& e : all) if (e.first > s0 + 1e-12) order.push_back(e.second);
        for (auto it = all.rbegin(); it != all.rend(); ++it) if (it->first < s0 - 1e-12) order.push_back(it->second);
    }
    // (An attempt that failed leaves Inf / NaN in the tables of the flagged sequences; the next attempt runs over them without a clear.
    //  That is sound because the vlin kernels mask every operand by SELECT (`ok ? x : 0.0`), never by a multiplication with 0, and
    //  rewrite every interior cell they read before reading it -- the invariant `tests: test_vienna_bl_scale_exponent_ladder` and
    //  tools/fuzz_ladder.py exercise: chains of hairpins that overflow the first exponent, results equal to the log-space path's.)
    int rc = RH_OK;
    const bool per_pair = !c->is_helper && c->pair_helper && c->has_dx && c->np >= 4 && !c->mc.allow && !c->co.allow;
    for (size_t a = 0; a < order.size(); a++) {
        if ((rc = select_vlin(c, order[a]))) break;
        c->defer_log = a + 1 < order.size();
        c->flagged_pairs.clear();
        if ((rc = compute_once(c))) break;
        if (c->deferred && a == 0 && per_pair) {
            std::sort(c->flagged_pairs.begin(), c->flagged_pairs.end());
            c->flagged_pairs.erase(std::unique(c->flagged_pairs.begin(), c->flagged_pairs.end()), c->flagged_pairs.end());
            // cost: the helper pays the launch latency of a few pairs (tens of ms per attempt at n = 500 - 1000, whatever the batch), a
            // second pass over the batch pays its whole device time again: the helper wins when the flagged pairs are a small share
            // (measured at n = 500: equal at 64 pairs and one flagged pair, 2 x at 256).  RH_PAIR_HELPER=2: whenever at most half are flagged
            const size_t share = c->pair_helper >= 2 ? 2 : 16;
            if (!c->flagged_pairs.empty() && share * c->flagged_pairs.size() <= (size_t)c->np) {
                rc = recompute_pairs_on_helper(c, c->flagged_pairs);
                break;
            }
        }
        if (!c->deferred) {
            if (a > 0) {   // held by another exponent
                c->last_path = 3;
                std::sort(c->flagged_mc.begin(), c->flagged_mc.end());
                c->flagged_mc.erase(std::unique(c->flagged_mc.begin(), c->flagged_mc.end()), c->flagged_mc.end());
                if (!c->went_log) {   // (the last attempt may still have ended in log space)
                    c->rescaled_mc = c->flagged_mc;
                    if (c->scale_memory && c->mc.ns >= 8) c->vlin_primary = order[a];   // a batch, not a single call: the next one starts here
                }
            }
            break;
        }
    }
    c->defer_log = false;
    const int back = select_vlin(c, c->vlin_primary);
    return rc ? rc : back;
}

}  // namespace rh::host
