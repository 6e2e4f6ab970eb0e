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

// ---- hipGraph replay of the fast path.  The launch sequence of a batch depends only on its shape (and on the
// buffer addresses baked into the kernel arguments), so it is captured once per shape and replayed: the ~1000
// launches per sweep then cost the GPU-side ~1.5 us boundary instead of a host launch each.
template <class F>
int run_graphed(rh_ctx* c, GraphSlot& g, size_t key, hipStream_t stream, int* launch_counter, int* far_counter, F&& launch)
{
    if (!c->use_graphs || c->time_cls >= 0) return launch();   // (timed launches are host launches: events between graph nodes would be captured)
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

static size_t shape_key(const rh_ctx* c, int which)
{
    auto mix = [](size_t h, size_t v) { return (h ^ v) * 0x100000001b3ull + 0x9e3779b97f4a7c15ull; };
    size_t h = 1469598103934665603ull + which;
    if (which == 3) {
        const McBatch& B = c->co;
        for (size_t v : {(size_t)B.ns, (size_t)B.nmax, (size_t)B.ld, (size_t)B.lds, (size_t)B.tab, (size_t)B.seq, (size_t)B.n, (size_t)B.f5i,
                         (size_t)B.bp, (size_t)c->d_cobad.p, (size_t)c->lin_bs, (size_t)B.tri_stride, (size_t)c->dx.hp, (size_t)c->dx.logz,
                         (size_t)c->dx.ldd, (size_t)c->dx.tab_stride, (size_t)c->dx.n1max, (size_t)c->dx.n2max, (size_t)B.allow, (size_t)B.pk,
                         (size_t)c->far_pk, (size_t)B.rowp, (size_t)c->lookahead, (size_t)B.seeded, (size_t)c->mc.tab, (size_t)c->mc.ld, (size_t)c->d_vlin,
                         // the windowed grid and its pin offset are baked into the captured launches (launch_mc_vlin)
                         (size_t)c->co_window, (size_t)(c->co_cut_min + 1), (size_t)(c->co_cut_max + 1), (size_t)(c->far2 + 2)})
            h = mix(h, v);
    } else if (which <= 1) {
        const McBatch& B = c->mc;
        for (size_t v : {(size_t)B.ns, (size_t)B.nmax, (size_t)B.ld, (size_t)B.lds, (size_t)B.tab, (size_t)B.seq, (size_t)B.n,
                         (size_t)B.f5i, (size_t)B.bp, (size_t)B.up, (size_t)c->d_bad.p, (size_t)c->d_mclogz.p, (size_t)c->lin_w, (size_t)c->lin_w_in,
                         (size_t)c->lin_bs, (size_t)B.tri_stride, (size_t)c->far_mfma, (size_t)c->max_w, (size_t)c->d_gaps.p,
                         (size_t)c->d_hplen.p, (size_t)B.allow, (size_t)B.pk, (size_t)c->far_pk, (size_t)B.rowp, (size_t)c->lookahead, (size_t)c->strip, (size_t)c->lin->wT.p, (size_t)c->strip_w, (size_t)(c->strip_filt && c->strip_filt_ok), (size_t)c->strip_xcd, (size_t)(c->far2 + 2), (size_t)c->acc_wide, (size_t)c->acc_final_t, (size_t)c->d_vlin,
                         (size_t)c->small_on, c->small_list.size(), (size_t)c->nmax_sweep, (size_t)c->d_small_list.p, (size_t)c->d_n_sweep.p,
                         (size_t)c->n_short, (size_t)c->nmax_short, (size_t)c->d_n_short.p})
            h = mix(h, v);
    } else {
        const DxLinBatch& X = c->dxl;
        for (size_t v : {(size_t)X.np, (size_t)X.n1max, (size_t)X.n2max, (size_t)X.lda, (size_t)X.ldd, (size_t)X.tab, (size_t)X.hp,
                         (size_t)X.seq, (size_t)X.n, (size_t)c->d_zbar.p, (size_t)c->d_logz.p, (size_t)c->d_dxbad.p, (size_t)c->dx_w, (size_t)c->d_zpart.p, (size_t)c->dx_quad, (size_t)c->dx_strip})
            h = mix(h, v);
    }
    return h;
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
    // the organisation of each sweep's linear first pass: decided here, on every compute (a replayed graph does not call its launcher),
    // from switches and shapes that are all part of shape_key
    const bool vienna = c->model == RH_MODEL_VIENNA_BL;
    for (int phase = 0; phase < 2; phase++) c->plan[phase] = vienna ? plan_mc_vlin(c, phase, false, c->mc.nmax) : plan_mc_lin(c, phase, c->mc.nmax);
    c->plan[2] = !vienna ? plan_dx_lin(c, c->dx_w) : c->hybrid == RH_HYBRID_COFOLD ? plan_mc_vlin(c, 0, true, c->co.nmax) : plan_dx_vlin();
    // sequence -> XCD affinity only when the batch spreads evenly over the 8 XCDs (speed only)
    const int pin = (c->has_mc && c->mc.ns % 8 == 0) ? 1 : 0;
    int rc;
    // duplex first on its own stream: it is independent of the McCaskill sweeps and overlaps them
    HIP_TRY(c, hipEventRecord(c->ev[3], c->s_dx));
    bool dx_lin_launched = false, co_lin_launched = false, co_seed_bad = false, out_from_ev5 = false;
    // two-molecule sweeps in linear space next to the single-molecule folds of the same pairs (no structure constraints): the cells
    // on one strand are copied from those folds (vlin_co_seed), so the sweeps over s1+s2 start when their inside tables are final
    const bool co_seed = c->has_dx && c->has_mc && c->model == RH_MODEL_VIENNA_BL && c->hybrid == RH_HYBRID_COFOLD && c->mode != RH_MODE_LOG &&
                         c->co_seed && !c->mc.allow && !c->co.allow && c->mc.ns == 2 * c->co.ns;
    c->co.seeded = co_seed ? 1 : 0;
    auto launch_co_lin = [&]() -> int {   // scaled linear sweeps over s1+s2; out-of-range values send the batch to the log-space kernels
        const int cpin = c->co.ns % 8 == 0 ? 1 : 0;
        return run_graphed(c, c->g_dx, shape_key(c, 3), c->s_dx, &c->n_launch[2], &c->n_far[2], [&] {
            const int r = launch_mc_vlin(c, cpin, 0, true, plan_mc_vlin(c, 0, true, c->co.nmax));
            return r ? r : launch_mc_vlin(c, cpin, 1, true, plan_mc_vlin(c, 1, true, c->co.nmax));
        });
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
        if (c->mode != RH_MODE_LOG) {   // scaled linear sweeps; pairs outside the double range send the batch to the log-space kernels
            if ((rc = run_graphed(c, c->g_dx, shape_key(c, 2), c->s_dx, &c->n_launch[2], &c->n_far[2], [&] { return launch_dx_vlin(c); }))) return rc;
            dx_lin_launched = true;
        } else {
            if ((rc = launch_dx_vlog(c))) return rc;
            c->last_dx_path = 2;
        }
    } else if (c->has_dx) {
        if (c->mode != RH_MODE_LOG) {
            if ((rc = run_graphed(c, c->g_dx, shape_key(c, 2), c->s_dx, &c->n_launch[2], &c->n_far[2], [&] { return launch_dx_lin(c, c->plan[2]); }))) return rc;
            dx_lin_launched = true;
        } else {
            if ((rc = launch_dx_log(c))) return rc;
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
            if ((rc = run_graphed(c, c->g_in, shape_key(c, 0), c->s_mc, &c->n_launch[0], &c->n_far[0], [&] { return launch_mc_vlin(c, pin, 0, false, c->plan[0]); }))) return rc;
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
            if ((rc = run_graphed(c, c->g_out, shape_key(c, 1), c->s_mc, &c->n_launch[1], &c->n_far[1], [&] { return launch_mc_vlin(c, pin, 1, false, c->plan[1]); }))) return rc;
            c->last_path = 1;
            if (c->mode == RH_MODE_AUTO) {
                std::vector<int> bad(c->mc.ns);
                HIP_TRY(c, hipMemcpyAsync(bad.data(), c->d_bad.p, sizeof(int) * c->mc.ns, hipMemcpyDeviceToHost, c->s_mc));
                HIP_TRY(c, hipStreamSynchronize(c->s_mc));
                for (int b : bad) log_path |= (b != 0);
                if (log_path) { c->last_path = 3; c->tables_dirty = true; co_seed_bad = co_seed; }
                if (log_path && c->defer_log) {   // another exponent first (compute): this attempt ends here
                    for (int k = 0; k < c->mc.ns; k++) if (bad[k]) { c->flagged_mc.push_back(k); if (c->has_dx) c->flagged_pairs.push_back(k / 2); }
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
        // the exponent most of the last batch needed (scale-exponent ladder); c->lin is the default's again afterwards
        const bool on_rung = c->mode == RH_MODE_AUTO && c->scale_ladder && c->lin_primary >= 0 && c->lin_r;
        if (on_rung) c->lin = &c->lin_r[c->lin_primary];
        struct Back { rh_ctx* c; ~Back() { c->lin = &c->lin0; } } back{c};
        if ((rc = run_graphed(c, c->g_in, shape_key(c, 0), c->s_mc, &c->n_launch[0], &c->n_far[0], [&] { return launch_mc_lin(c, pin, 0, c->plan[0]); }))) return rc;
        HIP_TRY(c, hipEventRecord(c->ev[1], c->s_mc));
        if ((rc = run_graphed(c, c->g_out, shape_key(c, 1), c->s_mc, &c->n_launch[1], &c->n_far[1], [&] { return launch_mc_lin(c, pin, 1, c->plan[1]); }))) return rc;
        c->last_path = 1;
        if (c->mode == RH_MODE_AUTO) {  // did every sequence stay inside the double range?
            std::vector<int> bad(c->mc.ns);
            HIP_TRY(c, hipMemcpyAsync(bad.data(), c->d_bad.p, sizeof(int) * c->mc.ns, hipMemcpyDeviceToHost, c->s_mc));
            HIP_TRY(c, hipStreamSynchronize(c->s_mc));
            for (int k = 0; k < c->mc.ns; k++) if (bad[k]) c->fallback_mc.push_back(k);
            if (!c->fallback_mc.empty()) {
                c->last_path = 3;
                c->tables_dirty = true;
                if ((rc = retry_mc_lin_rungs(c, &c->fallback_mc))) return rc;   // another exponent first; what is left goes to log space
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
        if ((rc = launch_mc_log(c, pin))) return rc;
        if (c->last_path == 0) c->last_path = 2;
    }
    HIP_TRY(c, hipEventRecord(c->ev[2], c->s_mc));
    if (co_lin_launched && c->mode == RH_MODE_AUTO) {
        std::vector<int> bad(c->co.ns);
        HIP_TRY(c, hipMemcpyAsync(bad.data(), c->d_cobad.p, sizeof(int) * c->co.ns, hipMemcpyDeviceToHost, c->s_dx));
        HIP_TRY(c, hipStreamSynchronize(c->s_dx));
        bool redo = co_seed_bad;   // a molecule left the double range on its own: what was copied from its fold is not usable
        for (int b : bad) redo |= (b != 0);
        if (redo && c->defer_log) {
            c->tables_dirty = true; c->deferred = true;
            for (int k = 0; k < c->co.ns; k++) if (bad[k]) c->flagged_pairs.push_back(k);
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
        if (c->mode == RH_MODE_AUTO) {
            std::vector<int> bad(c->dx.np);
            HIP_TRY(c, hipMemcpyAsync(bad.data(), c->d_dxbad.p, sizeof(int) * c->dx.np, hipMemcpyDeviceToHost, c->s_dx));
            HIP_TRY(c, hipStreamSynchronize(c->s_dx));
            bool redo = false;
            for (int k = 0; k < c->dx.np; k++) if (bad[k]) { redo = true; c->fallback_dx.push_back(k); }
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
                if ((rc = (c->model == RH_MODEL_VIENNA_BL ? launch_dx_vlog(c) : launch_dx_log(c)))) return rc;
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
