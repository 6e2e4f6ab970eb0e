// compute.hip -- one batch from staged to computed: hipGraph capture / replay of the launch sequences, the two streams
// and their events, and the decision which fallback a flagged problem takes: one schedule per product (CONTRAfold folds + duplex,
// Vienna-BL folds + pf_duplex, Vienna-BL folds + two-molecule ensemble) under one driver (run_attempt), and compute() above it.
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
    A.pin = xcd_pin(B.ns);
    A.strip_xcd = c->strip_xcd;
    A.f5_jlo = 32;   // inside_pairs(S, A, 30) ends with F5i[31]
    A.up_w = c->max_w;
    A.f5_pass = c->f5_pass && f5_pass_fits(B.ld);   // (F5 in LDS: up to about 4300 letters; longer batches keep the serial kernels)
    return A;
}

// One phase over the staged single-molecule batch or (co) the s1+s2 batch, on the model select_vlin selected last
static McVlinArgs mc_vlin_args(const rh_ctx* c, int phase, bool co)
{
    McVlinArgs A;
    A.B = co ? c->co : c->mc; A.phase = phase; A.co = co;
    A.pin = xcd_pin(A.B.ns);
    A.plan = plan_mc_vlin(c, phase, co, A.B.nmax);
    A.d_vlin = c->d_vlin; A.h_vlin = c->h_vlin; A.hplen = c->h_hplen.data(); A.d_hplen = c->d_hplen.as<const double>();
    A.bad = co ? c->d_cobad.as<int>() : c->d_bad.as<int>();
    if (co) {
        const DxBatch& D = c->dx;
        if (A.B.seeded) { A.from = c->mc; A.pair_seq = c->d_pidx.as<const int>(); }
        A.hp = D.hp; A.hp_logz = D.logz; A.hp_stride = D.tab_stride; A.hp_ldd = D.ldd; A.n1max = D.n1max; A.n2max = D.n2max;
        A.cut_min = c->co_cut_min; A.cut_max = c->co_cut_max;
        A.window = c->co_window && c->co_cut_min >= 1 && (phase == 1 || A.B.seeded);   // (an unseeded inside sweep computes every group)
    } else {
        A.logz = c->d_mclogz.as<double>(); A.gaps = c->d_gaps.as<double>(); A.max_w = c->max_w;
        // (vlin_acc_gaps_wide addresses a sequence's tables with 32-bit offsets; vlin_acc_final_t has up to fifteen widths)
        A.acc_wide = c->acc_wide && (size_t)VM_COUNT * A.B.tab_stride * sizeof(double) < ((size_t)1 << 32);
        A.acc_final_t = c->acc_final_t && c->max_w <= 15;
    }
    return A;
}

// The hybridization sweeps over the staged batch of pairs: what both models' arguments share ...
static DxLinArgs dx_args(const rh_ctx* c)
{
    DxLinArgs A;
    A.X = c->dxl; A.plan = c->plan[2]; A.lz_chunks = c->lz_chunks;
    A.zpart = c->d_zpart.as<double>(); A.zbar = c->d_zbar.as<double>();
    A.logz = c->d_logz.as<double>(); A.bad = c->d_dxbad.as<int>();
    return A;
}

// ... of launch_dx_lin (CONTRAfold model) ...
DxLinArgs dx_lin_args(const rh_ctx* c)
{
    DxLinArgs A = dx_args(c);
    A.dm = c->d_dxlin; A.hm = &c->h_dxlin;
    return A;
}

// ... and of launch_dx_vlin (Vienna-BL pf_duplex)
static DxLinArgs dx_vlin_args(const rh_ctx* c)
{
    DxLinArgs A = dx_args(c);
    A.vdx_s = c->vdx_s; A.sem20 = c->vienna_sem == kViennaSem20;
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

// ---- One attempt at the staged batch: what compute() asks of a schedule, and what the schedule reports back.  Only the Vienna-BL
// schedules defer (compute() has another exponent for the whole batch); the CONTRAfold schedule settles its flags itself.
struct Attempt {
    bool defer_log = false;           // in: a flagged problem ends the attempt instead of starting the log-space kernels
    bool deferred = false;            // out: it ended that way ...
    std::vector<int> flagged_seqs;    // ... with these sequences (folds) ...
    std::vector<int> flagged_pairs;   // ... and pairs (folds, two-molecule sweeps or pf_duplex) flagged
    bool went_log = false;            // out: the folds or the two-molecule sweeps ran on the log-space kernels
    Ev outside_from = kEvMcInside;    // out: the event the outside phase starts at (kEvMcOutside: something ran between the sweeps)
};

// ---- what the schedules share
// The hybridization stream is fed: its end event, and -- isolated phase timings -- nothing else on the device while it runs
static int close_dx_phase(rh_ctx* c)
{
    HIP_TRY(c, hipEventRecord(c->ev[kEvDxEnd], c->s_dx));
    if (!c->overlap) HIP_TRY(c, hipStreamSynchronize(c->s_dx));
    return RH_OK;
}

// Start the folds over in log space on the McCaskill stream: what the linear pass launched does not count, the phase times start
// again, the bp rows are cleared, `launch` feeds the stream
template <class Launch>
static int restart_mc_log(rh_ctx* c, Launch launch)
{
    c->n_launch[0] = c->n_launch[1] = 0;
    c->n_far[0] = c->n_far[1] = 0;
    HIP_TRY(c, hipEventRecord(c->ev[kEvMcStart], c->s_mc));
    HIP_TRY(c, hipMemsetAsync(c->d_bp.p, 0, sizeof(double) * c->mc.tri_stride * c->mc.ns, c->s_mc));
    if (int rc = launch()) return rc;
    if (c->last_path == 0) c->last_path = 2;
    return RH_OK;
}

// The same for the hybridization source on its stream.  clear_cobp: the two-molecule sweeps accumulate into their bp rows; pf_duplex
// and the duplex sweeps clear nothing
template <class Launch>
static int restart_dx_log(rh_ctx* c, bool clear_cobp, Launch launch)
{
    c->n_launch[2] = 0; c->n_far[2] = 0;
    HIP_TRY(c, hipEventRecord(c->ev[kEvDxStart], c->s_dx));
    if (clear_cobp) HIP_TRY(c, hipMemsetAsync(c->d_cobp.p, 0, sizeof(double) * c->co.tri_stride * c->co.ns, c->s_dx));
    if (int rc = launch()) return rc;
    HIP_TRY(c, hipEventRecord(c->ev[kEvDxEnd], c->s_dx));
    c->last_dx_path = 3;
    return RH_OK;
}

// ---- CONTRAfold model: duplex sweeps on s_dx, folds on s_mc; every flagged problem is settled here, alone where it can be
static int schedule_contrafold(rh_ctx* c, int dx_mode)
{
    int rc;
    // duplex first on its own stream: it is independent of the McCaskill sweeps and overlaps them
    const bool dx_lin = c->has_dx && dx_mode != RH_MODE_LOG;
    if (dx_lin) {
        if ((rc = run_graphed(c, c->g_dx, c->s_dx, 2, launch_dx_lin, dx_lin_args(c)))) return rc;
    } else if (c->has_dx) {
        if ((rc = launch_dx_log(c, c->dx))) return rc;
        c->dxtab_log = true;
        c->last_dx_path = 2;
    }
    if ((rc = close_dx_phase(c))) return rc;

    HIP_TRY(c, hipEventRecord(c->ev[kEvMcStart], c->s_mc));
    bool need_log = c->has_mc && c->mode == RH_MODE_LOG;
    if (c->has_mc && c->mode != RH_MODE_LOG) {
        // on the exponent most of the last batch needed (scale-exponent ladder), or the default one
        const int model = c->mode == RH_MODE_AUTO && c->scale_ladder && c->lin_primary >= 0 && c->lin_r ? c->lin_primary : -1;
        const LinSet* lin = model < 0 ? &c->lin0 : &c->lin_r[model];
        if ((rc = run_graphed(c, c->g_in, c->s_mc, 0, launch_mc_lin, mc_lin_args(c, 0, c->mc, lin, true)))) return rc;
        HIP_TRY(c, hipEventRecord(c->ev[kEvMcInside], c->s_mc));
        if ((rc = run_graphed(c, c->g_out, c->s_mc, 1, launch_mc_lin, mc_lin_args(c, 1, c->mc, lin, true)))) return rc;
        if ((rc = launch_mc_acc(c, c->mc, lin, true))) return rc;   // (region accessibility, when it is on: outside the graph)
        c->last_path = 1;
        if (c->mode == RH_MODE_AUTO) {  // did every sequence stay inside the double range?
            if ((rc = flagged(c, c->d_bad.as<int>(), c->mc.ns, c->s_mc, &c->fallback_mc))) return rc;
            if (!c->fallback_mc.empty()) {
                c->last_path = 3;
                c->tables_dirty = true;
                int rescued_by[rh_ctx::kRungs + 1];
                if ((rc = retry_mc_lin_rungs(c, model, &c->fallback_mc, rescued_by))) return rc;   // another exponent first; what is left goes to log space
                for (int q = 0; q <= rh_ctx::kRungs; q++)   // more than half of the batch on one exponent: the next batch starts there
                    if (c->scale_memory && c->mc.ns >= 8 && 2 * rescued_by[q] > c->mc.ns) c->lin_primary = q - 1;   // (a batch, not a single call)
                if (c->fallback_mc.empty()) { }
                else if (2 * c->fallback_mc.size() > (size_t)c->mc.ns) need_log = true;   // most of the batch: redo it whole
                else if ((rc = recompute_mc_subset_log(c, c->fallback_mc))) return rc;
            }
        }
    } else {
        HIP_TRY(c, hipEventRecord(c->ev[kEvMcInside], c->s_mc));
    }
    if (need_log && (rc = restart_mc_log(c, [&] {
            const int r = launch_mc_log(c, xcd_pin(c->mc.ns), c->mc, c->d_mclogz.as<double>());
            return r ? r : launch_mc_acc(c, c->mc, nullptr, true);
        }))) return rc;
    HIP_TRY(c, hipEventRecord(c->ev[kEvMcEnd], c->s_mc));

    if (dx_lin) {
        c->last_dx_path = 1;
        if (dx_mode == RH_MODE_AUTO) {
            if ((rc = flagged(c, c->d_dxbad.as<int>(), c->dx.np, c->s_dx, &c->fallback_dx))) return rc;
            if (c->fallback_dx.empty()) { }
            else if (2 * c->fallback_dx.size() <= (size_t)c->dx.np) {
                // only the flagged pairs, as a compacted sub-batch with its own tables: another scale exponent on the linear kernels
                // first (retry_dx_lin_rungs), the log-space kernels for what is left
                if ((rc = retry_dx_lin_rungs(c, &c->fallback_dx))) return rc;
                if (!c->fallback_dx.empty() && (rc = recompute_dx_subset_log(c, c->fallback_dx))) return rc;
                HIP_TRY(c, hipEventRecord(c->ev[kEvDxEnd], c->s_dx));
                c->last_dx_path = 3;
            } else {   // most pairs: recompute the batch with the log-space kernels
                if ((rc = restart_dx_log(c, false, [&] { return launch_dx_log(c, c->dx); }))) return rc;
                c->dxtab_log = true;
            }
        }
    }
    return RH_OK;
}

// ---- Vienna-BL model: the single-molecule folds of both schedules on s_mc, up to their end event.  between(): what the schedule
// puts behind the inside sweep.  A flagged sequence sends the BATCH to the log-space kernels, or ends the attempt (defer_log).
// *overflowed: a sequence was flagged
template <class Between>
static int vienna_folds(rh_ctx* c, Attempt* at, Between between, bool* overflowed)
{
    int rc;
    *overflowed = false;
    HIP_TRY(c, hipEventRecord(c->ev[kEvMcStart], c->s_mc));
    if (!c->has_mc) {
        HIP_TRY(c, hipEventRecord(c->ev[kEvMcInside], c->s_mc));
        HIP_TRY(c, hipEventRecord(c->ev[kEvMcEnd], c->s_mc));
        return RH_OK;
    }
    bool log_path = c->mode == RH_MODE_LOG;
    if (!log_path) {   // scaled linear sweeps; a sequence that leaves the double range sends the batch to the log-space kernels
        if ((rc = run_graphed(c, c->g_in, c->s_mc, 0, launch_mc_vlin, mc_vlin_args(c, 0, false)))) return rc;
        HIP_TRY(c, hipEventRecord(c->ev[kEvMcInside], c->s_mc));
        if ((rc = between())) return rc;
        HIP_TRY(c, hipEventRecord(c->ev[kEvMcOutside], c->s_mc));   // (= kEvMcInside unless something ran in between)
        at->outside_from = kEvMcOutside;
        if ((rc = run_graphed(c, c->g_out, c->s_mc, 1, launch_mc_vlin, mc_vlin_args(c, 1, false)))) return rc;
        c->last_path = 1;
        if (c->mode == RH_MODE_AUTO) {
            std::vector<int> bad;
            if ((rc = flagged(c, c->d_bad.as<int>(), c->mc.ns, c->s_mc, &bad))) return rc;
            log_path = *overflowed = !bad.empty();
            if (log_path) { c->last_path = 3; c->tables_dirty = true; }
            if (log_path && at->defer_log) {   // another exponent first (compute): this attempt ends here
                for (int k : bad) { at->flagged_seqs.push_back(k); if (c->has_dx) pairs_of_seq(c, k, &at->flagged_pairs); }
                at->deferred = true;
                log_path = false;
            }
        }
    }
    if (log_path) {
        at->went_log = true;
        at->outside_from = kEvMcInside;
        if ((rc = restart_mc_log(c, [&] { return launch_mc_vienna(c, xcd_pin(c->mc.ns)); }))) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev[kEvMcEnd], c->s_mc));
    return RH_OK;
}

// ---- Vienna-BL model, hp from pf_duplex: its sweeps on s_dx, the folds on s_mc; a flagged pair sends the batch of pairs to the
// log-space kernels, or ends the attempt (defer_log: the flagged pairs go to the helper context, or the batch to another exponent)
static int schedule_vienna_duplex(rh_ctx* c, int dx_mode, Attempt* at)
{
    int rc;
    const bool dx_lin = c->has_dx && dx_mode != RH_MODE_LOG;
    if (dx_lin) {
        if ((rc = run_graphed(c, c->g_dx, c->s_dx, 2, launch_dx_vlin, dx_vlin_args(c)))) return rc;
    } else if (c->has_dx) {
        if ((rc = launch_dx_vlog(c))) return rc;
        c->dxtab_log = true;
        c->last_dx_path = 2;
    }
    if ((rc = close_dx_phase(c))) return rc;

    bool overflowed;
    if ((rc = vienna_folds(c, at, [] { return (int)RH_OK; }, &overflowed))) return rc;

    if (dx_lin) {
        c->last_dx_path = 1;
        if (dx_mode == RH_MODE_AUTO) {
            if ((rc = flagged(c, c->d_dxbad.as<int>(), c->dx.np, c->s_dx, &c->fallback_dx))) return rc;
            if (c->fallback_dx.empty()) { }
            else if (at->defer_log) {
                c->tables_dirty = true; at->deferred = true;
                at->flagged_pairs.insert(at->flagged_pairs.end(), c->fallback_dx.begin(), c->fallback_dx.end());
                c->fallback_dx.clear();
            } else {
                if ((rc = restart_dx_log(c, false, [&] { return launch_dx_vlog(c); }))) return rc;
                c->dxtab_log = true;
            }
        }
    }
    return RH_OK;
}

// ---- Vienna-BL model, hp from the two-molecule ensemble: sweeps over s1+s2 on s_dx, the folds on s_mc.  Without structure
// constraints the sweeps are seeded: their cells on one strand are copied from the folds of the same pairs (vlin_co_seed), so they
// start behind the inside sweep of the folds instead of next to it; through the index of the upload, N + M folds seed N x M sweeps.  A flagged pair -- or, seeded, a flagged sequence: what was
// copied from its fold is not usable -- sends the batch of pairs to the log-space kernels, or ends the attempt (defer_log)
static int schedule_vienna_cofold(rh_ctx* c, Attempt* at)
{
    int rc;
    // (both sequences of every pair are in c->mc: stage() has checked the index of an upload that has folds and pairs against it)
    const bool seed = c->has_dx && c->has_mc && c->mode != RH_MODE_LOG && c->co_seed && !c->mc.allow && !c->co.allow &&
                      c->pair_seq.size() == 2 * (size_t)c->co.ns && c->mc.ns == c->ns;
    c->co.seeded = seed ? 1 : 0;
    bool lin_launched = false;   // (its overflow flags are read after the McCaskill stream has been fed: the two overlap)
    const auto launch_lin = [&]() -> int {   // scaled linear sweeps over s1+s2, one graph of both phases
        if (int r = run_graphed(c, c->g_dx, c->s_dx, 2, launch_mc_vlin, mc_vlin_args(c, 0, true), mc_vlin_args(c, 1, true))) return r;
        c->last_dx_path = 1;
        lin_launched = true;
        return RH_OK;
    };
    if (c->has_dx) {
        HIP_TRY(c, hipMemsetAsync(c->d_cobp.p, 0, sizeof(double) * c->co.tri_stride * c->co.ns, c->s_dx));
        if (c->mode == RH_MODE_LOG) {
            if ((rc = launch_cofold(c))) return rc;
            if (c->last_dx_path != 3) c->last_dx_path = 2;
        } else if (!seed) {
            if ((rc = launch_lin())) return rc;
        }
    }
    if ((rc = close_dx_phase(c))) return rc;

    bool overflowed;
    const auto seeded_sweeps = [&]() -> int {   // the inside tables of both molecules are final behind kEvMcInside
        if (!seed) return RH_OK;
        HIP_TRY(c, hipStreamWaitEvent(c->s_dx, c->ev[kEvMcInside], 0));
        HIP_TRY(c, hipEventRecord(c->ev[kEvDxStart], c->s_dx));
        if (int r = launch_lin()) return r;
        return close_dx_phase(c);
    };
    if ((rc = vienna_folds(c, at, seeded_sweeps, &overflowed))) return rc;

    if (lin_launched && c->mode == RH_MODE_AUTO) {
        std::vector<int> bad;
        if ((rc = flagged(c, c->d_cobad.as<int>(), c->co.ns, c->s_dx, &bad))) return rc;
        const bool redo = (seed && overflowed) || !bad.empty();
        if (redo && at->defer_log) {
            c->tables_dirty = true; at->deferred = true;
            at->flagged_pairs.insert(at->flagged_pairs.end(), bad.begin(), bad.end());
        } else if (redo) {
            at->went_log = true;
            c->tables_dirty = true;
            if ((rc = restart_dx_log(c, true, [&] { return launch_cofold(c); }))) return rc;
        }
    }
    return RH_OK;
}

// ---- the driver: what every product needs before and behind its schedule
static int run_attempt(rh_ctx* c, Attempt* at)
{
    HIP_TRY(c, hipSetDevice(c->device));
    c->tev_n = 0;
    c->n_launch[0] = c->n_launch[1] = c->n_launch[2] = 0;
    c->n_far[0] = c->n_far[1] = c->n_far[2] = 0;
    c->last_path = 0;
    c->last_went_log = false;
    c->acc_timed = false;
    c->fallback_mc.clear(); c->fallback_dx.clear(); c->rescaled_mc.clear(); c->rescaled_dx.clear();
    const bool vienna = c->model == RH_MODEL_VIENNA_BL, cofold = vienna && c->hybrid == RH_HYBRID_COFOLD;
    // the organisation of each sweep's linear first pass: decided here, on every compute (a replayed graph does not call its launcher);
    // the arguments of the launchers carry the same plans to them
    for (int phase = 0; phase < 2; phase++) c->plan[phase] = vienna ? plan_mc_vlin(c, phase, false, c->mc.nmax) : plan_mc_lin(c, phase, c->mc.nmax);
    c->plan[2] = !vienna ? plan_dx_lin(c, c->dx_w) : cofold ? plan_mc_vlin(c, 0, true, c->co.nmax) : plan_dx_vlin(c->vienna_sem == kViennaSem20);
    // the path of the duplex / pf_duplex sweeps: rh_set_duplex_mode, or what rh_set_mode says
    const int dx_mode = c->duplex_mode == RH_MODE_INHERIT ? c->mode : c->duplex_mode;
    // the linear duplex kernels share d_dxtab with the log-space ones and read zero pad columns: after a log-space compute on this
    // upload (another mode since, or a fallback) the image stage() left is gone
    if (c->has_dx && c->dxtab_log && dx_mode != RH_MODE_LOG && !cofold) {
        HIP_TRY(c, hipMemsetAsync(c->d_dxtab.p, 0, c->dx_bytes, c->s_dx));
        c->dxtab_log = false;
    }
    HIP_TRY(c, hipEventRecord(c->ev[kEvDxStart], c->s_dx));   // (the McCaskill stream's start event: where the schedule turns to it)

    if (int rc = !vienna ? schedule_contrafold(c, dx_mode) : cofold ? schedule_vienna_cofold(c, at) : schedule_vienna_duplex(c, dx_mode, at)) return rc;

    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_dx));
    float t01 = 0, t12 = 0, t34 = 0, t02 = 0;
    HIP_TRY(c, hipEventElapsedTime(&t01, c->ev[kEvMcStart], c->ev[kEvMcInside]));
    HIP_TRY(c, hipEventElapsedTime(&t12, c->ev[c->overlap ? kEvMcInside : at->outside_from], c->ev[kEvMcEnd]));
    HIP_TRY(c, hipEventElapsedTime(&t02, c->ev[kEvMcStart], c->ev[kEvMcEnd]));
    HIP_TRY(c, hipEventElapsedTime(&t34, c->ev[kEvDxStart], c->ev[kEvDxEnd]));
    c->ms[0] = t01; c->ms[1] = t12; c->ms[2] = t34; c->ms[3] = std::max(t02, t34);
    c->last_went_log = at->went_log;
    c->computed = true;
    return RH_OK;
}

int compute(rh_ctx* c)
{
    const bool ladder = c->model == RH_MODEL_VIENNA_BL && c->mode == RH_MODE_AUTO && c->scale_ladder && c->has_mc && c->h_vienna &&
                        c->vienna_sem != kViennaSem20 && !std::getenv("RH_VLIN_S");
    if (!ladder) { Attempt at; return run_attempt(c, &at); }
    HIP_TRY(c, hipSetDevice(c->device));
    // the exponent the batch starts with, then the others
    std::vector<int> order = {c->vlin_primary};
    for (int model : exponent_order(c->vlin_primary, c->vlin_m[0].h->s, kVRungS, rh_ctx::kVRungs)) order.push_back(model);
    // (An attempt that failed leaves Inf / NaN in the tables of the flagged sequences; the next attempt runs over them without a clear.
    //  That is sound because the vlin kernels mask every operand by SELECT (`ok ? x : 0.0`), never by a multiplication with 0, and
    //  rewrite every interior cell they read before reading it -- the invariant `tests: test_vienna_bl_scale_exponent_ladder` and
    //  tools/fuzz_ladder.py exercise: chains of hairpins that overflow the first exponent, results equal to the log-space path's.
    //  An attempt that UNDERFLOWED leaves zeros and denormals instead; tests/test_gpu_vanishing.py runs 0.7 and 1.8 over those before
    //  s = 0 holds the batch, against the oracle.)
    int rc = RH_OK;
    // (the helper recomputes whole pairs and copies their folds back into the pairs' own rows: an indexed batch, whose fold rows are
    //  shared between pairs, runs the whole batch again instead)
    const bool per_pair = !c->is_helper && c->pair_helper && c->has_dx && c->np >= 4 && !c->mc.allow && !c->co.allow && !c->indexed;
    const auto sort_unique = [](std::vector<int>& v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); };
    std::vector<int> flagged_seqs;   // by the deferred attempts so far
    bool pairs_alone = false;        // the first attempt flagged two-molecule sweeps and no fold: the joint ensemble left the range by itself
    for (size_t a = 0; a < order.size(); a++) {
        if ((rc = select_vlin(c, order[a]))) break;
        Attempt at;
        at.defer_log = a + 1 < order.size();
        if ((rc = run_attempt(c, &at))) break;
        flagged_seqs.insert(flagged_seqs.end(), at.flagged_seqs.begin(), at.flagged_seqs.end());
        if (a == 0) pairs_alone = at.deferred && at.flagged_seqs.empty() && !at.flagged_pairs.empty() && c->hybrid == RH_HYBRID_COFOLD;
        if (at.deferred && a == 0 && per_pair) {
            sort_unique(at.flagged_pairs);
            // cost: the helper pays the launch latency of a few pairs (tens of ms per attempt at n = 500 - 1000, whatever the batch), a
            // second pass over the batch pays its whole device time again: the helper wins when the flagged pairs are a small share
            // (measured at n = 500: equal at 64 pairs and one flagged pair, 2 x at 256).  RH_PAIR_HELPER=2: whenever at most half are flagged
            const size_t share = c->pair_helper >= 2 ? 2 : 16;
            if (!at.flagged_pairs.empty() && share * at.flagged_pairs.size() <= (size_t)c->np) {
                rc = recompute_pairs_on_helper(c, at.flagged_pairs);
                break;
            }
        }
        if (!at.deferred) {
            if (a > 0) {   // held by another exponent
                c->last_path = 3;
                // two-molecule sweeps that vanished (or overflowed) while every fold stayed inside, held by this exponent: the hybrid
                // path says so as the path of the folds does (sweeps that only followed a flagged fold keep reporting 1)
                if (pairs_alone && c->last_dx_path == 1) c->last_dx_path = 3;
                sort_unique(flagged_seqs);
                if (!at.went_log) {   // (the last attempt may still have ended in log space)
                    c->rescaled_mc = flagged_seqs;
                    if (c->scale_memory && c->mc.ns >= 8) c->vlin_primary = order[a];   // a batch, not a single call: the next one starts here
                }
            }
            break;
        }
    }
    const int back = select_vlin(c, c->vlin_primary);
    return rc ? rc : back;
}

}  // namespace rh::host
