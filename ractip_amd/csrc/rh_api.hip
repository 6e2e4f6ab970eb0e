// rh_api.hip -- context, batch management and the C ABI of include/ractip_hot.h.
//
// Host side of the drop-in boundary.  One rh_ctx owns one
// GPU's streams, the score model in HBM and the DP tables of the current batch;
// tables are kept and reused across batches of equal or smaller shape (the z-score
// loop, the reference's src/ractip.cpp:1638-1657, shuffles preserve lengths).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "kernels.h"

using namespace rh;
using namespace rh::host;

// out[3p..3p+2] = F5i[n] of pair p's sequences idx[2p], idx[2p+1] and the duplex logZ of pair p
__global__ void collect_logz(const double* __restrict__ mc_logz, const int* __restrict__ idx, DxBatch D, double* __restrict__ out)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.np) return;
    out[3 * p + 0] = mc_logz[idx[2 * p]];
    out[3 * p + 1] = mc_logz[idx[2 * p + 1]];
    out[3 * p + 2] = D.logz[p];
}

static thread_local std::string g_create_error;

namespace rh::host {

int fail(rh_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

// grow-only device buffer
int ensure(rh_ctx* c, DevBuf& buf, size_t bytes, bool zero)
{
    if (bytes <= buf.cap && buf.p) return RH_OK;
    if (buf.p) { HIP_TRY(c, hipFree(buf.p)); buf.p = nullptr; buf.cap = 0; }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b) return fail(c, RH_ERR_OOM, "batch needs %zu MiB of HBM, %zu MiB free", bytes >> 20, free_b >> 20);
    HIP_TRY(c, hipMalloc(&buf.p, bytes));
    buf.cap = bytes;
    if (zero) HIP_TRY(c, hipMemset(buf.p, 0, bytes));
    return RH_OK;
}

}  // namespace rh::host

namespace {

std::string default_param_path()
{
    Dl_info info;
    if (dladdr((void*)&default_param_path, &info) && info.dli_fname) {
        std::string p(info.dli_fname);
        size_t k = p.find_last_of('/');
        p = (k == std::string::npos) ? std::string(".") : p.substr(0, k);
        return p + "/data/";
    }
    return "ractip_amd/data/";
}


// copy one sequence's posterior out of the (nmax-strided) device buffer
int fetch_bp(rh_ctx* c, int sq, double* out)
{
    const int n = c->n[sq];
    HIP_TRY(c, hipMemcpy(out, c->d_bp.as<const double>() + (size_t)sq * c->mc.tri_stride, sizeof(double) * tri_size(n),
                         hipMemcpyDeviceToHost));
    return RH_OK;
}
int fetch_up(rh_ctx* c, int sq, double* out)
{
    HIP_TRY(c, hipMemcpy(out, c->d_up.as<const double>() + (size_t)sq * c->mc.ld * c->max_w, sizeof(double) * c->n[sq] * c->max_w,
                         hipMemcpyDeviceToHost));
    return RH_OK;
}
int fetch_logz(rh_ctx* c, int sq, double* out)
{
    HIP_TRY(c, hipMemcpy(out, c->d_mclogz.as<const double>() + sq, sizeof(double), hipMemcpyDeviceToHost));
    return RH_OK;
}
int fetch_hp(rh_ctx* c, int p, double* out, double* logz)
{
    const int n1 = c->n[seq_of(c, p, 0)], n2 = c->n[seq_of(c, p, 1)];
    if (out)
        HIP_TRY(c, hipMemcpy2D(out, sizeof(double) * (n2 + 1), c->d_hp.as<const double>() + (size_t)p * c->dx.tab_stride,
                               sizeof(double) * c->dx.ldd, sizeof(double) * (n2 + 1), n1 + 1, hipMemcpyDeviceToHost));
    if (logz) HIP_TRY(c, hipMemcpy(logz, c->d_logz.as<const double>() + p, sizeof(double), hipMemcpyDeviceToHost));
    return RH_OK;
}

// ---- the environment switches, read once by create_ctx in this order (what each one selects: the field's comment in ctx.h)
enum EnvKind { ENV_INT, ENV_FLAG /* != 0 */, ENV_NOT /* == 0 */, ENV_4OR8 /* 4, anything else 8 */, ENV_DOUBLE };
struct EnvSwitch {
    const char* name;
    EnvKind kind;
    int Ctx::*field;
    double Ctx::*dfield = nullptr;
};
const EnvSwitch kEnvSwitches[] = {
    {"RH_LIN_W", ENV_INT, &Ctx::lin_w},        {"RH_LIN_W", ENV_INT, &Ctx::lin_w_in},   // both sweeps ...
    {"RH_LIN_W_IN", ENV_INT, &Ctx::lin_w_in},                                            // ... then the inside sweep alone
    {"RH_LIN_BS", ENV_INT, &Ctx::lin_bs},
    {"RH_NO_GRAPH", ENV_NOT, &Ctx::use_graphs},
    {"RH_FAR_MFMA", ENV_FLAG, &Ctx::far_mfma},
    {"RH_FAR_PK", ENV_FLAG, &Ctx::far_pk},
    {"RH_FAR_WAVE", ENV_FLAG, &Ctx::far_wave},
    {"RH_LOOKAHEAD", ENV_INT, &Ctx::lookahead},
    {"RH_STRIP", ENV_INT, &Ctx::strip},
    {"RH_STRIP_W", ENV_4OR8, &Ctx::strip_w},
    {"RH_STRIP_FILT", ENV_FLAG, &Ctx::strip_filt},
    {"RH_SMALL", ENV_FLAG, &Ctx::small_on},
    {"RH_FAR2", ENV_INT, &Ctx::far2},
    {"RH_STRIP_XCD", ENV_INT, &Ctx::strip_xcd},
    {"RH_F5_PASS", ENV_FLAG, &Ctx::f5_pass},
    {"RH_ACC_WIDE", ENV_INT, &Ctx::acc_wide},
    {"RH_ACC_FINAL_T", ENV_INT, &Ctx::acc_final_t},
    {"RH_CO_WINDOW", ENV_INT, &Ctx::co_window},
    {"RH_SCALE_LADDER", ENV_INT, &Ctx::scale_ladder},
    {"RH_SCALE_MEMORY", ENV_INT, &Ctx::scale_memory},
    {"RH_PAIR_HELPER", ENV_INT, &Ctx::pair_helper},
    {"RH_CO_SEED", ENV_INT, &Ctx::co_seed},
    {"RH_DX_W", ENV_INT, &Ctx::dx_w},
    {"RH_DX_QUAD", ENV_FLAG, &Ctx::dx_quad},
    {"RH_DX_STRIP", ENV_INT, &Ctx::dx_strip},
    {"RH_VDX_S", ENV_DOUBLE, nullptr, &Ctx::vdx_s},
};

}  // namespace

extern "C" {

static rh_ctx* create_ctx(int device, int model, const char* param_file, const char* defaults_file, int use_bl, int semantics);

rh_ctx* rh_create(int device, int model, const char* param_file) { return create_ctx(device, model, param_file, nullptr, 1, 0); }
rh_ctx* rh_create_vienna(int device, const char* defaults_file, int use_bl_param, const char* param_file, int semantics)
{
    return create_ctx(device, RH_MODEL_VIENNA_BL, param_file, defaults_file, use_bl_param, semantics);
}
int rh_vienna_semantics(const rh_ctx* c) { return c ? c->vienna_sem : RH_ERR_ARG; }

static rh_ctx* create_ctx(int device, int model, const char* param_file, const char* defaults_file, int use_bl, int semantics)
{
    if (model != RH_MODEL_CONTRAFOLD && model != RH_MODEL_VIENNA_BL) {
        fail(nullptr, RH_ERR_UNSUPPORTED, "unknown model %d", model);
        return nullptr;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        fail(nullptr, RH_ERR_HIP, "no HIP device available (%s): this library has no CPU fallback",
             e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        fail(nullptr, RH_ERR_ARG, "device %d out of range (have %d)", device, ndev);
        return nullptr;
    }
    ScoreModel host_model;
    ViennaDx* host_vienna = nullptr;
    char err[256];
    if (model == RH_MODEL_CONTRAFOLD) {
        const std::string path = param_file ? std::string(param_file) : default_param_path() + "contrafold_complementary.params";
        if (!load_score_model(path.c_str(), &host_model, err, sizeof err)) {
            fail(nullptr, RH_ERR_PARAM, "%s", err);
            return nullptr;
        }
    } else {
        const std::string bl = default_param_path() + "vienna_bl_star.params";
        host_vienna = new ViennaDx;
        if (!load_vienna_dx_ex(defaults_file, use_bl != 0, bl.c_str(), param_file, semantics, host_vienna, err, sizeof err)) {
            delete host_vienna;
            fail(nullptr, RH_ERR_PARAM, "%s", err);
            return nullptr;
        }
        std::memset(&host_model, 0, sizeof host_model);
    }
    rh_ctx* c = new rh_ctx;
    c->device = device; c->model = model;
    c->max_w = model == RH_MODEL_VIENNA_BL ? 15 : 1;   // RactIP's default --max-w (src/cmdline.c:151-186) / contrafold's width 1
    c->vienna_sem = host_vienna ? host_vienna->semantics : 0;
    if (c->vienna_sem == kViennaSem20) c->mode = RH_MODE_LOG;   // the scaled linear kernels hold the 1.8 semantics only (pf_duplex: rh_set_duplex_mode)
    // scale exponent of the linear fast path: log Z per nucleotide of typical sequences under this model
    // (random ACGU: 0.107..0.129 for n = 200..2000); deviations only cost dynamic range, never accuracy
    build_lin_model(host_model, 0.12, &c->lin0.h);
    c->h_score = new ScoreModel(host_model);
    // duplex: log Z per unit of (i + L2+1-j) is 0.62..0.82 on the bundled pairs, 0.645 for random sequences
    build_dx_lin_model(host_model, 0.65, &c->h_dxlin);
    for (const EnvSwitch& sw : kEnvSwitches) {
        const char* e = std::getenv(sw.name);
        if (!e) continue;
        switch (sw.kind) {
            case ENV_INT: c->*sw.field = std::atoi(e); break;
            case ENV_FLAG: c->*sw.field = std::atoi(e) != 0; break;
            case ENV_NOT: c->*sw.field = std::atoi(e) == 0; break;
            case ENV_4OR8: c->*sw.field = std::atoi(e) == 4 ? 4 : 8; break;
            case ENV_DOUBLE: c->*sw.dfield = std::atof(e); break;
        }
    }
    c->p_has_param = param_file != nullptr; if (param_file) c->p_param = param_file;
    c->p_has_defaults = defaults_file != nullptr; if (defaults_file) c->p_defaults = defaults_file;
    c->p_use_bl = use_bl; c->p_sem = semantics;
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&c->s_mc, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&c->s_dx, hipStreamNonBlocking) == hipSuccess &&
              c->d_model.upload(&host_model) == hipSuccess && c->lin0.d.upload(&c->lin0.h) == hipSuccess &&
              c->d_dxlin.upload(&c->h_dxlin) == hipSuccess;
    if (ok) {
        const std::vector<double> wT = strip_weights(c->lin0.h, &c->strip_filt_ok);
        ok = c->lin0.wT.upload(wT.data(), wT.size()) == hipSuccess;
    }
    if (ok && host_vienna) {
        VLinSet& v0 = c->vlin_m[0];
        v0.h = new VLinModel;
        // scale exponent: log Z per nucleotide of random ACGU under the BL* energies is 0.21..0.33 for n = 200..500 (up to 0.45 on the bundled RNAs)
        build_vlin_model(*host_vienna, 0.28, v0.h);
        // (RH_VLIN_S is not in the table: it also switches the scale-exponent ladder off, per compute())
        if (const char* e = std::getenv("RH_VLIN_S")) build_vlin_model(*host_vienna, std::atof(e), v0.h);
        ok = c->d_vienna.upload(host_vienna) == hipSuccess && v0.d.upload(v0.h) == hipSuccess;
        c->h_vlin = v0.h; c->d_vlin = v0.d;
        if (ok) {   // pf_duplex in scaled linear space: the loop tables at the duplex scale + its own end / mismatch weights
            VLinModel* tmp = new VLinModel;
            VDxLin hd;
            build_vlin_model(*host_vienna, c->vdx_s, tmp);
            build_vdx_lin(*host_vienna, c->vdx_s, &hd);
            ok = c->d_vdxl.upload(tmp) == hipSuccess && c->d_vdx.upload(&hd) == hipSuccess;
            delete tmp;
        }
    }
    c->h_vienna = host_vienna;   // (kept: the rung models of the scale-exponent ladder are built from it)
    for (int k = 0; ok && k < kEvCount; k++) ok = hipEventCreate(&c->ev[k]) == hipSuccess;
    if (!ok) {
        fail(nullptr, RH_ERR_HIP, "context setup failed: %s", hipGetErrorString(hipGetLastError()));
        rh_destroy(c);
        return nullptr;
    }
    return c;
}

void rh_destroy(rh_ctx* c)
{
    if (!c) return;
    if (c->helper) { rh_destroy(c->helper); c->helper = nullptr; }
    (void)hipSetDevice(c->device);
    for (GraphSlot* g : {&c->g_in, &c->g_out, &c->g_dx}) if (g->exec) (void)hipGraphExecDestroy(g->exec);
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->tev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->pack_ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->acc_ev) if (e) (void)hipEventDestroy(e);
    if (c->s_mc) (void)hipStreamDestroy(c->s_mc);
    if (c->s_dx) (void)hipStreamDestroy(c->s_dx);
    delete c;   // device buffers and host models go with their owners (ctx.h)
}

const char* rh_last_error(const rh_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

// the one-shot folds: check, stage one sequence, compute, fetch what the caller asked for
static int fold_one(rh_ctx* c, const char* seq, int n, const char* constraint, double* bp_tri, double* up, double* logZ)
{
    if (!c) return RH_ERR_ARG;
    BatchRequest r;
    r.ns = 1; r.seqs = &seq; r.lens = &n;
    r.with_mc = true;
    r.fold_cons = &constraint;
    int rc;
    std::string why;
    if ((rc = check_model(r, c->model == RH_MODEL_VIENNA_BL, &why))) return fail(c, rc, "%s", why.c_str());   // (answers before the sequence is looked at)
    if (!seq || n < 0) return fail(c, RH_ERR_ARG, "bad sequence");
    if (n == 0) { if (bp_tri) bp_tri[0] = 0.0; if (logZ) *logZ = 0.0; return RH_OK; }
    if ((rc = stage(c, r))) return rc;
    if ((rc = compute(c))) return rc;
    if (bp_tri && (rc = fetch_bp(c, 0, bp_tri))) return rc;
    if (up && (rc = fetch_up(c, 0, up))) return rc;
    if (logZ && (rc = fetch_logz(c, 0, logZ))) return rc;
    return RH_OK;
}

int rh_bpp(rh_ctx* c, const char* seq, int n, const char* constraint, double* bp_tri, double* logZ)
{
    return fold_one(c, seq, n, constraint, bp_tri, nullptr, logZ);
}

int rh_unpaired(rh_ctx* c, const char* seq, int n, int max_w, double* up)
{
    if (!c) return RH_ERR_ARG;
    if (!seq || n < 0 || !up) return fail(c, RH_ERR_ARG, "bad argument");
    if (n == 0) return RH_OK;
    const int rc = rh_set_max_w(c, max_w);
    return rc ? rc : fold_one(c, seq, n, nullptr, nullptr, up, nullptr);
}

int rh_fold(rh_ctx* c, const char* seq, int n, double* bp_tri, double* up, double* logZ)
{
    return fold_one(c, seq, n, nullptr, bp_tri, up, logZ);   // (takes no constraint: nothing to reject on the CONTRAfold model)
}

int rh_fold_constrained(rh_ctx* c, const char* seq, int n, const char* constraint, double* bp_tri, double* up, double* logZ)
{
    return fold_one(c, seq, n, constraint, bp_tri, up, logZ);
}

// the one-shot pair calls.  cofold: the two-molecule ensemble for this call only -- the context's hybridization mode is restored and
// the staged batch (which belongs to the other mode) invalidated on every path
static int pair_one(rh_ctx* c, bool cofold, const char* s1, int n1, const char* s2, int n2, const char* constraint, double* hp, double* logZ)
{
    if (!s1 || !s2 || n1 < 1 || n2 < 1) return fail(c, RH_ERR_ARG, "bad sequence");
    const char* seqs[2] = {s1, s2};
    const int lens[2] = {n1, n2};
    BatchRequest r;
    r.ns = 2; r.seqs = seqs; r.lens = lens;
    r.with_dx = true;
    r.joint_cons = &constraint;
    const int keep = c->hybrid;
    if (cofold) c->hybrid = RH_HYBRID_COFOLD;
    int rc = stage(c, r);
    if (!rc) rc = compute(c);
    if (!rc) rc = fetch_hp(c, 0, hp, logZ);
    if (cofold) { c->hybrid = keep; c->ns = 0; c->computed = false; }
    return rc;
}

int rh_duplex(rh_ctx* c, const char* s1, int n1, const char* s2, int n2, double* hp, double* logZ)
{
    if (!c) return RH_ERR_ARG;
    return pair_one(c, false, s1, n1, s2, n2, nullptr, hp, logZ);
}

int rh_cofold_constrained(rh_ctx* c, const char* s1, int n1, const char* s2, int n2, const char* constraint, double* hp, double* logZ)
{
    if (!c) return RH_ERR_ARG;
    if (c->model != RH_MODEL_VIENNA_BL) return fail(c, RH_ERR_UNSUPPORTED, "the two-molecule ensemble needs RH_MODEL_VIENNA_BL");
    return pair_one(c, true, s1, n1, s2, n2, constraint, hp, logZ);
}

int rh_batch_upload(rh_ctx* c, int npairs, const char* const* s1, const int* n1, const char* const* s2, const int* n2)
{
    return rh_batch_upload_constrained(c, npairs, s1, n1, s2, n2, nullptr, nullptr, nullptr);
}

int rh_batch_upload_constrained(rh_ctx* c, int npairs, const char* const* s1, const int* n1, const char* const* s2, const int* n2,
                                const char* const* cons1, const char* const* cons2, const char* const* co_cons)
{
    if (!c) return RH_ERR_ARG;
    if (npairs < 1 || !s1 || !s2 || !n1 || !n2) return fail(c, RH_ERR_ARG, "bad batch");
    std::vector<const char*> seqs(2 * (size_t)npairs), cons(2 * (size_t)npairs, nullptr);
    std::vector<int> lens(2 * (size_t)npairs);
    for (int p = 0; p < npairs; p++) {
        seqs[2 * p] = s1[p]; seqs[2 * p + 1] = s2[p];
        lens[2 * p] = n1[p]; lens[2 * p + 1] = n2[p];
        if (cons1) cons[2 * p] = cons1[p];
        if (cons2) cons[2 * p + 1] = cons2[p];
    }
    BatchRequest r;   // (constraint arrays whose entries are all NULL: the batch of rh_batch_upload)
    r.ns = 2 * npairs; r.seqs = seqs.data(); r.lens = lens.data();
    r.with_mc = r.with_dx = true;
    r.fold_cons = cons.data(); r.joint_cons = co_cons;
    return stage(c, r);
}

int rh_batch_upload_indexed(rh_ctx* c, int nseq, const char* const* seqs, const int* lens, int npairs, const int* first, const int* second)
{
    return rh_batch_upload_indexed_constrained(c, nseq, seqs, lens, npairs, first, second, nullptr, nullptr, nullptr);
}

int rh_batch_upload_indexed_constrained(rh_ctx* c, int nseq, const char* const* seqs, const int* lens, int npairs, const int* first, const int* second,
                                        const char* const* cons, const char* const* co_first, const char* const* co_second)
{
    if (!c) return RH_ERR_ARG;
    if (nseq < 1 || npairs < 1 || !seqs || !lens || !first || !second) return fail(c, RH_ERR_ARG, "bad indexed batch");
    BatchRequest r;   // (stage() checks every index and constraint before it changes the context)
    r.ns = nseq; r.seqs = seqs; r.lens = lens;
    r.with_mc = r.with_dx = true;
    r.fold_cons = cons;
    r.npairs = npairs; r.first = first; r.second = second;
    r.share_first = co_first; r.share_second = co_second;
    return stage(c, r);
}

int rh_batch_index(rh_ctx* c, int* nseq, int* npairs, int* first, int* second)
{
    if (!c) return RH_ERR_ARG;
    if (c->ns == 0 || !c->has_mc || !c->has_dx) return fail(c, RH_ERR_ARG, "no pair batch");
    if (nseq) *nseq = c->ns;
    if (npairs) *npairs = c->np;
    for (int p = 0; p < c->np; p++) {
        if (first) first[p] = seq_of(c, p, 0);
        if (second) second[p] = seq_of(c, p, 1);
    }
    return RH_OK;
}

int rh_debug_batch_allow_mask(rh_ctx* c, int which, int k, unsigned char* out, int* ld)
{
    if (!c) return RH_ERR_ARG;
    if (which != 0 && which != 1) return fail(c, RH_ERR_ARG, "rh_debug_batch_allow_mask: which = %d", which);
    const bool co = which == 1;
    if (c->ns == 0 || (co ? !c->has_dx : !c->has_mc)) return fail(c, RH_ERR_ARG, "no batch uploaded");
    const bool co_staged = c->model == RH_MODEL_VIENNA_BL && c->hybrid == RH_HYBRID_COFOLD;   // (otherwise c->co is not of this batch)
    if (k < 0 || k >= (co ? c->np : c->ns)) return fail(c, RH_ERR_ARG, "%s %d out of range", co ? "pair" : "sequence", k);
    const McBatch* B = co ? (co_staged ? &c->co : nullptr) : &c->mc;
    if (!B || !B->allow) return 1;
    if (ld) *ld = B->ld;
    if (out) HIP_TRY(c, hipMemcpy(out, B->allow + (size_t)k * B->ld * B->ld, (size_t)B->ld * B->ld, hipMemcpyDeviceToHost));
    return RH_OK;
}

int rh_batch_compute(rh_ctx* c)
{
    if (!c) return RH_ERR_ARG;
    if (c->ns == 0) return fail(c, RH_ERR_ARG, "no batch uploaded");
    return compute(c);
}

int rh_batch_results(rh_ctx* c, int p, double* bp1, double* bp2, double* up1, double* up2, double* hp, double* logZ3)
{
    if (!c) return RH_ERR_ARG;
    if (!c->computed || !c->has_mc || !c->has_dx) return fail(c, RH_ERR_ARG, "no computed pair batch");
    if (p < 0 || p >= c->np) return fail(c, RH_ERR_ARG, "pair %d out of range", p);
    int rc;
    const int sq1 = seq_of(c, p, 0), sq2 = seq_of(c, p, 1);
    if (bp1 && (rc = fetch_bp(c, sq1, bp1))) return rc;
    if (bp2 && (rc = fetch_bp(c, sq2, bp2))) return rc;
    if (up1 && (rc = fetch_up(c, sq1, up1))) return rc;
    if (up2 && (rc = fetch_up(c, sq2, up2))) return rc;
    if ((hp || logZ3) && (rc = fetch_hp(c, p, hp, logZ3 ? logZ3 + 2 : nullptr))) return rc;
    if (logZ3) {
        if ((rc = fetch_logz(c, sq1, logZ3))) return rc;
        if ((rc = fetch_logz(c, sq2, logZ3 + 1))) return rc;
    }
    return RH_OK;
}

int rh_batch_logz(rh_ctx* c, double* out)
{
    if (!c) return RH_ERR_ARG;
    if (!c->computed || !c->has_mc || !c->has_dx || !out) return fail(c, RH_ERR_ARG, "no computed pair batch");
    int rc;
    if ((rc = ensure(c, c->d_scal, sizeof(double) * 3 * c->np, false))) return rc;
    hipLaunchKernelGGL(collect_logz, dim3((c->np + 63) / 64), dim3(64), 0, c->s_mc, c->d_mclogz.as<const double>(), c->d_pidx.as<const int>(), c->dx, c->d_scal.as<double>());
    HIP_TRY(c, hipMemcpyAsync(out, c->d_scal.p, sizeof(double) * 3 * c->np, hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    return RH_OK;
}


int rh_batch_layout(rh_ctx* c, size_t* tri_stride, int* up_ld, size_t* hp_stride, int* hp_ld)
{
    if (!c) return RH_ERR_ARG;
    if (!c->has_mc || !c->has_dx) return fail(c, RH_ERR_ARG, "no pair batch");
    if (tri_stride) *tri_stride = c->mc.tri_stride;
    if (up_ld) *up_ld = c->mc.ld * c->max_w;
    if (hp_stride) *hp_stride = c->dx.tab_stride;
    if (hp_ld) *hp_ld = c->dx.ldd;
    return RH_OK;
}

int rh_batch_results_all(rh_ctx* c, double* bp, double* up, double* hp, double* logz)
{
    if (!c) return RH_ERR_ARG;
    if (!c->computed || !c->has_mc || !c->has_dx) return fail(c, RH_ERR_ARG, "no computed pair batch");
    HIP_TRY(c, hipSetDevice(c->device));
    if (bp) HIP_TRY(c, hipMemcpyAsync(bp, c->d_bp.p, sizeof(double) * c->mc.tri_stride * c->ns, hipMemcpyDeviceToHost, c->s_mc));
    if (up) HIP_TRY(c, hipMemcpyAsync(up, c->d_up.p, sizeof(double) * c->mc.ld * c->max_w * c->ns, hipMemcpyDeviceToHost, c->s_mc));
    if (hp) HIP_TRY(c, hipMemcpyAsync(hp, c->d_hp.p, sizeof(double) * c->dx.tab_stride * c->np, hipMemcpyDeviceToHost, c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    if (logz) return rh_batch_logz(c, logz);
    return RH_OK;
}

// the offsets of the packed float image of the staged batch (packed_layout, batch.h) in c->pack_off: bp_off, up_off, hp_off one behind
// the other, as the pack kernel reads them
static void packed_offsets(rh_ctx* c, size_t totals[3])
{
    c->pack_off.resize(2 * ((size_t)c->ns + 1) + c->np + 1);
    size_t* off = c->pack_off.data();
    packed_layout(c->ns, c->n.data(), c->np, c->pair_seq.data(), c->max_w, off, off + c->ns + 1, off + 2 * ((size_t)c->ns + 1), totals);
}

int rh_batch_packed_layout(rh_ctx* c, size_t* bp_off, size_t* up_off, size_t* hp_off, size_t totals[3])
{
    if (!c) return RH_ERR_ARG;
    if (c->ns == 0 || !c->has_mc || !c->has_dx) return fail(c, RH_ERR_ARG, "no pair batch");
    size_t tot[3];
    packed_offsets(c, tot);
    const size_t* off = c->pack_off.data();
    const size_t ns1 = (size_t)c->ns + 1;
    if (bp_off) std::copy(off, off + ns1, bp_off);
    if (up_off) std::copy(off + ns1, off + 2 * ns1, up_off);
    if (hp_off) std::copy(off + 2 * ns1, off + 2 * ns1 + c->np + 1, hp_off);
    if (totals) std::copy(tot, tot + 3, totals);
    return RH_OK;
}

int rh_batch_results_packed_f32(rh_ctx* c, float* bp, float* up, float* hp, double* logz)
{
    if (!c) return RH_ERR_ARG;
    if (!c->computed || !c->has_mc || !c->has_dx) return fail(c, RH_ERR_ARG, "no computed pair batch");
    HIP_TRY(c, hipSetDevice(c->device));
    c->pack_timed = false;
    if (bp || up || hp) {
        int rc;
        size_t tot[3];
        packed_offsets(c, tot);
        // the grid: a row of workgroups per block of the kinds asked for, as many as the largest block needs
        size_t largest = 0;
        for (int k = 0; k < c->ns; k++) largest = std::max(largest, std::max(bp ? tri_size(c->n[k]) : 0, up ? (size_t)c->n[k] * c->max_w : 0));
        for (int p = 0; hp && p < c->np; p++) largest = std::max(largest, ((size_t)c->n[seq_of(c, p, 0)] + 1) * ((size_t)c->n[seq_of(c, p, 1)] + 1));
        if (largest >= ((size_t)1 << 31)) return fail(c, RH_ERR_UNSUPPORTED, "a table of %zu entries is too large for the packed fetch", largest);
        const size_t blocks = (bp ? (size_t)c->ns : 0) + (up ? (size_t)c->ns : 0) + (hp ? (size_t)c->np : 0);
        if (blocks >= ((size_t)1 << 31)) return fail(c, RH_ERR_UNSUPPORTED, "%zu tables are too many for the packed fetch", blocks);
        const size_t per_wg = (size_t)kPackThreads * kPackGroupsPerThread * kPackAlign;
        const unsigned chunks = (unsigned)std::min<size_t>(65535, std::max<size_t>(1, (largest + per_wg - 1) / per_wg));
        // the staging buffer holds the images asked for, one behind the other (every total is a multiple of 16 bytes)
        const size_t at_up = bp ? tot[0] : 0, at_hp = at_up + (up ? tot[1] : 0), floats = at_hp + (hp ? tot[2] : 0);
        if ((rc = ensure(c, c->d_pack, sizeof(float) * floats, false))) return rc;
        if ((rc = ensure(c, c->d_packoff, sizeof(size_t) * c->pack_off.size(), false))) return rc;
        for (hipEvent_t& e : c->pack_ev) if (!e) HIP_TRY(c, hipEventCreate(&e));
        HIP_TRY(c, hipMemcpyAsync(c->d_packoff.p, c->pack_off.data(), sizeof(size_t) * c->pack_off.size(), hipMemcpyHostToDevice, c->s_mc));
        PackArgs A{};
        A.bp = bp ? c->d_bp.as<const double>() : nullptr;
        A.up = up ? c->d_up.as<const double>() : nullptr;
        A.hp = hp ? c->d_hp.as<const double>() : nullptr;
        A.n = c->d_n.as<const int>(); A.pn = c->d_pn.as<const int>();
        A.off = c->d_packoff.as<const size_t>();
        A.dst_bp = c->d_pack.as<float>(); A.dst_up = A.dst_bp + at_up; A.dst_hp = A.dst_bp + at_hp;
        A.tri_stride = c->mc.tri_stride; A.up_stride = (size_t)c->mc.ld * c->max_w; A.hp_stride = c->dx.tab_stride;
        A.nseq = c->ns; A.np = c->np; A.max_w = c->max_w; A.ldd = c->dx.ldd;
        HIP_TRY(c, hipEventRecord(c->pack_ev[0], c->s_mc));
        hipLaunchKernelGGL(pack_results_f32, dim3((unsigned)blocks, chunks), dim3(kPackThreads), 0, c->s_mc, A);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->pack_ev[1], c->s_mc));
        if (bp) HIP_TRY(c, hipMemcpyAsync(bp, A.dst_bp, sizeof(float) * tot[0], hipMemcpyDeviceToHost, c->s_mc));
        if (up) HIP_TRY(c, hipMemcpyAsync(up, A.dst_up, sizeof(float) * tot[1], hipMemcpyDeviceToHost, c->s_mc));
        if (hp) HIP_TRY(c, hipMemcpyAsync(hp, A.dst_hp, sizeof(float) * tot[2], hipMemcpyDeviceToHost, c->s_mc));
        HIP_TRY(c, hipStreamSynchronize(c->s_mc));
        c->pack_timed = true;
    }
    if (logz) return rh_batch_logz(c, logz);
    return RH_OK;
}

int rh_batch_pack_time(rh_ctx* c, double* ms)
{
    if (!c || !ms) return RH_ERR_ARG;
    if (!c->pack_timed) return fail(c, RH_ERR_ARG, "no packed fetch to time");
    float t = 0.f;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventElapsedTime(&t, c->pack_ev[0], c->pack_ev[1]));
    *ms = t;
    return RH_OK;
}

void* rh_host_alloc(rh_ctx* c, size_t bytes)
{
    if (!c || bytes == 0) return nullptr;
    void* p = nullptr;
    if (hipSetDevice(c->device) != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        fail(c, RH_ERR_OOM, "hipHostMalloc of %zu bytes failed", bytes);
        return nullptr;
    }
    return p;
}

void rh_host_free(rh_ctx* c, void* p)
{
    if (c && p) { (void)hipSetDevice(c->device); (void)hipHostFree(p); }
}

int rh_set_max_w(rh_ctx* c, int max_w)
{
    if (!c) return RH_ERR_ARG;
    if (max_w < 1 || max_w > 64) return fail(c, RH_ERR_ARG, "max_w=%d out of range [1,64]", max_w);
    if (c->model == RH_MODEL_CONTRAFOLD && max_w != 1 && !c->region_acc)
        return fail(c, RH_ERR_UNSUPPORTED, "max_w=%d: the CONTRAfold path has width-1 accessibility only (src/ractip.cpp:213-222) unless rh_set_region_accessibility is on", max_w);
    if (max_w != c->max_w) { c->max_w = max_w; c->computed = false; c->ns = 0; }   // buffers are sized at upload
    return RH_OK;
}
int rh_get_max_w(const rh_ctx* c) { return c ? c->max_w : RH_ERR_ARG; }

int rh_set_region_accessibility(rh_ctx* c, int on)
{
    if (!c) return RH_ERR_ARG;
    on = on != 0;
    if (c->model != RH_MODEL_CONTRAFOLD) return RH_OK;   // Vienna-BL computes every width already: accepted, nothing changes
    if (on == c->region_acc) return RH_OK;
    c->region_acc = on;
    if (!on && c->max_w != 1) { c->max_w = 1; c->computed = false; c->ns = 0; }   // back to the width the default path has
    return RH_OK;
}
int rh_get_region_accessibility(const rh_ctx* c) { return c ? c->region_acc : RH_ERR_ARG; }

int rh_batch_acc_time(rh_ctx* c, double* ms)
{
    if (!c || !ms) return RH_ERR_ARG;
    if (!c->computed || !c->acc_timed) return fail(c, RH_ERR_ARG, "no region accessibility phase to time");
    float t = 0.f;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventElapsedTime(&t, c->acc_ev[0], c->acc_ev[1]));
    *ms = t;
    return RH_OK;
}

int rh_set_hybrid(rh_ctx* c, int hybrid)
{
    if (!c) return RH_ERR_ARG;
    if (hybrid != RH_HYBRID_DUPLEX && hybrid != RH_HYBRID_COFOLD) return fail(c, RH_ERR_ARG, "unknown hybridization mode %d", hybrid);
    if (hybrid == RH_HYBRID_COFOLD && c->model != RH_MODEL_VIENNA_BL)
        return fail(c, RH_ERR_UNSUPPORTED, "the two-molecule (co_pf_fold) hybridization matrix needs RH_MODEL_VIENNA_BL");
    if (hybrid != c->hybrid) { c->hybrid = hybrid; c->computed = false; c->ns = 0; }
    return RH_OK;
}

int rh_set_mode(rh_ctx* c, int mode)
{
    if (!c) return RH_ERR_ARG;
    if (mode < RH_MODE_AUTO || mode > RH_MODE_LINEAR) return fail(c, RH_ERR_ARG, "unknown mode %d", mode);
    if (c->vienna_sem == kViennaSem20) {   // ViennaRNA-2.x semantics: log-space kernels only (AUTO means LOG)
        if (mode == RH_MODE_LINEAR) return fail(c, RH_ERR_UNSUPPORTED, "RH_VIENNA_SEM_20 runs on the log-space kernels only");
        c->mode = RH_MODE_LOG;
        return RH_OK;
    }
    c->mode = mode;
    return RH_OK;
}

int rh_set_duplex_mode(rh_ctx* c, int mode)
{
    if (!c) return RH_ERR_ARG;
    if (mode < RH_MODE_INHERIT || mode > RH_MODE_LINEAR) return fail(c, RH_ERR_ARG, "unknown duplex mode %d", mode);
    c->duplex_mode = mode;
    return RH_OK;
}
int rh_get_duplex_mode(const rh_ctx* c) { return c ? c->duplex_mode : RH_ERR_ARG; }

int rh_last_path(const rh_ctx* c) { return c ? c->last_path : RH_ERR_ARG; }
int rh_last_hybrid_path(const rh_ctx* c) { return c ? c->last_dx_path : RH_ERR_ARG; }

int rh_batch_kernels(rh_ctx* c, const char* fine[3], const char* far[3], int n_far[3])
{
    if (!c) return RH_ERR_ARG;
    if (!c->computed) return fail(c, RH_ERR_ARG, "no computed batch");
    // the plans of the linear first pass (run_attempt, compute.hip) where it stood; the fixed names of the log-space kernels where it did not
    const bool vienna = c->model == RH_MODEL_VIENNA_BL, lin = c->last_path == 1, dx_lin = c->last_dx_path == 1;
    const char* names[6] = {"", "", "", "", "", ""};
    if (c->has_mc) {
        names[0] = lin ? c->plan[0].fine : vienna ? "mcv_inside_diag" : "mc_inside_diag";
        names[1] = lin ? c->plan[1].fine : vienna ? "mcv_outside_diag" : "mc_outside_diag";
        if (lin && c->n_far[0]) names[3] = c->plan[0].far_name;
        if (lin && c->n_far[1]) names[4] = c->plan[1].far_name;
    }
    if (c->has_dx)
        names[2] = dx_lin ? c->plan[2].fine : !vienna ? "dx_sweep_diag" : c->hybrid == RH_HYBRID_COFOLD ? "mcv_inside_diag + mcv_outside_diag (s1+s2)" : "dxv_sweep_diag";
    for (int k = 0; k < 3; k++) {
        if (fine) fine[k] = names[k];
        if (far) far[k] = names[3 + k];
        if (n_far) n_far[k] = c->n_far[k];
    }
    return RH_OK;
}

int rh_batch_fallbacks(rh_ctx* c, int which, int* out, int cap)
{
    if (!c || which < 0 || which > 3) return RH_ERR_ARG;
    if (!c->computed) return fail(c, RH_ERR_ARG, "no computed batch");
    const std::vector<int>& F = which == 3 ? c->rescaled_dx : (which == 2 ? c->rescaled_mc : (which ? c->fallback_dx : c->fallback_mc));
    if (cap > 0 && !out) return fail(c, RH_ERR_ARG, "rh_batch_fallbacks: out is NULL with cap > 0");
    for (int k = 0; k < (int)F.size() && k < cap; k++) out[k] = F[k];
    return (int)F.size();
}

int rh_set_scale_memory(rh_ctx* c, int on)
{
    if (!c) return RH_ERR_ARG;
    c->scale_memory = on != 0;
    if (!on) { c->lin_primary = -1; c->vlin_primary = -1; }
    return RH_OK;
}

int rh_set_kernel_timing(rh_ctx* c, int cls)
{
    if (!c || cls < -1 || cls > 4) return RH_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (cls >= 0 && c->tev.empty()) {
        c->tev.resize(8192);
        for (auto& e : c->tev) HIP_TRY(c, hipEventCreate(&e));
    }
    c->time_cls = cls;
    c->tev_n = 0;
    return RH_OK;
}

int rh_kernel_times(rh_ctx* c, int* n_launches, double* total_ms)
{
    if (!c || !n_launches || !total_ms) return RH_ERR_ARG;
    if (!c->computed) return fail(c, RH_ERR_ARG, "no computed batch");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->s_mc));
    HIP_TRY(c, hipStreamSynchronize(c->s_dx));
    double tot = 0.0;
    for (size_t k = 0; k + 1 < c->tev_n; k += 2) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->tev[k], c->tev[k + 1]));
        tot += ms;
    }
    *n_launches = (int)(c->tev_n / 2);
    *total_ms = tot;
    return RH_OK;
}

int rh_set_overlap(rh_ctx* c, int on)
{
    if (!c) return RH_ERR_ARG;
    c->overlap = on != 0;
    return RH_OK;
}

int rh_batch_timings(rh_ctx* c, double ms[4], int n_launch[3])
{
    if (!c) return RH_ERR_ARG;
    if (!c->computed) return fail(c, RH_ERR_ARG, "no computed batch");
    if (ms) for (int k = 0; k < 4; k++) ms[k] = c->ms[k];
    if (n_launch) for (int k = 0; k < 3; k++) n_launch[k] = c->n_launch[k];
    return RH_OK;
}

int rh_batch_device_views(rh_ctx* c, const double** bp, size_t* tri_stride, const double** hp, size_t* hp_stride, int* hp_ld)
{
    if (!c) return RH_ERR_ARG;
    if (!c->computed) return fail(c, RH_ERR_ARG, "no computed batch");
    if (bp) *bp = c->d_bp.as<const double>();
    if (tri_stride) *tri_stride = c->mc.tri_stride;
    if (hp) *hp = c->d_hp.as<const double>();
    if (hp_stride) *hp_stride = c->dx.tab_stride;
    if (hp_ld) *hp_ld = c->dx.ldd;
    return RH_OK;
}

}  // extern "C"

// (alias of create_ctx for the per-pair helper context of fallbacks.hip; C++ linkage, not part of the C ABI)
rh_ctx* make_ctx_for_helper(int device, int model, const char* param_file, const char* defaults_file, int use_bl, int semantics)
{
    return create_ctx(device, model, param_file, defaults_file, use_bl, semantics);
}
