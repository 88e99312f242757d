// tnml_core.hip -- the context of the C-ABI (include/tnml.h): errors, profiling, the option table, the workspace plan,
// tnml_create / tnml_destroy, the small statistics getters and the host-side rules of the sweep.
//
// No CPU fallback lives here: every contraction is a HIP kernel launch on the context's stream.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>

#include "tnml_host.h"

static std::string g_create_err;

int tnml_fail(tnml_ctx* c, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) { c->err = buf; if (c->local && c->coll_depth > 0) local_comm_abort(c); } else g_create_err = buf;   // (inside a collective entry point the peers of an in-process communicator must not wait for a rank that has failed; an error of a local query leaves the communicator alone)
    return 1;
}
const char* tnml_last_error(const tnml_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }
const char* tnml_last_warning(const tnml_ctx* c) { return c ? c->warn.c_str() : ""; }

// ---- profiling ------------------------------------------------------------------------------
static hipEvent_t prof_event(tnml_ctx* c) {
    if (!c->prof_free.empty()) { hipEvent_t e = c->prof_free.back(); c->prof_free.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
void prof_begin(tnml_ctx* c, int, hipEvent_t* e0, hipStream_t st) { *e0 = prof_event(c); (void)hipEventRecord(*e0, st ? st : c->stream); }
void prof_end(tnml_ctx* c, int kc, hipEvent_t e0, hipStream_t st) {
    hipEvent_t e1 = prof_event(c); (void)hipEventRecord(e1, st ? st : c->stream);
    c->prof_pending.push_back({e0, e1, kc});
    if (c->prof_pending.size() > 8192) prof_resolve(c);
}
void prof_resolve(tnml_ctx* c) {
    if (c->prof_pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->prof_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) { c->prof_ms[p.kc] += ms; c->prof_launches[p.kc] += 1; }
        c->prof_free.push_back(p.e0); c->prof_free.push_back(p.e1);
    }
    c->prof_pending.clear();
}
int tnml_profile_enable(tnml_ctx* c, int on) { prof_resolve(c); c->prof = on != 0; return 0; }
int tnml_profile_select(tnml_ctx* c, const char* class_name) {
    prof_resolve(c);
    if (!class_name || !*class_name) { c->prof_mask = 0xffffffffu; return 0; }
    unsigned mask = 0;                                    // one class name, or several separated by commas
    const char* s = class_name;
    while (*s) {
        const char* e = strchr(s, ',');
        const size_t len = e ? (size_t)(e - s) : strlen(s);
        bool found = false;
        for (int i = 0; i < KC_COUNT; ++i) if (strlen(kclass_names[i]) == len && !strncmp(s, kclass_names[i], len)) { mask |= 1u << i; found = true; }
        if (!found) return tnml_fail(c, "tnml_profile_select: unknown kernel class in %s", class_name);
        s = e ? e + 1 : s + len;
    }
    c->prof_mask = mask;
    return 0;
}
int tnml_profile_count(tnml_ctx*) { return KC_COUNT; }
int tnml_profile_get(tnml_ctx* c, int idx, char* name64, int64_t* launches, double* total_ms) {
    if (idx < 0 || idx >= KC_COUNT) return tnml_fail(c, "profile index out of range");
    prof_resolve(c);
    if (name64) { strncpy(name64, kclass_names[idx], 63); name64[63] = 0; }
    if (launches) *launches = c->prof_launches[idx];
    if (total_ms) *total_ms = c->prof_ms[idx];
    return 0;
}
int tnml_profile_reset(tnml_ctx* c) {
    prof_resolve(c);
    for (int i = 0; i < KC_COUNT; ++i) { c->prof_launches[i] = 0; c->prof_ms[i] = 0.; }
    return 0;
}
// ---- context options ------------------------------------------------------------------------
// One row per option of tnml_set_option / tnml_set_option_real: its name, the environment variable that supplies its default at
// tnml_create (or none), the field it sets, its kind and the values it accepts.  A bool option takes any value (nonzero: on).
enum OptKind { OPT_BOOL, OPT_INT, OPT_REAL };
enum OptHook { HK_NONE, HK_REUSE_P, HK_DEFER_TAIL, HK_CHECK_REPLICAS, HK_ENV_BUDGET, HK_COMM_TIMEOUT, HK_FAIL_SPLIT, HK_MISPREDICT, HK_SVD_PRINT, HK_CG_METHOD, HK_NOISE, HK_PREDICT_TILE, HK_LOSS, HK_LOSS_BETA };
struct OptDef {
    const char* name; const char* env; OptKind kind;
    int tnml_ctx::* ifield; double tnml_ctx::* rfield;    // the field set (none for env_budget_mb: its hook stores bytes)
    double lo, hi; OptHook hook;
};
static const OptDef k_options[] = {
    {"fast_cg",          "TNML_FAST_CG",        OPT_BOOL, &tnml_ctx::fast_cg,             nullptr,          0, 1,       HK_NONE},
    {"reuse_p",          "TNML_REUSE_P",        OPT_BOOL, &tnml_ctx::reuse_p,             nullptr,          0, 1,       HK_REUSE_P},
    {"fuse_z",           "TNML_FUSE_Z",         OPT_BOOL, &tnml_ctx::fuse_z,              nullptr,          0, 1,       HK_NONE},
    {"merged_cg",        "TNML_MERGED_CG",      OPT_INT,  &tnml_ctx::merged_cg,           nullptr,          0, 2,       HK_NONE},
    {"defer_tail",       "TNML_DEFER_TAIL",     OPT_BOOL, &tnml_ctx::defer_tail,          nullptr,          0, 1,       HK_DEFER_TAIL},
    {"check_replicas",   "TNML_CHECK_REPLICAS", OPT_INT,  &tnml_ctx::check_replicas_mode, nullptr,          0, 2,       HK_CHECK_REPLICAS},
    {"fused_fwd",        "TNML_FUSED_FWD",      OPT_INT,  &tnml_ctx::fused_fwd,           nullptr,          0, INT_MAX, HK_NONE},   // > 2: always, with that many workgroups at most
    {"fwd_res",          "TNML_FWD_RES",        OPT_INT,  &tnml_ctx::fwd_res,             nullptr,          0, 3,       HK_NONE},   // 3: the general form on 120 x 120 bonds too
    {"shift_res",        "TNML_SHIFT_RES",      OPT_INT,  &tnml_ctx::shift_res,           nullptr,          0, 2,       HK_NONE},
    {"shift_skip",       "TNML_SHIFT_SKIP",     OPT_BOOL, &tnml_ctx::shift_skip,          nullptr,          0, 1,       HK_NONE},
    {"fwd_skip",         "TNML_FWD_SKIP",       OPT_BOOL, &tnml_ctx::fwd_skip,            nullptr,          0, 1,       HK_NONE},
    {"res_grid",         nullptr,               OPT_INT,  &tnml_ctx::res_grid,            nullptr,          0, INT_MAX, HK_NONE},
    {"res_pace",         "TNML_RES_PACE",       OPT_INT,  &tnml_ctx::res_pace,            nullptr,          0, 4,       HK_NONE},
    {"grad_quad",        "TNML_GRAD_QUAD",      OPT_INT,  &tnml_ctx::grad_quad,           nullptr,          0, 2,       HK_NONE},
    {"grad_pair",        "TNML_GRAD_PAIR",      OPT_BOOL, &tnml_ctx::grad_pair,           nullptr,          0, 1,       HK_NONE},
    {"bgemm_wgs",        "TNML_BGEMM_WGS",      OPT_INT,  &tnml_ctx::bgemm_wgs,           nullptr,          0, INT_MAX, HK_NONE},
    {"bgemm_per",        "TNML_BGEMM_PER",      OPT_INT,  &tnml_ctx::bgemm_per,           nullptr,          0, 1 << 20, HK_NONE},   // (x 32 images: stays an int)
    {"sytrd_exit",       nullptr,               OPT_BOOL, &tnml_ctx::sytrd_exit,          nullptr,          0, 1,       HK_NONE},
    {"bgs_chol",         "TNML_BGS_CHOL",       OPT_BOOL, &tnml_ctx::bgs_chol,            nullptr,          0, 1,       HK_NONE},
    {"spec_split",       "TNML_SPEC_SPLIT",     OPT_BOOL, &tnml_ctx::spec_split,          nullptr,          0, 1,       HK_NONE},
    {"debug_fail_split", nullptr,               OPT_INT,  &tnml_ctx::debug_fail_split,    nullptr,         -1, INT_MAX, HK_FAIL_SPLIT},
    {"spec_predict",     "TNML_SPEC_PREDICT",   OPT_BOOL, &tnml_ctx::spec_predict,        nullptr,          0, 1,       HK_NONE},
    {"debug_mispredict", nullptr,               OPT_INT,  &tnml_ctx::debug_mispredict,    nullptr,         -1, INT_MAX, HK_MISPREDICT},
    {"bf16_grad",        nullptr,               OPT_BOOL, &tnml_ctx::bf16_grad,           nullptr,          0, 1,       HK_NONE},
    {"bf16_once",        nullptr,               OPT_BOOL, &tnml_ctx::bf16_once,           nullptr,          0, 1,       HK_NONE},
    {"env_async",        nullptr,               OPT_BOOL, &tnml_ctx::env_async,           nullptr,          0, 1,       HK_NONE},
    {"env_budget_mb",    nullptr,               OPT_INT,  nullptr,                        nullptr,          0, INT_MAX, HK_ENV_BUDGET},
    {"comm_timeout_s",   nullptr,               OPT_INT,  &tnml_ctx::comm_timeout_s,      nullptr,          1, INT_MAX, HK_COMM_TIMEOUT},
    {"cg_method",        nullptr,               OPT_INT,  &tnml_ctx::cg_method,           nullptr,          0, 2,       HK_CG_METHOD},
    {"debug_nudge_rank", nullptr,               OPT_INT,  &tnml_ctx::debug_nudge_rank,    nullptr,         -1, INT_MAX, HK_NONE},
    {"mc_spin_max",      nullptr,               OPT_INT,  &tnml_ctx::mc_spin_max,         nullptr,         -1, INT_MAX, HK_NONE},
    {"svd_print",        "TNML_SVD_PRINT",      OPT_INT,  &tnml_ctx::svd_print,           nullptr,         -2, INT_MAX, HK_SVD_PRINT},
    {"predict_chunk",    nullptr,               OPT_INT,  &tnml_ctx::predict_chunk,       nullptr,          1, 1 << 20, HK_NONE},
    {"predict_tile",     nullptr,               OPT_INT,  &tnml_ctx::predict_tile,        nullptr,          0, 64,      HK_PREDICT_TILE},
    {"predict_dtype",    nullptr,               OPT_INT,  &tnml_ctx::predict_dtype,       nullptr,          0, 1,       HK_NONE},   // TNML_PREDICT_F64 / TNML_PREDICT_F32
    {"response_chunk",   nullptr,               OPT_INT,  &tnml_ctx::response_chunk,      nullptr,          1, 1 << 20, HK_NONE},
    {"gradient_chunk",   nullptr,               OPT_INT,  &tnml_ctx::gradient_chunk,      nullptr,          1, 1 << 20, HK_NONE},
    {"gradient_dtype",   nullptr,               OPT_INT,  &tnml_ctx::gradient_dtype,      nullptr,          0, 1,       HK_NONE},   // TNML_GRADIENT_F64 / TNML_GRADIENT_F32
    {"fg64_cfg",         "TNML_FG64_CFG",       OPT_INT,  &tnml_ctx::opt_fg64_cfg,        nullptr,          0, 2,       HK_NONE},
    {"ldot_cfg",         "TNML_LDOT_CFG",       OPT_INT,  &tnml_ctx::opt_ldot_cfg,        nullptr,          0, 2,       HK_NONE},
    {"loss",             nullptr,               OPT_INT,  &tnml_ctx::loss,                nullptr,          0, 1,       HK_LOSS},   // TNML_LOSS_QUADRATIC / TNML_LOSS_SOFTMAX
    {"loss_beta",        nullptr,               OPT_REAL, nullptr,                        &tnml_ctx::loss_beta, 0, HUGE_VAL, HK_LOSS_BETA},
    {"pcut",             nullptr,               OPT_REAL, nullptr,                        &tnml_ctx::pcut,  0, HUGE_VAL, HK_NONE},
    {"noise",            nullptr,               OPT_REAL, nullptr,                        &tnml_ctx::noise, 0, HUGE_VAL, HK_NOISE},
};
// checks v against the row, then the option's own refusals and side effects, then sets the field; `who` and `what` name the caller
// and the option (or the environment variable) in a message
static int apply_option(tnml_ctx* c, const OptDef& d, double v, const char* who, const char* what) {
    if (d.kind != OPT_BOOL && !(v >= d.lo && v <= d.hi)) {
        if (d.hi >= INT_MAX) return tnml_fail(c, "%s: %s = %.15g, must be >= %.15g", who, what, v, d.lo);
        return tnml_fail(c, "%s: %s = %.15g, must be in %.15g..%.15g", who, what, v, d.lo, d.hi);
    }
    switch (d.hook) {
        case HK_NONE: break;
        case HK_REUSE_P: c->p_valid = false; break;
        case HK_DEFER_TAIL: if (c->pend_count) return tnml_fail(c, "defer_tail: a bond update is in flight"); break;
        case HK_CHECK_REPLICAS: c->check_replicas = v != 0; break;
        case HK_ENV_BUDGET: c->env_budget_bytes = (long)v << 20; break;
        case HK_COMM_TIMEOUT: local_comm_set_timeout(c, (int)v); break;
        case HK_FAIL_SPLIT: c->spec_splits = 0; break;
        case HK_MISPREDICT: c->pred_splits = 0; break;
        case HK_SVD_PRINT: c->svd_calls = 0; break;
        case HK_CG_METHOD:
            if (v >= 1 && !c->single()) return tnml_fail(c, "cg_method: 0 (conj) or, in TNML_MODE_SINGLE, 1 (fast_conj) / 2 (exact)");
            break;
        case HK_PREDICT_TILE:
            if (v != 0 && v != 16 && v != 32 && v != 64) return tnml_fail(c, "%s: %s = %.15g, must be 0, 16, 32 or 64", who, what, v);
            break;
        case HK_LOSS:
            if (v >= 1 && c->single()) return tnml_fail(c, "loss: 0 (quadratic) in TNML_MODE_SINGLE: one output has no softmax");
            break;
        case HK_LOSS_BETA:                                             // (NaN has failed the range check above)
            if (!(v > 0 && std::isfinite(v))) return tnml_fail(c, "%s: %s = %.15g, must be finite and > 0", who, what, v);
            break;
        case HK_NOISE:                                                 // single.cc:25,222: the noise of every sweep
            if (v >= 1e-14 && !c->single()) return tnml_fail(c, "noise: the density-matrix split exists in the per-label variant only (single.h:648-672)");
            if (v >= 1e-14 && !c->env64()) return tnml_fail(c, "noise: needs fp64 environments (dtype f64)");
            break;
    }
    if (d.ifield) c->*d.ifield = d.kind == OPT_BOOL ? v != 0 : (int)v;
    if (d.rfield) c->*d.rfield = v;
    return 0;
}
static int set_option(tnml_ctx* c, const char* who, const char* name, double v, bool real) {
    if (!c || !name) return tnml_fail(c, "%s: null argument", who);
    for (const OptDef& d : k_options)
        if ((d.kind == OPT_REAL) == real && !strcmp(d.name, name)) return apply_option(c, d, v, who, name);
    return tnml_fail(c, "%s: unknown option %s", who, name);
}
int tnml_set_option(tnml_ctx* c, const char* name, int value) { return set_option(c, "tnml_set_option", name, value, false); }
int tnml_set_option_real(tnml_ctx* c, const char* name, double value) { return set_option(c, "tnml_set_option_real", name, value, true); }
int tnml_synchronize(tnml_ctx* c) { HIPCK(c, hipStreamSynchronize(c->stream)); if (c->copy_stream) HIPCK(c, hipStreamSynchronize(c->copy_stream)); return ipc_comm_check(c); }
int64_t tnml_device_bytes(tnml_ctx* c) { return c->bytes; }
int64_t tnml_replica_repairs(tnml_ctx* c) { return c->replica_repairs; }
// resolves the event pairs of the roll-backs that have finished (call after tnml_synchronize for the full sum)
static void resolve_redo_events(std::vector<std::pair<hipEvent_t, hipEvent_t>>& ev, double* sum_ms) {
    for (size_t k = 0; k < ev.size();) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[k].first, ev[k].second) == hipSuccess) {
            *sum_ms += ms;
            (void)hipEventDestroy(ev[k].first); (void)hipEventDestroy(ev[k].second);
            ev.erase(ev.begin() + k);
        } else { (void)hipGetLastError(); ++k; }
    }
}
int tnml_spec_predict_stats(tnml_ctx* c, int64_t* predicted, int64_t* mispredicted, double* redo_ms) {
    if (!c) return tnml_fail(c, "tnml_spec_predict_stats: null argument");
    resolve_redo_events(c->pred_redo_events, &c->pred_redo_ms);
    if (predicted) *predicted = c->pred_splits_total;
    if (mispredicted) *mispredicted = c->mispredicted;
    if (redo_ms) *redo_ms = c->pred_redo_ms;
    return 0;
}
int tnml_truncate_device(tnml_ctx* c, const double* evals_ascending, int n, int maxm, int minm, double cutoff, int m_pred, int* m, int* wrong) {
    if (!c || !evals_ascending || !m || !wrong) return tnml_fail(c, "tnml_truncate_device: null argument");
    if (n < 1 || n > (1 << 20)) return tnml_fail(c, "tnml_truncate_device: n = %d, must be in 1..%d", n, 1 << 20);
    if (c->pend_count > 0) return tnml_fail(c, "tnml_truncate_device: a bond update is in flight (tnml_bond_update_end first)");
    HIPCK(c, hipSetDevice(c->cfg.device));
    double* d = nullptr;                                                // a test entry: its own buffer, [n eigenvalues | count | verdict | carried word]
    HIPCK(c, hipMalloc((void**)&d, sizeof(double) * ((size_t)n + 3)));
    double out[3] = {-1., -1., -1.};
    int rc = 0;
    if (hipMemcpyAsync(d, evals_ascending, sizeof(double) * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = tnml_fail(c, "tnml_truncate_device: copy to the device failed");
    if (!rc) rc = launch_truncate_verdict(c, d, n, maxm, minm, cutoff, m_pred, d + n, d + n + 2);
    if (!rc && hipMemcpyAsync(out, d + n, sizeof out, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = tnml_fail(c, "tnml_truncate_device: copy from the device failed");
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = tnml_fail(c, "tnml_truncate_device: the kernel failed");
    (void)hipFree(d);
    if (rc) return rc;
    if (out[1] != out[2]) return tnml_fail(c, "tnml_truncate_device: the mirrored verdict %g differs from the carried word %g", out[1], out[2]);
    *m = (int)out[0]; *wrong = out[1] != 0. ? 1 : 0;
    return 0;
}
int tnml_split_stats(tnml_ctx* c, int64_t* spec_splits, int64_t* roll_backs, double* roll_back_ms) {
    resolve_redo_events(c->redo_events, &c->redo_ms);
    resolve_redo_events(c->pred_redo_events, &c->pred_redo_ms);       // mispredictions are roll-backs too (tnml_spec_predict_stats reports them apart)
    if (spec_splits) *spec_splits = c->spec_splits_total;
    if (roll_backs) *roll_backs = c->spec_redos;
    if (roll_back_ms) *roll_back_ms = c->redo_ms + c->pred_redo_ms;
    return 0;
}
int tnml_svd_stats(tnml_ctx* c, int64_t* fallbacks, int64_t* cluster_repairs, double* d0, double* d1) {
    if (fallbacks) *fallbacks = c->svd_fallbacks;
    if (cluster_repairs) *cluster_repairs = c->svd_cholqr;
    if (d0) *d0 = c->svd_last_dev0;
    if (d1) *d1 = c->svd_last_dev1;
    return 0;
}

// ---- host-side rules ------------------------------------------------------------------------
// ITensor v2 truncate() as recalled in SURVEY.md 8(a9): always cut to maxm; then with
// scale = sum(p) (DoRelCutoff) discard while (discarded + p_n) < cutoff*scale and kept > minm.
int tnml_truncate(const double* P, int origm, int maxm, int minm, double cutoff, double* truncerr) {
    if (origm <= 1) { if (truncerr) *truncerr = 0.; return origm; }
    int n = origm - 1;
    double te = 0.;
    while (n >= maxm) { te += P[n]; --n; }
    double scale = 0.;
    for (int j = 0; j < origm; ++j) scale += P[j];
    if (scale == 0.) scale = 1.;
    while (n >= 0 && te + P[n] < cutoff * scale && n >= minm) { te += P[n]; --n; }
    if (n < 0) n = 0;
    if (truncerr) *truncerr = te / scale;
    return n + 1;
}
// ITensor sweepnext: b = 1..N-1 (ha=1) then N-1..1 (ha=2); ha==3 ends the sweep
void tnml_sweepnext(int* b, int* ha, int N) {
    const int inc = (*ha == 1) ? +1 : -1;
    *b += inc;
    if (*b == ((*ha == 1) ? N : 0)) { *b -= inc; ++*ha; }
}
// ParallelDo's static chunking (paralleldo.h:32-43) with ranks in place of threads: equal chunks,
// the last rank takes the remainder
void tnml_shard_bounds(int64_t NT_total, int nranks, int rank, int64_t* begin, int64_t* end) {
    const int64_t th = NT_total / nranks;
    *begin = th * rank;
    *end = (rank == nranks - 1) ? NT_total : th * (rank + 1);
}

// ---- workspace plan -------------------------------------------------------------------------
// the dimensions and workspace sizes a configuration implies, and the shape of the site-tensor sets (tnml_create, tnml_estimate_bytes)
static void ctx_plan(tnml_ctx* c, const tnml_config& cfg) {
    c->cfg = cfg;
    c->N = cfg.N; c->NT = cfg.NT_local; c->maxm = cfg.maxm;
    c->c0 = cfg.mode == TNML_MODE_SINGLE ? -1 : cfg.N / 2;      // fixedL.cc:616; no Label site in the per-label variant
    c->NTp = (cfg.NT_local + TNML_NTPAD - 1) / TNML_NTPAD * TNML_NTPAD;
    const size_t NTp = c->NTp, m = c->maxm;
    const int Kmax = c->bf16() ? (2 * c->maxm + 31) / 32 * 32 : ru16(2 * c->maxm);
    c->mcap = (size_t)TNML_NL * Kmax * Kmax;
    c->small_elems = m * NTp;
    c->big_elems = TNML_NL * m * NTp;
    c->svd_n = 2 * c->maxm;
    c->slab_bytes = (size_t)128 * Kmax * Kmax * 4 * (c->f64() ? 2 : 1);
    c->partial_cap = (int)(NTp / 64);
    // sM holds (a) the Label-permuted bond matrix of the split, 40 maxm^2, and (b) the 16-padded site matrix of an
    // environment shift, L * ru16(2 m) * ru16(m) -- at small maxm the padding of (b) dominates
    c->sM_cap = std::max(40 * m * m, (size_t)TNML_NL * Kmax * ru16(c->maxm));
    c->ebt_cap = c->bf16() ? bf16e_env_elems(c->maxm, c->NTp, c->bf16() == 2) : 0;   // bf16 copies of the forward pass's operands (kernels_bf16e.hip)
    c->mbt_cap = c->bf16() ? bf16e_m_elems(c->maxm, c->bf16() == 2) : 0;
    c->W.resize(c->N + 2);
    c->env.resize(c->N + 2);
    c->bond_hist.assign(c->N + 1, tnml_ctx::BondHist());
    // speculative split: spare site tensors (two bond updates in flight replace two sites each; the Label site has its own size class)
    c->spare_small.assign(4, nullptr);
    c->spare_big.assign(c->c0 > 0 ? 2 : 0, nullptr);
}
// Every device buffer tnml_create allocates, in its order: the slot, its bytes, whether this configuration has it, and whether it is a
// site tensor (W and the spares trade buffers during speculative splits: tnml_destroy frees those by their own rule)
struct DevBuf { void** slot; size_t bytes; bool on, site; };
static std::vector<DevBuf> device_buffers(tnml_ctx* c) {
    const size_t NTp = c->NTp, m = c->maxm, n = c->svd_n, esz = c->esz(), eesz = c->eesz(), D = sizeof(double);
    std::vector<DevBuf> v;
    auto add = [&](auto& p, size_t bytes, bool on = true) { v.push_back({(void**)&p, bytes, on, false}); };
    add(c->phi, c->N * 2 * NTp * eesz); add(c->label, NTp * sizeof(int)); add(c->ones, NTp * eesz);
    add(c->U, c->big_elems * esz); add(c->P, TNML_NL * NTp * esz); add(c->dP, TNML_NL * NTp * esz); add(c->Pp, TNML_NL * NTp * esz);
    add(c->Zp, c->small_elems * esz); add(c->Mf, c->mcap * sizeof(float)); add(c->slab, c->slab_bytes);
    add(c->partials, c->partial_cap * 12 * D); add(c->partials2, c->partial_cap * 12 * D); add(c->counters, 16 * sizeof(unsigned));
    add(c->Ppart, 2 * TNML_NL * NTp * D, c->cfg.dtype == TNML_F64 && c->cfg.mode == TNML_MODE_FIXEDL && m >= 33);   // k_fwd_res (input dimensions 33..120)
    // tile order tables of k_shift_res (input dimensions 33..120, fp64-stored environments): one byte per site and image, one per site and 64-image tile
    const bool zs = c->cfg.dtype == TNML_F64 && c->cfg.mode == TNML_MODE_FIXEDL && m >= 33;
    add(c->zs_ord, c->N * NTp, zs); add(c->zs_nz, c->N * (NTp / 64), zs); add(c->zs_cnt, c->N * sizeof(int), zs);
    add(c->zf_ord, c->N * NTp, zs); add(c->zf_cnt, c->N * sizeof(int), zs);        // the order table of k_fwd_res's 32-image tiles: one byte per site and image
    add(c->ebt, c->ebt_cap * sizeof(unsigned short), c->bf16() != 0); add(c->mbt, c->mbt_cap * sizeof(unsigned short), c->bf16() != 0);
    add(c->vB, c->mcap * D); add(c->vR, c->mcap * D); add(c->vP, c->mcap * D); add(c->arbuf, (c->mcap + TNML_TAILN) * D); add(c->locals, 32 * D);
    add(c->scal, (SC_N + 4 * TNML_MAX_PASS) * D);      // CG scalars, then the per-pass trace: one copy to the host
    add(c->vpart, (1024 + 16) * D);     // [256][2] phase-1 partials, then [256][2] for |p|^2 of the next pass, then the summed cost of an output update
    add(c->tB, c->mcap * D); add(c->tB2, c->mcap * D);
    add(c->sM, c->sM_cap * D); add(c->sG, n * n * D); add(c->sD, n * D); add(c->sE, 2 * n * D); add(c->sF, (n * m + 2 * TNML_NL * m * m) * D);
    add(c->sInfo, 4 * sizeof(int)); add(c->fprint, 2 * sizeof(unsigned long long));
    add(c->sE2, n * D); add(c->sTau, n * D); add(c->sV, n * n * D); add(c->sC, n * n * D);
    add(c->sW, (n + 8) * D);            // + room for the orthogonality check values behind the eigenvalues
    add(c->sScr, std::max<size_t>(5 * n * m, TEIG_SCRATCH_DOUBLES) * D); add(c->sS, m * m * D); add(c->sCm, m * m * D); add(c->sQ1, n * m * D); add(c->sDev, 4 * D);
    add(c->mc_xbuf, eigh_mc_xbuf_bytes(), n > 240);                  // multi-workgroup tridiagonalisation (eigh_mc.hip)
    for (int j = 1; j <= c->N; ++j) v.push_back({(void**)&c->W[j].a, 2 * m * m * (j == c->c0 ? TNML_NL : 1) * D, true, true});   // the W replica
    for (auto& p : c->spare_small) v.push_back({(void**)&p, 2 * m * m * D, true, true});
    for (auto& p : c->spare_big) v.push_back({(void**)&p, 2 * m * m * TNML_NL * D, true, true});
    return v;
}
int dalloc(tnml_ctx* c, void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return tnml_fail(c, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    c->bytes += (int64_t)bytes;
    return 0;
}
int ctx_alloc_doubles(tnml_ctx* c, double** p, size_t n) { return dalloc(c, (void**)p, (n ? n : 1) * sizeof(double)); }

// Device memory a context of this configuration will own once a sweep has touched every environment: the buffers of tnml_create
// plus what is allocated on first use.
int64_t tnml_estimate_bytes(const tnml_config* cfg) {
    if (!cfg || cfg->N < 1 || cfg->NT_local < 1 || cfg->maxm < 1) return -1;
    tnml_ctx t;
    ctx_plan(&t, *cfg);
    double b = 0.;
    for (const DevBuf& d : device_buffers(&t)) if (d.on) b += (double)d.bytes;
    const double m = t.maxm, NTp = t.NTp;
    // the environment slabs (about N/2 Label-carrying + N/2 Label-free environments at any time = 0.55 N slabs
    // of 10*maxm*NTp elements, + the three chain buffers of tnml_classify; the per-label variant: N Label-free environments, 10 per slab)
    const double nslab = t.single() ? (t.N / 10. + 2.) : (0.55 * t.N + 3.);
    b += nslab * TNML_NL * m * NTp * t.eesz();
    if (t.single()) b += 8. * (5. * m * NTp + 3. * NTp + 3. * m * m);       // noise_ws: the workspace of the noise split (svd.hip, first use with noise > 0)
    return (int64_t)b;
}
int tnml_device_memory(int device, int64_t* free_bytes, int64_t* total_bytes) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return tnml_fail(nullptr, "tnml_device_memory: no HIP device %d", device);
    int cur = 0; (void)hipGetDevice(&cur);
    size_t f = 0, t = 0;
    if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&f, &t) != hipSuccess) return tnml_fail(nullptr, "tnml_device_memory: hipMemGetInfo failed");
    (void)hipSetDevice(cur);
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return 0;
}
// Largest bond dimension <= wanted (and >= floor_m) whose context fits into budget_bytes; also bounded by what an MPS of
// N sites can reach at all: min over the two sides of a bond of the full dimension, 2^j and 10*2^(N-j).
int tnml_plan_maxm(const tnml_config* cfg, int wanted, int floor_m, int64_t budget_bytes) {
    if (!cfg || wanted < 1) return -1;
    long reach = 1;
    for (int j = 1; j < cfg->N; ++j) {
        const int l = j, r = cfg->N - j;
        const double dl = l >= 40 ? 1e12 : (double)(1L << l) * (cfg->mode == TNML_MODE_SINGLE ? 1 : TNML_NL);   // the Label index may sit on either side
        const double dr = r >= 40 ? 1e12 : (double)(1L << r) * (cfg->mode == TNML_MODE_SINGLE ? 1 : TNML_NL);
        const double d = dl < dr ? dl : dr;
        if (d > reach) reach = d > 1e9 ? 1000000000L : (long)d;
    }
    int hi = wanted < reach ? wanted : (int)reach;
    if (hi < floor_m) hi = floor_m;
    tnml_config t = *cfg;
    t.maxm = hi;
    if (budget_bytes <= 0 || tnml_estimate_bytes(&t) <= budget_bytes) return hi;
    int lo = floor_m < 1 ? 1 : floor_m;
    t.maxm = lo;
    if (tnml_estimate_bytes(&t) > budget_bytes) return lo;      // even the floor does not fit: let tnml_create report it
    while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; t.maxm = mid; if (tnml_estimate_bytes(&t) <= budget_bytes) lo = mid; else hi = mid; }
    return lo;
}

int tnml_create(tnml_ctx** out, const tnml_config* cfg) {
    if (!out || !cfg) return tnml_fail(nullptr, "tnml_create: null argument");
    *out = nullptr;
    if (cfg->N < 4) return tnml_fail(nullptr, "tnml_create: need N >= 4 sites");
    if (cfg->NT_local < 1 || cfg->maxm < 1) return tnml_fail(nullptr, "tnml_create: NT_local and maxm must be positive");
    if (cfg->dtype < TNML_F32 || cfg->dtype > TNML_BF16X3) return tnml_fail(nullptr, "tnml_create: dtype must be TNML_F64, TNML_F64_E32, TNML_F32, TNML_BF16 or TNML_BF16X3");
    if (cfg->nranks < 1 || cfg->rank < 0 || cfg->rank >= cfg->nranks) return tnml_fail(nullptr, "tnml_create: bad rank/nranks");
    if (cfg->mode != TNML_MODE_FIXEDL && cfg->mode != TNML_MODE_SINGLE) return tnml_fail(nullptr, "tnml_create: mode must be TNML_MODE_FIXEDL or TNML_MODE_SINGLE");
    if (cfg->mode == TNML_MODE_SINGLE && (cfg->target_label < 0 || cfg->target_label >= TNML_NL)) return tnml_fail(nullptr, "tnml_create: target_label must be in 0..9");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return tnml_fail(nullptr, "tnml_create: no HIP device available (the HIP path is the only path; there is no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return tnml_fail(nullptr, "tnml_create: device %d out of range (%d visible)", cfg->device, ndev);
    if (hipSetDevice(cfg->device) != hipSuccess) return tnml_fail(nullptr, "tnml_create: hipSetDevice failed");
    tnml_ctx* c = new tnml_ctx();
    ctx_plan(c, *cfg);
    int rc = 0;
    auto bail = [&](int r) { g_create_err = c->err; tnml_destroy(c); return r; };
    for (const OptDef& d : k_options)                         // the environment's defaults of the options
        if (const char* e = d.env ? getenv(d.env) : nullptr)
            if ((rc = apply_option(c, d, atoi(e), "tnml_create", d.env))) return bail(rc);
    if (const char* e = getenv("TNML_SVD_BACKEND")) c->cfg.svd_backend = atoi(e);
    if (const char* e = getenv("TNML_SVD_DUMP")) c->svd_dump = e;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(tnml_fail(c, "hipStreamCreate failed"));
    if (rocblas_create_handle(&c->blas) != rocblas_status_success) return bail(tnml_fail(c, "rocblas_create_handle failed"));
    rocblas_set_stream(c->blas, c->stream);
    // replicas of W must stay bit-identical over the ranks: no atomics-based split-K inside rocBLAS
    rocblas_set_atomics_mode(c->blas, rocblas_atomics_not_allowed);
    for (const DevBuf& d : device_buffers(c))
        if (d.on && (rc = dalloc(c, d.slot, d.bytes))) return bail(rc);
    c->tail = c->arbuf; c->vG = c->arbuf + TNML_TAILN;
    c->cgtrace = c->scal + SC_N;
    for (int k = 0; k < 2; ++k)
        if (hipEventCreateWithFlags(&c->pend[k].ev, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->pend[k].ev2, hipEventDisableTiming) != hipSuccess)
            return bail(tnml_fail(c, "hipEventCreate failed"));
    if (hipHostMalloc((void**)&c->h_scal, sizeof(double) * hscal_doubles(c)) != hipSuccess) return bail(tnml_fail(c, "hipHostMalloc failed"));
    // speculative split: pinned mirrors [eigenvalues + check words | CG scalars + trace | ...] per bond update in flight (the layout: tnml_host.h)
    c->hrep_stride = hrep_slot_doubles(c);
    if (hipHostMalloc((void**)&c->hrep, sizeof(double) * 2 * c->hrep_stride) != hipSuccess) return bail(tnml_fail(c, "hipHostMalloc failed"));
    if (hipHostMalloc((void**)&c->hcost, sizeof(double) * 2 * (size_t)c->partial_cap * 12) != hipSuccess) return bail(tnml_fail(c, "hipHostMalloc failed"));
    memset(c->hrep, 0, sizeof(double) * 2 * c->hrep_stride);
    if (hipMemsetAsync(c->counters, 0, 16 * sizeof(unsigned), c->stream) != hipSuccess ||
        (c->mc_xbuf && hipMemsetAsync(c->mc_xbuf, 0, eigh_mc_xbuf_bytes(), c->stream) != hipSuccess) ||
        hipMemsetAsync(c->arbuf, 0, sizeof(double) * (c->mcap + TNML_TAILN), c->stream) != hipSuccess ||
        hipMemsetAsync(c->locals, 0, sizeof(double) * 32, c->stream) != hipSuccess ||
        hipMemsetAsync(c->scal, 0, sizeof(double) * SC_N, c->stream) != hipSuccess) return bail(tnml_fail(c, "memset failed"));
    if ((rc = c->env64() ? launch_fill_f64(c, (double*)c->ones, 1.0, c->NTp) : launch_fill_f32(c, (float*)c->ones, 1.0f, c->NTp))) return bail(rc);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return bail(tnml_fail(c, "sync failed"));
    *out = c;
    return 0;
}

int tnml_destroy(tnml_ctx* c) {
    if (!c) return 0;
    if (c->ho) heldout_release(c);                        // either context of a held-out pair: detach first
    if (c->held) heldout_release(c->held->train);
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) ncclCommDestroy(c->comm);
    local_comm_release(c);
    ipc_comm_release(c);
    for (int k = 0; k < 2; ++k) { if (c->pend[k].ev) (void)hipEventDestroy(c->pend[k].ev); if (c->pend[k].ev2) (void)hipEventDestroy(c->pend[k].ev2); if (c->pend[k].ev_ho) (void)hipEventDestroy(c->pend[k].ev_ho); }
    for (auto& p : c->prof_pending) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
    for (auto e : c->prof_free) (void)hipEventDestroy(e);
    for (auto& p : c->redo_events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto& p : c->pred_redo_events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (const DevBuf& d : device_buffers(c)) if (!d.site && *d.slot) (void)hipFree(*d.slot);
    // (site tensors and spares have changed places during speculative splits: every buffer is in exactly one of the two sets,
    // or held by the undo record of a bond update in flight)
    for (auto& s : c->W) if (s.a) (void)hipFree(s.a);
    for (size_t k = 0; k < c->spare_small.size(); ++k) if (c->spare_small[k]) (void)hipFree(c->spare_small[k]);
    for (size_t k = 0; k < c->spare_big.size(); ++k) if (c->spare_big[k]) (void)hipFree(c->spare_big[k]);
    for (int k = 0; k < 2; ++k) for (int u = 0; u < c->pend[k].nundo; ++u) if (c->pend[k].undo[u].old) (void)hipFree(c->pend[k].undo[u].old);
    if (c->noise_ws) (void)hipFree(c->noise_ws);          // allocated on first use
    if (c->psave) (void)hipFree(c->psave);                // (option spec_predict)
    predict_release(c);                                   // the workspace of tnml_predict_* (first call)
    response_release(c);                                  // and of tnml_response_*
    sitegrad_release(c);                                  // and of tnml_site_gradient_*
    step_release(c);                                      // the optimiser state of tnml_site_step_*
    io_release(c);                                        // the check block and the entry event of the tnml_*_dev calls
    for (auto& sl : c->slabs) if (sl.base) (void)hipFree(sl.base);
    if (c->hrep) (void)hipHostFree(c->hrep);
    if (c->hcost) (void)hipHostFree(c->hcost);
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    if (c->ev_compute) (void)hipEventDestroy(c->ev_compute);
    for (auto& e : c->env) { if (e.host) { if (e.host_pinned) (void)hipHostFree(e.host); else free(e.host); } if (e.ev) (void)hipEventDestroy(e.ev); }
    for (auto& sl : c->slabs) if (sl.ev) (void)hipEventDestroy(sl.ev);
    if (c->h_scal) (void)hipHostFree(c->h_scal);
    if (c->blas) rocblas_destroy_handle(c->blas);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}
