// tnml_env.hip -- environments: the slab allocator with its host tier, and the environment shift (TrainStates::init / shiftE,
// fixedL.cc:122-157,192-233).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "tnml_host.h"

// ---- environments -------------------------------------------------------------------------------
void slot_release(tnml_ctx* c, EnvSlot& e) {
    e.on_host = false;                                   // (a spilled copy of an environment that is being rebuilt is stale)
    if (!e.ptr) return;
    if (e.ev_pending) {                                  // a prefetch of the value that is being replaced is still in flight: the unit's next user must not overtake it
        EnvSlab& sl = c->slabs[e.slab];
        if (!sl.ev) (void)hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming);
        (void)hipEventRecord(sl.ev, c->copy_stream);
        sl.ev_pending = true; e.ev_pending = false;
    }
    c->slabs[e.slab].mask &= (e.unit < 0) ? 0u : ~(1u << e.unit);
    e.ptr = nullptr; e.slab = e.unit = -1;
}
// The host tier.  With option env_budget_mb the environment slabs on the device are capped; when a new slab would exceed the cap (or
// hipMalloc fails) a whole slab is evicted: the one whose environments lie farthest from the current bond -- in a sweep those are
// needed last -- and none of which is an operand of the operation in flight.  Copies run on the compute stream (in order with the
// kernels that wrote / will read the data); pinned host buffers when the host grants them, pageable ones otherwise.
static bool env_is_protected(const tnml_ctx* c, int j) { for (int k = 0; k < 4; ++k) if (c->env_protect[k] == j) return true; return false; }
static int env_copy_stream(tnml_ctx* c) {
    if (c->copy_stream) return 0;
    HIPCK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    HIPCK(c, hipEventCreateWithFlags(&c->ev_compute, hipEventDisableTiming));
    return 0;
}
static int env_host_buffer(tnml_ctx* c, EnvSlot& e, size_t bytes, int j) {
    if (e.host_cap >= bytes) return 0;
    if (e.host) { if (e.host_pinned) (void)hipHostFree(e.host); else free(e.host); e.host = nullptr; e.host_cap = 0; }
    void* hp = nullptr;
    if (hipHostMalloc(&hp, bytes, hipHostMallocDefault) == hipSuccess) { e.host = (char*)hp; e.host_pinned = true; }
    else { (void)hipGetLastError(); e.host = (char*)malloc(bytes); e.host_pinned = false; }
    if (!e.host) return tnml_fail(c, "environment spill: no host memory for %zu bytes (site %d)", bytes, j);
    e.host_cap = bytes;
    return 0;
}
// environment j -> host.  Asynchronous form (pinned buffer, option env_async): the copy runs on the copy stream once everything the
// compute stream holds so far has finished, and the slab remembers the event that marks its end; whoever takes a unit of that slab
// next waits for it.  Otherwise: on the compute stream, in order.
static int env_spill(tnml_ctx* c, int j) {
    EnvSlot& e = c->env[j];
    const size_t bytes = (size_t)e.L * e.m * c->NTp * c->eesz();
    TCK(env_host_buffer(c, e, bytes, j));
    EnvSlab& sl = c->slabs[e.slab];
    if (c->env_async && e.host_pinned) {
        TCK(env_copy_stream(c));
        HIPCK(c, hipEventRecord(c->ev_compute, c->stream));
        HIPCK(c, hipStreamWaitEvent(c->copy_stream, c->ev_compute, 0));
        HIPCK(c, hipMemcpyAsync(e.host, e.ptr, bytes, hipMemcpyDeviceToHost, c->copy_stream));
        if (!sl.ev) HIPCK(c, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
        HIPCK(c, hipEventRecord(sl.ev, c->copy_stream));
        sl.ev_pending = true;
    } else {
        if (e.ev_pending) { HIPCK(c, hipStreamWaitEvent(c->stream, e.ev, 0)); }
        HIPCK(c, hipMemcpyAsync(e.host, e.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
        if (!e.host_pinned) SYNCK(c, c->stream);
    }
    e.ev_pending = false;                               // (a copy back that was still in flight is ordered before this one: same stream, or waited for above)
    sl.mask &= (e.unit < 0) ? 0u : ~(1u << e.unit);
    e.ptr = nullptr; e.slab = e.unit = -1; e.on_host = true;
    c->env_spills += 1;
    return 0;
}
static int env_evict_slab(tnml_ctx* c) {                // frees one whole slab; 1 = nothing could be evicted
    const int pos = c->currb > 0 ? c->currb : 1;
    int best = -1, best_d = -1;
    for (size_t k = 0; k < c->slabs.size(); ++k) {
        if (!c->slabs[k].mask) continue;
        int dmin = 1 << 30; bool ok = true, any = false;
        for (int j = 1; j <= c->N; ++j) {
            const EnvSlot& e = c->env[j];
            if (!e.ptr || e.slab != (int)k) continue;
            any = true;
            if (env_is_protected(c, j)) { ok = false; break; }
            const int d = j > pos ? j - pos : pos - j;
            if (d < dmin) dmin = d;
        }
        if (!ok || !any) continue;                      // (slabs that hold classify's chain buffers have no environment: never evicted)
        if (dmin > best_d) { best_d = dmin; best = (int)k; }
    }
    if (best < 0) return 1;
    for (int j = 1; j <= c->N; ++j) if (c->env[j].ptr && c->env[j].slab == best) TCK(env_spill(c, j));
    return 0;
}
// consumer: the stream whose work will touch the new unit first (it waits for a copy to the host that may still be reading the slab)
int slot_acquire(tnml_ctx* c, EnvSlot& e, int m, int L, hipStream_t consumer) {
    slot_release(c, e);
    if (!consumer) consumer = c->stream;
    const unsigned FULL = (1u << TNML_NL) - 1;
    const size_t slab_bytes = c->big_elems * c->eesz();
    for (;;) {
        int pick = -1;
        if (L != TNML_NL) for (size_t k = 0; k < c->slabs.size(); ++k) if (c->slabs[k].mask && c->slabs[k].mask != FULL) { pick = (int)k; break; }   // fill split slabs first
        if (pick < 0) for (size_t k = 0; k < c->slabs.size(); ++k) if (!c->slabs[k].mask) { pick = (int)k; break; }
        if (pick < 0) {
            const bool capped = c->env_budget_bytes > 0 && (c->slabs.size() + 1) * slab_bytes > (size_t)c->env_budget_bytes;
            EnvSlab sl;
            if (!capped && hipMalloc((void**)&sl.base, slab_bytes) == hipSuccess) {
                c->bytes += (int64_t)slab_bytes;
                c->slabs.push_back(sl); pick = (int)c->slabs.size() - 1;
            } else {
                if (!capped) (void)hipGetLastError();
                if (env_evict_slab(c) != 0)
                    return tnml_fail(c, capped ? "environment memory: the budget of %ld MB holds no slab that could be evicted (%zu slabs of %zu MB; every one holds an operand of the operation in flight)"
                                               : "environment memory: hipMalloc failed and no slab could be evicted (env_budget %ld MB, %zu slabs of %zu MB)",
                                     c->env_budget_bytes >> 20, c->slabs.size(), slab_bytes >> 20);
                continue;
            }
        }
        EnvSlab& sl = c->slabs[pick];
        if (sl.ev_pending) HIPCK(c, hipStreamWaitEvent(consumer, sl.ev, 0));
        e.slab = pick; e.m = m; e.L = L;
        if (L == TNML_NL) { e.unit = -1; sl.mask = FULL; e.ptr = sl.base; }
        else {
            int u = 0; while (sl.mask & (1u << u)) ++u;
            e.unit = u; sl.mask |= 1u << u; e.ptr = sl.base + (size_t)u * c->small_elems * c->eesz();
        }
        return 0;
    }
}
// host -> device for environment j, started now; the compute stream is made to wait for it by env_ensure
static int env_fetch(tnml_ctx* c, int j) {
    EnvSlot& e = c->env[j];
    const int m = e.m, L = e.L;
    const size_t bytes = (size_t)L * m * c->NTp * c->eesz();
    const bool async = c->env_async && e.host_pinned;
    c->env_epoch += 1;
    if (async) TCK(env_copy_stream(c));
    TCK(slot_acquire(c, e, m, L, async ? c->copy_stream : c->stream));     // (clears on_host; the host copy stays valid until the copy below has read it)
    if (async) {
        // the unit may have been vacated by slot_release a moment ago (no event of its own): order the copy behind everything the compute
        // stream has been given so far -- work that is normally long finished, so the overlap with the current bond update stays
        HIPCK(c, hipEventRecord(c->ev_compute, c->stream));
        HIPCK(c, hipStreamWaitEvent(c->copy_stream, c->ev_compute, 0));
        HIPCK(c, hipMemcpyAsync(e.ptr, e.host, bytes, hipMemcpyHostToDevice, c->copy_stream));
        if (!e.ev) HIPCK(c, hipEventCreateWithFlags(&e.ev, hipEventDisableTiming));
        HIPCK(c, hipEventRecord(e.ev, c->copy_stream));
        e.ev_pending = true;
    } else {
        HIPCK(c, hipMemcpyAsync(e.ptr, e.host, bytes, hipMemcpyHostToDevice, c->stream));
        if (!e.host_pinned) SYNCK(c, c->stream);
    }
    c->env_fetches += 1;
    return 0;
}
// the environment of site j on the device and visible to the compute stream (no-op when it is there)
int env_ensure(tnml_ctx* c, int j) {
    EnvSlot& e = c->env[j];
    if (e.on_host) TCK(env_fetch(c, j));
    if (e.ev_pending) { HIPCK(c, hipStreamWaitEvent(c->stream, e.ev, 0)); e.ev_pending = false; }
    return 0;
}
static int env_alloc(tnml_ctx* c, int j, int m, int L) { return slot_acquire(c, c->env[j], m, L); }
// Host tier, beside the bond update that is about to be enqueued: the environment the NEXT bond of the sweep will need is started on
// its way back (half 1 moves right: bond b + 1 reads the right environment of site b + 3; half 2 moves left: site b - 2), and one slab
// is kept free for the environment shiftE will build at the end of this bond update -- its eviction, if one is needed, then runs beside
// this bond update's kernels instead of in front of the shift.
int env_lookahead(tnml_ctx* c, int b, int ha) {
    const int next = ha == 1 ? b + 3 : b - 2;
    EnvProtect keep(c, b - 1 > 0 ? b - 1 : 0, b + 2 <= c->N ? b + 2 : 0, (next >= 1 && next <= c->N) ? next : 0);
    if (next >= 1 && next <= c->N && c->env[next].on_host) { TCK(env_fetch(c, next)); c->env_prefetches += 1; }
    bool free_slab = false;
    for (const auto& sl : c->slabs) if (!sl.mask) { free_slab = true; break; }
    const size_t slab_bytes = c->big_elems * c->eesz();
    if (!free_slab && (c->slabs.size() + 1) * slab_bytes > (size_t)c->env_budget_bytes) (void)env_evict_slab(c);     // (nothing evictable: the shift will say so if it matters)
    return 0;
}
const void* phi_site(const tnml_ctx* c, int j) { return (const char*)c->phi + (size_t)(j - 1) * 2 * c->NTp * c->eesz(); }

// dst = src*(t.A(cs)*W.A(cs)) (fixedL.cc:142-149,221-228); src == nullptr: chain end.  dst is an environment
// ([Lout][m_out][NTp] in the env type) or, with acc_out, a buffer of the arithmetic type (the last step of toverlap)
int shift_core(tnml_ctx* c, int cs, bool from_left, const void* src, int Le, void* dst, bool acc_out, int* Lout_p) {
    const SiteT& A = c->W[cs];
    const int m_in = from_left ? A.ml : A.mr, m_out = from_left ? A.mr : A.ml;
    if (!src && m_in != 1) return tnml_fail(c, "shift: chain-end site %d has outer dimension %d", cs, m_in);
    if (Le == TNML_NL && A.L == TNML_NL) return tnml_fail(c, "shift: Label index on both env and site");
    const int Lout = A.L > Le ? A.L : Le;
    if (Lout_p) *Lout_p = Lout;
    c->env_epoch += 1;                                  // an environment is about to be written: bf16 copies made from environments are stale
    PackDesc d;
    d.TO = 1; d.L = A.L; d.st = 0; d.ss = A.ml; d.sl = (long)2 * A.ml * A.mr;
    if (from_left) { d.nx = A.ml; d.sx = 1; d.ny = A.mr; d.sy = 2 * A.ml; }
    else           { d.nx = A.mr; d.sx = 2 * A.ml; d.ny = A.ml; d.sy = 1; }
    d.Kp = ru16(2 * d.nx); d.Np = ru16(d.ny);
    if ((size_t)d.L * d.Kp * d.Np > c->sM_cap || (size_t)d.L * d.Kp * d.Np > c->mcap)
        return tnml_fail(c, "shift: packed site matrix of site %d (%d x %d x %d) exceeds the workspace", cs, d.L, d.Kp, d.Np);
    if (c->f64()) {                                     // fp64 MFMA shift (M in the free SVD workspace); fp32-stored environments (TNML_F64_E32) are rounded once, on the store
        TCK(launch_pack(c, d, A.a, c->sM, nullptr));
        Fgemm64Args f;
        f.EI = src ? src : c->ones;
        f.EI_lstride = (Le == TNML_NL) ? (size_t)m_in * c->NTp : 0;
        f.mI = m_in; f.phiI = phi_site(c, cs);
        f.M = c->sM; f.M_lstride = (A.L == TNML_NL) ? (size_t)d.Kp * d.Np : 0; f.Kp = d.Kp; f.Np = d.Np;
        f.phiO = nullptr;
        f.out = (double*)dst; f.out_lstride = (size_t)m_out * c->NTp; f.mO = m_out;
        f.NTp = c->NTp; f.L = Lout; f.env64 = c->env64(); f.out32 = !c->env64() && !acc_out;
        // the Label-carrying shift with the site matrix resident in registers (kernels_res.hip): input dimensions 33..120, output up to 128
        if (c->shift_res && c->env64() && !acc_out && src && Le == TNML_NL && A.L == 1 && shift_res_applies(m_in, m_out) && d.Np <= 128 &&
            (c->shift_res >= 2 || c->NTp >= 7680) &&
            (size_t)TNML_NL * m_in * c->NTp * sizeof(double) < ((size_t)1 << 32)) {      // (32-bit lane offsets: beyond ~447 000 images per rank the generic kernel takes over)
            ShiftResArgs sa{(const double*)src, (size_t)m_in * c->NTp, (const double*)phi_site(c, cs), c->sM, (double*)dst, (size_t)m_out * c->NTp, m_out, c->NTp, Lout, m_in, d.Kp, d.Np};
            if (c->shift_skip && c->zs_ord) { sa.ord = c->zs_ord + (size_t)(cs - 1) * c->NTp; sa.nz = c->zs_nz + (size_t)(cs - 1) * (c->NTp / 64); }
            return launch_shift_res(c, sa);
        }
        return launch_fgemm64(c, f);
    }
    TCK(launch_pack(c, d, A.a, nullptr, c->Mf));
    FgemmArgs f;
    f.EI = src ? (const float*)src : (const float*)c->ones;
    f.EI_lstride = (Le == TNML_NL) ? (size_t)m_in * c->NTp : 0;
    f.mI = m_in; f.phiI = (const float*)phi_site(c, cs);
    f.M = c->Mf; f.M_lstride = (A.L == TNML_NL) ? (size_t)d.Kp * d.Np : 0; f.Kp = d.Kp; f.Np = d.Np;
    f.phiO = nullptr;
    f.out = (float*)dst; f.out_lstride = (size_t)m_out * c->NTp; f.mO = m_out;
    f.NTp = c->NTp; f.L = Lout;
    return launch_fgemm(c, f);
}
// new env at site cs from the env at ps (0: chain end)
static int shift_site(tnml_ctx* c, int cs, int ps, bool from_left) {
    const SiteT& A = c->W[cs];
    const bool has_prev = ps >= 1 && ps <= c->N;
    if (has_prev && !c->env[ps].built()) return tnml_fail(c, "shift: environment of site %d missing", ps);
    // the source, the destination and the two environments of the bond in flight (its plan holds their addresses) stay on the device
    EnvProtect keep(c, has_prev ? ps : 0, cs, c->currb > 0 ? c->currb - 1 : 0, c->currb > 0 ? c->currb + 2 : 0);
    if (has_prev) TCK(env_ensure(c, ps));
    const int m_in = from_left ? A.ml : A.mr, m_out = from_left ? A.mr : A.ml;
    const int Le = has_prev ? c->env[ps].L : 1;
    if (has_prev && c->env[ps].m != m_in) return tnml_fail(c, "shift: env dim %d != site dim %d at site %d", c->env[ps].m, m_in, cs);
    if (Le == TNML_NL && A.L == TNML_NL) return tnml_fail(c, "shift: Label index on both env and site");
    TCK(env_alloc(c, cs, m_out, A.L > Le ? A.L : Le));
    return shift_core(c, cs, from_left, has_prev ? c->env[ps].ptr : nullptr, Le, c->env[cs].ptr, false, nullptr);
}

int env_init_impl(tnml_ctx* c) {
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (!c->data_set) return tnml_fail(c, "tnml_env_init: training data not set");
    TCK(check_W(c));
    for (int j = 1; j <= c->N; ++j) c->W[j].placed = false;                                // (a series of tnml_mps_place ends where W is used)
    for (int n = c->N; n >= 3; --n) TCK(shift_site(c, n, n == c->N ? 0 : n + 1, false));   // :136-153
    c->currb = -1;
    const int rc = set_bond_impl(c, 1);                                                    // :156
    if (rc) { c->currb = -1; c->plan = BondPlan(); }
    return rc;
}
int tnml_env_init(tnml_ctx* c) {       // TrainStates::init, fixedL.cc:122-157
    CollScope coll_(c);                // every rank calls it in step: a rank that fails here (host tier out of memory) tells its peers at once
    TCK(ho_locked(c, "tnml_env_init", true));
    TCK(env_init_impl(c));
    c->sweep_start = true;
    return 0;
}
int shift_env_impl(tnml_ctx* c, int b, int from_left) {
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (b < 1 || b > c->N - 1) return tnml_fail(c, "tnml_shift_env: bond %d out of range", b);
    const int cs = from_left ? b : b + 1;              // :196
    const int prevc = from_left ? b - 1 : b + 2;       // :199
    return shift_site(c, cs, (prevc >= 1 && prevc <= c->N) ? prevc : 0, from_left != 0);
}
int tnml_shift_env(tnml_ctx* c, int b, int from_left) {   // TrainStates::shiftE, fixedL.cc:192-233
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_shift_env", true));
    c->sweep_start = false;
    return shift_env_impl(c, b, from_left);
}
int tnml_env_stats(tnml_ctx* c, int64_t* spills, int64_t* fetches, int64_t* slabs_on_device, int64_t* host_bytes) {
    if (spills) *spills = c->env_spills;
    if (fetches) *fetches = c->env_fetches;
    if (slabs_on_device) *slabs_on_device = (int64_t)c->slabs.size();
    if (host_bytes) { int64_t hb = 0; for (const auto& e : c->env) if (e.on_host) hb += (int64_t)e.L * e.m * c->NTp * (int64_t)c->eesz(); *host_bytes = hb; }
    return 0;
}
int tnml_env_dims(tnml_ctx* c, int j, int* m, int* has_label) {
    if (j < 1 || j > c->N || !c->env[j].built()) return tnml_fail(c, "tnml_env_dims: environment of site %d not built", j);
    *m = c->env[j].m; *has_label = c->env[j].L == TNML_NL;
    return 0;
}
int tnml_get_env(tnml_ctx* c, int j, double* E) {
    if (j < 1 || j > c->N || !c->env[j].built()) return tnml_fail(c, "tnml_get_env: environment of site %d not built", j);
    {
        EnvProtect keep(c, j, c->currb > 0 ? c->currb - 1 : 0, c->currb > 0 ? c->currb + 2 : 0);
        TCK(env_ensure(c, j));
    }
    const EnvSlot& e = c->env[j];
    const size_t ne = (size_t)e.L * e.m * c->NTp;
    std::vector<char> h(ne * c->eesz());
    SYNCK(c, c->stream);
    HIPCK(c, hipMemcpy(h.data(), e.ptr, h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < c->NT; ++i)
        for (int l = 0; l < e.L; ++l)
            for (int q = 0; q < e.m; ++q) {
                const size_t k = ((size_t)l * e.m + q) * c->NTp + i;
                E[(size_t)i * e.m * e.L + q + (size_t)e.m * l] = c->env64() ? ((const double*)h.data())[k] : (double)((const float*)h.data())[k];
            }
    return 0;
}
