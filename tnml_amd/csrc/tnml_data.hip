// tnml_data.hip -- what a context is given: labels and features (as features, as bytes, as bytes through an input map), the tile
// order tables that follow the features, and the replica of the weight MPS.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "tnml_host.h"

// ---- training set -----------------------------------------------------------------------------
static int set_labels(tnml_ctx* c, const int32_t* labels) {
    std::vector<int> lab(c->NTp, -1);
    for (int i = 0; i < c->NT; ++i) {
        if (labels[i] < 0 || labels[i] >= TNML_NL) return tnml_fail(c, "label %d of image %d out of range", labels[i], i);
        lab[i] = labels[i];
    }
    HIPCK(c, hipMemcpy(c->label, lab.data(), sizeof(int) * c->NTp, hipMemcpyHostToDevice));
    return 0;
}
// the tile order tables of k_shift_res follow the stored features: rebuilt whenever the data are replaced (contexts that have them)
static int shift_order_build(tnml_ctx* c) {
    if (!c->zs_ord) return 0;
    TCK(launch_shift_order(c, (const double*)c->phi, c->N, c->NTp, c->zs_ord, c->zs_nz, c->zs_cnt));
    c->zs_groups.assign(c->N, 0);
    HIPCK(c, hipMemcpyAsync(c->zs_groups.data(), c->zs_cnt, sizeof(int) * c->N, hipMemcpyDeviceToHost, c->stream));
    if (c->zf_ord) {                                  // the table of k_fwd_res's 32-image tiles
        TCK(launch_fwd_order(c, (const double*)c->phi, c->N, c->NTp, c->zf_ord, c->zf_cnt));
        c->zf_groups.assign(c->N, 0);
        HIPCK(c, hipMemcpyAsync(c->zf_groups.data(), c->zf_cnt, sizeof(int) * c->N, hipMemcpyDeviceToHost, c->stream));
    }
    SYNCK(c, c->stream);
    return 0;
}
int tnml_fwd_skip_stats(tnml_ctx* c, int site, int64_t* groups, int64_t* skipped) {
    if (!c) return tnml_fail(c, "tnml_fwd_skip_stats: null argument");
    if (site < 1 || site > c->N) return tnml_fail(c, "tnml_fwd_skip_stats: site %d out of range", site);
    if (!c->zf_ord || !c->data_set || c->zf_groups.size() != (size_t)c->N) return tnml_fail(c, "tnml_fwd_skip_stats: this context has no tile order tables (fp64 storage, fixedL, maxm >= 33, data set)");
    if (groups) *groups = (int64_t)(c->NTp / 16);
    if (skipped) *skipped = c->zf_groups[site - 1];
    return 0;
}
int tnml_shift_skip_stats(tnml_ctx* c, int site, int64_t* groups, int64_t* skipped) {
    if (!c) return tnml_fail(c, "tnml_shift_skip_stats: null argument");
    if (site < 1 || site > c->N) return tnml_fail(c, "tnml_shift_skip_stats: site %d out of range", site);
    if (!c->zs_ord || !c->data_set || c->zs_groups.size() != (size_t)c->N) return tnml_fail(c, "tnml_shift_skip_stats: this context has no tile order tables (fp64 storage, fixedL, maxm >= 33, data set)");
    if (groups) *groups = (int64_t)(c->NTp / 16);
    if (skipped) *skipped = c->zs_groups[site - 1];
    return 0;
}
// ---- input map (tnml.h): geometry + table; consulted by tnml_set_data_u8 / tnml_predict_u8 when bytes arrive -------------------------
StageGeom stage_geom(const tnml_ctx* c) {
    const tnml_input_map& m = c->im;
    return StageGeom{m.src_rows * m.src_cols, m.src_cols, m.block, m.row0, m.col0, m.out_rows, m.out_cols};
}
int tnml_set_input_map(tnml_ctx* c, const tnml_input_map* m) {
    if (!c) return tnml_fail(c, "tnml_set_input_map: null argument");
    TCK(ho_locked(c, "tnml_set_input_map"));
    if (c->pend_count > 0) return tnml_fail(c, "tnml_set_input_map: a bond update is in flight (tnml_bond_update_end first)");
    if (m) {
        if (m->block < 1 || m->block > 8) return tnml_fail(c, "tnml_set_input_map: block = %d, must be 1..8", m->block);
        if (m->ncodes != 255 * m->block * m->block + 1) return tnml_fail(c, "tnml_set_input_map: ncodes = %d, must be 255 block^2 + 1 = %d", m->ncodes, 255 * m->block * m->block + 1);
        if (m->src_rows < 1 || m->src_cols < 1 || (int64_t)m->src_rows * m->src_cols > (int64_t)1 << 30)
            return tnml_fail(c, "tnml_set_input_map: src_rows x src_cols = %d x %d, must be at least 1 x 1 and at most 2^30 bytes", m->src_rows, m->src_cols);
        if (m->out_rows < 1 || m->out_cols < 1 || (int64_t)m->out_rows * m->out_cols != c->N)
            return tnml_fail(c, "tnml_set_input_map: out_rows * out_cols = %d * %d, must be N = %d", m->out_rows, m->out_cols, c->N);
        if (m->row0 < 0 || m->row0 + (int64_t)m->block * m->out_rows > m->src_rows)
            return tnml_fail(c, "tnml_set_input_map: row0 = %d: blocks of %d rows from there leave the %d source rows", m->row0, m->block, m->src_rows);
        if (m->col0 < 0 || m->col0 + (int64_t)m->block * m->out_cols > m->src_cols)
            return tnml_fail(c, "tnml_set_input_map: col0 = %d: blocks of %d columns from there leave the %d source columns", m->col0, m->block, m->src_cols);
        if (!m->table) return tnml_fail(c, "tnml_set_input_map: table is NULL");
        for (int k = 0; k < 2 * m->ncodes; ++k)
            if (!std::isfinite(m->table[k])) return tnml_fail(c, "tnml_set_input_map: table[%d][%d] is not finite", k / 2, k % 2);
    }
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (c->pk.map_bytes) { HIPCK(c, hipStreamSynchronize(c->stream)); predict_release_map(c); }
    if (c->rs.bytes) { HIPCK(c, hipStreamSynchronize(c->stream)); response_release(c); }
    tape_kill(c, "tnml_set_input_map");
    if (c->sg.bytes) { HIPCK(c, hipStreamSynchronize(c->stream)); sitegrad_release(c); }
    if (!m) { c->im_set = false; c->im = tnml_input_map{}; c->im_table.clear(); return 0; }
    c->im_table.assign(m->table, m->table + (size_t)2 * m->ncodes);
    c->im = *m; c->im.table = nullptr;
    c->im_set = true;
    return 0;
}
int tnml_get_input_map(tnml_ctx* c, tnml_input_map* out) {
    if (!c || !out) return tnml_fail(c, "tnml_get_input_map: null argument");
    *out = c->im_set ? c->im : tnml_input_map{};
    out->table = nullptr;
    return 0;
}
// tnml_set_data_u8 under a map (k_features_codes): raw -> block sums (k_stage_codes with ld = NTp) -> phi [N][2][NTp] through the table in the
// context's storage type; the three temporaries are freed before the call returns
static int features_codes(tnml_ctx* c, const uint8_t* pixels) {
    const StageGeom g = stage_geom(c);
    const size_t nraw = (size_t)c->NT * g.S, ncode = (size_t)c->N * c->NTp * sizeof(uint16_t), ntab = c->im_table.size();
    std::vector<float> tab32;
    if (!c->env64()) { tab32.resize(ntab); for (size_t k = 0; k < ntab; ++k) tab32[k] = (float)c->im_table[k]; }   // rounded once, as tnml_set_data_phi rounds phi
    const size_t tabb = ntab * (c->env64() ? sizeof(double) : sizeof(float));
    uint8_t* d_raw = nullptr; uint16_t* d_codes = nullptr; void* d_tab = nullptr;
    int rc = 0;
    auto hip = [&](hipError_t e, const char* what) { if (!rc && e != hipSuccess) rc = tnml_fail(c, "tnml_set_data_u8: %s failed: %s", what, hipGetErrorString(e)); };
    hip(hipMalloc((void**)&d_raw, nraw), "hipMalloc of the raw bytes");
    if (!rc) hip(hipMalloc((void**)&d_codes, ncode), "hipMalloc of the block sums");
    if (!rc) hip(hipMalloc(&d_tab, tabb), "hipMalloc of the table");
    if (!rc) hip(hipMemcpyAsync(d_raw, pixels, nraw, hipMemcpyHostToDevice, c->stream), "copy of the raw bytes");
    if (!rc) hip(hipMemcpyAsync(d_tab, c->env64() ? (const void*)c->im_table.data() : (const void*)tab32.data(), tabb, hipMemcpyHostToDevice, c->stream), "copy of the table");
    if (!rc) {
        ProfScope ps(c, KC_PACK);
        rc = launch_stage_codes(c, d_raw, g, c->NT, c->NTp, d_codes);
        if (!rc) rc = launch_codes_phi(c, d_codes, d_tab, c->N, c->NT, c->NTp, c->phi);
    }
    hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    (void)hipFree(d_raw); (void)hipFree(d_codes); (void)hipFree(d_tab);
    return rc;
}
int tnml_set_data_u8(tnml_ctx* c, const uint8_t* pixels, const int32_t* labels) {
    TCK(ho_locked(c, "tnml_set_data_u8", true));
    HIPCK(c, hipSetDevice(c->cfg.device));
    TCK(set_labels(c, labels));
    if (c->im_set) {
        TCK(features_codes(c, pixels));
        TCK(shift_order_build(c));
        c->data_set = true; c->currb = -1; c->p_valid = false; c->sweep_start = false;
        return 0;
    }
    uint8_t* d_pix = nullptr;
    const size_t nb = (size_t)c->NT * c->N;
    HIPCK(c, hipMalloc((void**)&d_pix, nb));
    HIPCK(c, hipMemcpy(d_pix, pixels, nb, hipMemcpyHostToDevice));
    int rc = launch_features_u8(c, d_pix, c->N, c->NT, c->NTp, c->phi);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(d_pix);
    if (rc) return rc;
    TCK(shift_order_build(c));
    c->data_set = true; c->currb = -1; c->p_valid = false; c->sweep_start = false;
    return 0;
}
int tnml_set_data_phi(tnml_ctx* c, const double* phi, const int32_t* labels) {
    TCK(ho_locked(c, "tnml_set_data_phi", true));
    HIPCK(c, hipSetDevice(c->cfg.device));
    TCK(set_labels(c, labels));
    // TState::data[(j-1)*d + (n-1)] (fixedL.cc:39-46) -> [N][2][NTp], rounded once to fp32
    const size_t ne = (size_t)c->N * 2 * c->NTp;
    if (c->env64()) {
        std::vector<double> h(ne, 0.);
        for (int i = 0; i < c->NT; ++i) for (int j = 0; j < c->N; ++j) for (int s = 0; s < 2; ++s)
            h[((size_t)j * 2 + s) * c->NTp + i] = phi[((size_t)i * c->N + j) * 2 + s];
        HIPCK(c, hipMemcpy(c->phi, h.data(), sizeof(double) * ne, hipMemcpyHostToDevice));
        TCK(shift_order_build(c));
    } else {
        std::vector<float> h(ne, 0.f);
        for (int i = 0; i < c->NT; ++i) for (int j = 0; j < c->N; ++j) for (int s = 0; s < 2; ++s)
            h[((size_t)j * 2 + s) * c->NTp + i] = (float)phi[((size_t)i * c->N + j) * 2 + s];
        HIPCK(c, hipMemcpy(c->phi, h.data(), sizeof(float) * ne, hipMemcpyHostToDevice));
    }
    c->data_set = true; c->currb = -1; c->p_valid = false; c->sweep_start = false;
    return 0;
}

// ---- weight MPS replica -------------------------------------------------------------------------
// what tnml_set_site asks of its arguments, in its words
static int set_site_rules(tnml_ctx* c, int j, int ml, int mr, int has_label) {
    if (j < 1 || j > c->N) return tnml_fail(c, "tnml_set_site: site %d out of range", j);
    if (c->single() && has_label) return tnml_fail(c, "tnml_set_site: the per-label variant has no Label index");
    if ((j == c->c0) != (has_label != 0)) return tnml_fail(c, "Label Index not on site %d", c->c0);     // fixedL.cc:734
    if (ml < 1 || mr < 1 || ml > c->maxm || mr > c->maxm) return tnml_fail(c, "tnml_set_site: bond dimension outside 1..maxm");
    if ((j == 1 && ml != 1) || (j == c->N && mr != 1)) return tnml_fail(c, "tnml_set_site: edge sites must have outer dimension 1");
    return 0;
}
int tnml_set_site(tnml_ctx* c, int j, int ml, int mr, int has_label, const double* A) {
    TCK(ho_locked(c, "tnml_set_site", true));
    TCK(set_site_rules(c, j, ml, mr, has_label));
    SiteT& s = c->W[j];
    s.ml = ml; s.mr = mr; s.L = has_label ? TNML_NL : 1; s.set = true; s.placed = false;
    w_written(c, "tnml_set_site");
    HIPCK(c, hipMemcpy(s.a, A, sizeof(double) * (size_t)ml * 2 * mr * s.L, hipMemcpyHostToDevice));
    c->currb = -1; c->p_valid = false; c->sweep_start = false;
    for (int b = j - 1; b <= j; ++b) if (b >= 1 && b < (int)c->bond_hist.size()) c->bond_hist[b] = tnml_ctx::BondHist();   // the bonds of this site start over (option spec_predict)
    return 0;
}
int tnml_site_dims(tnml_ctx* c, int j, int* ml, int* mr, int* has_label) {
    if (j < 1 || j > c->N || !c->W[j].set) return tnml_fail(c, "tnml_site_dims: site %d not set", j);
    *ml = c->W[j].ml; *mr = c->W[j].mr; *has_label = c->W[j].L == TNML_NL;
    return 0;
}
int tnml_get_site(tnml_ctx* c, int j, double* A) {
    if (j < 1 || j > c->N || !c->W[j].set) return tnml_fail(c, "tnml_get_site: site %d not set", j);
    const SiteT& s = c->W[j];
    SYNCK(c, c->stream);
    HIPCK(c, hipMemcpy(A, s.a, sizeof(double) * (size_t)s.ml * 2 * s.mr * s.L, hipMemcpyDeviceToHost));
    return 0;
}
// ---- device-resident arguments (tnml.h, "device-resident arguments") ------------------------------------------------
int dev_check_args(tnml_ctx* c, const char* who, const std::vector<DevArg>& args) {
    struct Range { const char* name; uintptr_t lo, hi; bool out; };
    std::vector<Range> seen;
    for (const DevArg& a : args) {
        if (!a.p) continue;
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof(at));
        const hipError_t e = hipPointerGetAttributes(&at, a.p);
        if (e != hipSuccess) {
            (void)hipGetLastError();                      // (the runtime keeps the error of a pointer it does not know)
            return tnml_fail(c, "%s: %s = %p is not device memory: the runtime does not know the pointer (%s)", who, a.name, a.p, hipGetErrorString(e));
        }
        if (at.type != hipMemoryTypeDevice || at.isManaged)
            return tnml_fail(c, "%s: %s = %p is not device memory (%s): the _dev calls take plain device allocations only", who, a.name, a.p,
                             at.isManaged || at.type == hipMemoryTypeManaged ? "managed memory" : at.type == hipMemoryTypeHost ? "host memory known to the runtime" : "memory the runtime does not describe");
        if (at.device != c->cfg.device) return tnml_fail(c, "%s: %s = %p lies on device %d, the context is on device %d", who, a.name, a.p, at.device, c->cfg.device);
        const uintptr_t lo = (uintptr_t)a.p;
        if (a.align > 1 && lo % a.align) return tnml_fail(c, "%s: %s = %p is not aligned to %zu bytes", who, a.name, a.p, a.align);
        hipDeviceptr_t base = nullptr; size_t size = 0;
        const hipError_t r = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)a.p);
        if (r != hipSuccess) {
            (void)hipGetLastError();
            return tnml_fail(c, "%s: %s = %p: the runtime gives no allocation for the pointer (%s)", who, a.name, a.p, hipGetErrorString(r));
        }
        const uintptr_t b0 = (uintptr_t)base;
        if (lo < b0 || a.bytes > size || lo - b0 > size - a.bytes)
            return tnml_fail(c, "%s: %s = %p needs %zu bytes, its allocation ends %zu bytes behind it", who, a.name, a.p, a.bytes, (size_t)(b0 + size > lo ? b0 + size - lo : 0));
        for (const Range& o : seen)
            if ((a.out || o.out) && a.bytes && lo < o.hi && o.lo < lo + a.bytes)
                return tnml_fail(c, "%s: %s overlaps %s: an output may share no byte with another argument", who, a.name, o.name);
        if (a.bytes) seen.push_back({a.name, lo, lo + a.bytes, a.out});
    }
    return 0;
}
int dev_entry_wait(tnml_ctx* c, const char* who, void* stream) {
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (!c->io_ev && hipEventCreateWithFlags(&c->io_ev, hipEventDisableTiming) != hipSuccess) { c->io_ev = nullptr; return tnml_fail(c, "%s: hipEventCreate failed", who); }
    if ((hipStream_t)stream == c->stream) return 0;
    HIPCK(c, hipEventRecord(c->io_ev, (hipStream_t)stream));
    HIPCK(c, hipStreamWaitEvent(c->stream, c->io_ev, 0));
    return 0;
}
int tnml_set_site_dev(tnml_ctx* c, int j, int ml, int mr, int has_label, const double* A_dev, void* stream) {
    if (!c || !A_dev) return tnml_fail(c, "tnml_set_site_dev: null argument");
    TCK(ho_locked(c, "tnml_set_site_dev", true));
    TCK(set_site_rules(c, j, ml, mr, has_label));
    const size_t bytes = sizeof(double) * (size_t)ml * 2 * mr * (has_label ? TNML_NL : 1);
    TCK(dev_check_args(c, "tnml_set_site_dev", {{"A_dev", A_dev, bytes, 8, false}}));
    TCK(dev_entry_wait(c, "tnml_set_site_dev", stream));
    SiteT& s = c->W[j];
    w_written(c, "tnml_set_site_dev");
    HIPCK(c, hipMemcpyAsync(s.a, A_dev, bytes, hipMemcpyDeviceToDevice, c->stream));
    SYNCK(c, c->stream);
    s.ml = ml; s.mr = mr; s.L = has_label ? TNML_NL : 1; s.set = true; s.placed = false;
    c->currb = -1; c->p_valid = false; c->sweep_start = false;
    for (int b = j - 1; b <= j; ++b) if (b >= 1 && b < (int)c->bond_hist.size()) c->bond_hist[b] = tnml_ctx::BondHist();
    return 0;
}
// tnml_set_site_dev for `count` sites in the shapes W has now: every check first, then one entry wait, one table upload, ONE k_sites_gather
// launch (kernels_iocheck.hip) and one synchronisation
int tnml_set_sites_dev(tnml_ctx* c, int count, const int32_t* sites, const double* const* A_dev, void* stream) {
    const char* const who = "tnml_set_sites_dev";
    if (!c) return tnml_fail(c, "%s: null argument", who);
    if (count < 0) return tnml_fail(c, "%s: count = %d, must be >= 0", who, count);
    if (count == 0) return 0;
    if (!sites || !A_dev) return tnml_fail(c, "%s: null argument", who);
    TCK(ho_locked(c, who, true));
    std::vector<char> named(c->N + 1, 0);
    std::vector<std::string> names(count);
    std::vector<DevArg> args(count);
    std::vector<SiteCopy> tab(count);
    long long nblocks = 0;
    for (int k = 0; k < count; ++k) {
        const int j = sites[k];
        if (j < 1 || j > c->N) return tnml_fail(c, "%s: site %d out of range 1..%d (entry %d)", who, j, c->N, k);
        if (!c->W[j].set) return tnml_fail(c, "%s: site %d not set: the call takes the shapes W has (tnml_set_site first)", who, j);
        if (named[j]) return tnml_fail(c, "%s: site %d named twice (entry %d)", who, j, k);
        if (!A_dev[k]) return tnml_fail(c, "%s: null argument (the array of site %d)", who, j);
        named[j] = 1;
        const SiteT& s = c->W[j];
        const long long elems = (long long)s.ml * 2 * s.mr * s.L;
        names[k] = "A_dev of site " + std::to_string(j);
        args[k] = DevArg{names[k].c_str(), A_dev[k], (size_t)elems * sizeof(double), 8, false};
        tab[k] = SiteCopy{A_dev[k], s.a, elems, nblocks};
        nblocks += (elems + SITES_COPY_BLOCK - 1) / SITES_COPY_BLOCK;
    }
    TCK(dev_check_args(c, who, args));
    TCK(dev_entry_wait(c, who, stream));
    if (!c->io_tab) TCK(dalloc(c, (void**)&c->io_tab, (size_t)c->N * sizeof(SiteCopy)));
    w_written(c, who);
    HIPCK(c, hipMemcpyAsync(c->io_tab, tab.data(), sizeof(SiteCopy) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    TCK(launch_sites_gather(c, c->io_tab, count, nblocks));
    SYNCK(c, c->stream);                                        // (tab leaves scope with this call)
    for (int k = 0; k < count; ++k) {
        const int j = sites[k];
        c->W[j].placed = false;
        for (int b = j - 1; b <= j; ++b) if (b >= 1 && b < (int)c->bond_hist.size()) c->bond_hist[b] = tnml_ctx::BondHist();
    }
    c->currb = -1; c->p_valid = false; c->sweep_start = false;
    return 0;
}
int tnml_get_site_dev(tnml_ctx* c, int j, double* A_dev, void* stream) {
    if (!c || !A_dev) return tnml_fail(c, "tnml_get_site_dev: null argument");
    if (j < 1 || j > c->N || !c->W[j].set) return tnml_fail(c, "tnml_get_site: site %d not set", j);
    const SiteT& s = c->W[j];
    const size_t bytes = sizeof(double) * (size_t)s.ml * 2 * s.mr * s.L;
    TCK(dev_check_args(c, "tnml_get_site_dev", {{"A_dev", A_dev, bytes, 8, true}}));
    TCK(dev_entry_wait(c, "tnml_get_site_dev", stream));
    HIPCK(c, hipMemcpyAsync(A_dev, s.a, bytes, hipMemcpyDeviceToDevice, c->stream));
    SYNCK(c, c->stream);
    return 0;
}
int check_W(tnml_ctx* c) {
    for (int j = 1; j <= c->N; ++j) {
        if (!c->W[j].set) return tnml_fail(c, "W: site %d not set", j);
        if (j > 1 && c->W[j].ml != c->W[j - 1].mr) return tnml_fail(c, "W: bond dimension mismatch between sites %d and %d", j - 1, j);
    }
    return 0;
}
