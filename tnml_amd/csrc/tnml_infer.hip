// tnml_infer.hip -- inference: tnml_classify on the images a context holds, tnml_predict_* on images it does not.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "tnml_host.h"

// ---- inference: toverlap / fullTest (util.h:19-40,123-200) ------------------------------------------
// W_n[l] = (prod_{j<c} phi_j*A_j) * (phi_c*A_c) * (prod_{j>c} phi_j*A_j) for every local image, with rolling
// chain buffers borrowed from the environment pools (the training environments are left untouched).
int tnml_classify(tnml_ctx* c, double* weights, int32_t* pred, int64_t count[TNML_NL], int64_t nincorrect[TNML_NL]) {
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_classify"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (!c->data_set) return tnml_fail(c, "tnml_classify: image data not set");
    EnvProtect keep(c, c->currb > 0 ? c->currb - 1 : 0, c->currb > 0 ? c->currb + 2 : 0);      // the chain buffers below may evict, but not the operands of the bond that is set
    c->p_valid = false;
    TCK(check_W(c));
    EnvSlot buf[3];
    int rc = 0;
    for (int k = 0; k < 3 && !rc; ++k) rc = slot_acquire(c, buf[k], c->maxm, 1);
    auto give_back = [&]() { for (auto& b : buf) slot_release(c, b); };
    if (rc) { give_back(); return rc; }
    const int cs = c->single() ? 1 : c->c0;                // per-label variant: site 1 plays the centre, no left chain
    // right chain N -> c+1 (util.h:25-29), ping-pong between buf[0] and buf[1]
    const void* R = nullptr; int cur = 0;
    for (int j = c->N; j > cs && !rc; --j) { rc = shift_core(c, j, false, R, 1, buf[cur].ptr, false, nullptr); R = buf[cur].ptr; cur ^= 1; }
    // left chain 1 -> c-1 (util.h:32-37), ping-pong between buf[2] and the free one of the pair above
    const void* Lc = nullptr; void* lbuf[2] = {buf[2].ptr, buf[cur].ptr}; int lcur = 0;
    for (int j = 1; j < cs && !rc; ++j) { rc = shift_core(c, j, true, Lc, 1, lbuf[lcur], false, nullptr); Lc = lbuf[lcur]; lcur ^= 1; }
    // centre site: T[l][r][n] = sum_{a,s} L[a][n] phi_c[s][n] A_c[a,s,r,l], then W_n[l] = sum_r T[l][r][n] R[r][n]
    if (!rc) rc = shift_core(c, cs, true, Lc, 1, c->U, true, nullptr);
    double* tail = c->tail;
    if (!rc) {
        LdotArgs a;
        a.A = c->U; a.A_lstride = (size_t)c->W[cs].mr * c->NTp; a.Bv = R; a.a_is_env = 0;
        a.mq = c->W[cs].mr; a.NTp = c->NTp; a.label = c->label; a.nl = c->nl(); a.target = c->target();
        a.P = c->P; a.dP = nullptr; a.mode = LD_MODE_COST;
        rc = launch_labeldot(c, a, tail);
    }
    give_back();
    if (rc) return rc;
    std::vector<char> h((size_t)TNML_NL * c->NTp * c->esz());
    std::vector<int> lab(c->NTp);
    SYNCK(c, c->stream);
    HIPCK(c, hipMemcpy(h.data(), c->P, h.size(), hipMemcpyDeviceToHost));
    HIPCK(c, hipMemcpy(lab.data(), c->label, sizeof(int) * c->NTp, hipMemcpyDeviceToHost));
    HIPCK(c, hipMemsetAsync(tail, 0, sizeof(double) * TNML_NSCAL_AR, c->stream));
    if (count) for (int l = 0; l < TNML_NL; ++l) count[l] = 0;
    if (nincorrect) for (int l = 0; l < TNML_NL; ++l) nincorrect[l] = 0;
    const int nl = c->nl();
    for (int i = 0; i < c->NT; ++i) {
        double w[TNML_NL];
        for (int l = 0; l < nl; ++l) {
            const size_t k = (size_t)l * c->NTp + i;
            w[l] = c->f64() ? ((const double*)h.data())[k] : (double)((const float*)h.data())[k];
            if (weights) weights[(size_t)i * nl + l] = w[l];
        }
        bool wrong;
        if (c->single()) {                                         // decision function f(x): pred = [f > 1/2]
            const int pl = w[0] > 0.5 ? 1 : 0;
            if (pred) pred[i] = pl;
            wrong = pl != (lab[i] == c->target() ? 1 : 0);
        } else {
            int pl = 0; double best = std::fabs(w[0]);             // argmax of |W_l|, first maximum (util.h:42-57,160-163)
            for (int l = 1; l < TNML_NL; ++l) if (std::fabs(w[l]) > best) { best = std::fabs(w[l]); pl = l; }
            if (pred) pred[i] = pl;
            wrong = pl != lab[i];
        }
        if (count) count[lab[i]] += 1;
        if (nincorrect && wrong) nincorrect[lab[i]] += 1;
    }
    return 0;
}

// ---- streamed calls: images the context does not hold (util.h:19-40 toverlap + argmax, util.h:42-57) ----------
// tnml_predict_* / tnml_evaluate_*, tnml_response_* and tnml_site_gradient_* cut the n images into chunks of their chunk option; a chunk is
// staged (copy + the input map's block sums or one transposing pre-kernel), contracted by the call's own launches and copied back, with one
// synchronisation per chunk.  They read W only: no training data, environment, bond plan, P or p_valid is touched, no collective is entered.
// Each has a workspace of its own (tnml_ctx::pk, rs, sg; tnml.h has the sizes), allocated by its first call; what the three share is
// written once, here.
static int ws_alloc(tnml_ctx* c, StreamWs& s, void** p, size_t bytes) {
    TCK(dalloc(c, p, bytes));
    s.bytes += (int64_t)bytes;
    return 0;
}
// frees every buffer the workspace names (synchronise first) and starts it over: no pointer, size or capacity survives
template <typename W>
static void ws_release(tnml_ctx* c, W& s) {
    for (const auto& list : {s.buffers(), s.own()})
        for (void** p : list) if (*p) (void)hipFree(*p);
    c->bytes -= s.bytes;
    s = W();
    if (!c->pk.bytes && !c->rs.bytes && !c->sg.bytes) io_release(c);     // the last streamed workspace has gone: what the _dev calls keep goes with it
}
void predict_release(tnml_ctx* c) { ws_release(c, c->pk); }
void response_release(tnml_ctx* c) { ws_release(c, c->rs); }
void sitegrad_release(tnml_ctx* c) { tape_kill(c, "a release of the gradient workspace"); ws_release(c, c->sg); }
// the check block and the entry event of the tnml_*_dev calls (made by the first such call; the next one makes them again)
void io_release(tnml_ctx* c) {
    if (c->io_blk) { (void)hipFree(c->io_blk); c->io_blk = nullptr; c->bytes -= 3 * (int64_t)sizeof(unsigned long long); }
    if (c->io_tab) { (void)hipFree(c->io_tab); c->io_tab = nullptr; c->bytes -= (int64_t)c->N * (int64_t)sizeof(SiteCopy); }
    if (c->io_ev) { (void)hipEventDestroy(c->io_ev); c->io_ev = nullptr; }
}
// the part of the predict workspace that follows the input map: released by tnml_set_input_map, re-made by the next tnml_predict_u8 under a map
void predict_release_map(tnml_ctx* c) {
    for (void** p : {(void**)&c->pk.mraw, (void**)&c->pk.codes, (void**)&c->pk.mtab, (void**)&c->pk.f32.mtab32}) if (*p) { (void)hipFree(*p); *p = nullptr; }
    const int64_t freed = c->pk.map_bytes + c->pk.f32.mtab32_bytes;        // (the fp32 copy of the table: 8 ncodes bytes)
    c->bytes -= freed; c->pk.bytes -= freed;
    c->pk.map_bytes = 0; c->pk.f32.mtab32_bytes = 0;
}
// First call, or the chunk option has changed since: the old workspace goes (release), tab, w and pred are made for the new capacity;
// *fresh then tells the caller to allocate what it alone has.  On an error here and in the helpers below the caller releases the workspace.
static int ws_remake(tnml_ctx* c, StreamWs& s, int chunk, void (*release)(tnml_ctx*), bool* fresh) {
    const int cap = (chunk + 63) / 64 * 64;
    *fresh = s.cap != cap;
    if (!*fresh) return 0;
    if (s.bytes) { HIPCK(c, hipStreamSynchronize(c->stream)); release(c); }
    TCK(ws_alloc(c, s, (void**)&s.tab, (size_t)c->N * sizeof(ChainSite<double>)));
    TCK(ws_alloc(c, s, (void**)&s.w, (size_t)cap * c->nl() * sizeof(double)));
    TCK(ws_alloc(c, s, (void**)&s.pred, (size_t)cap * sizeof(int)));
    s.cap = cap;
    return 0;
}
// Buffers that follow W (a tape, the gradient): each holds *have units of `unit` bytes and is re-made for `want` units when W has grown
static int ws_grow(tnml_ctx* c, StreamWs& s, size_t want, size_t* have, size_t unit, std::initializer_list<double**> bufs) {
    if (want <= *have) return 0;
    for (double** p : bufs)
        if (*p) {
            HIPCK(c, hipStreamSynchronize(c->stream));
            (void)hipFree(*p); *p = nullptr;
            c->bytes -= (int64_t)(*have * unit); s.bytes -= (int64_t)(*have * unit);
        }
    *have = 0;
    for (double** p : bufs) TCK(ws_alloc(c, s, (void**)p, want * unit));
    *have = want;
    return 0;
}
// The staging buffers of the call's input form, made by the first call of that form.  Under an input map S C + 2 N C + 16 ncodes bytes: the
// bytes as given, the block sums site-first, the fp64 table (uploaded here).  f32: the site-first features are those of the fp32 side.
// k.dev (the arrays of the call are device memory): the stage kernels read the caller's array, so the buffer the images are copied into
// (mraw, raw8, rawphi) is left out; the first host-pointer call of that form makes it
static int ws_staging(tnml_ctx* c, StreamWs& s, const StreamCall& k, bool f32 = false) {
    const size_t cap = s.cap, N = c->N;
    const bool bytes_form = k.bytes_form(), dev = k.dev;
    const char* who = k.who;
    if (bytes_form && c->im_set) {
        const size_t S = (size_t)c->im.src_rows * c->im.src_cols, tabb = c->im_table.size() * sizeof(double);
        if (!dev && !s.mraw) TCK(ws_alloc(c, s, (void**)&s.mraw, S * cap));
        if (s.codes) return 0;
        TCK(ws_alloc(c, s, (void**)&s.codes, cap * N * sizeof(uint16_t)));
        TCK(ws_alloc(c, s, (void**)&s.mtab, tabb));
        if (hipMemcpyAsync(s.mtab, c->im_table.data(), tabb, hipMemcpyHostToDevice, c->stream) != hipSuccess) return tnml_fail(c, "%s: copy of the input map's table failed", who);
        if (hipStreamSynchronize(c->stream) != hipSuccess) return tnml_fail(c, "%s: hipStreamSynchronize failed", who);
        return 0;
    }
    if (bytes_form && !dev && !s.raw8) TCK(ws_alloc(c, s, (void**)&s.raw8, cap * N));
    if (bytes_form && !s.x8) TCK(ws_alloc(c, s, (void**)&s.x8, cap * N));
    if (!bytes_form && !dev && !s.rawphi) TCK(ws_alloc(c, s, (void**)&s.rawphi, 2 * cap * N * sizeof(double)));
    if (!bytes_form && !f32 && !s.xphi) TCK(ws_alloc(c, s, (void**)&s.xphi, 2 * cap * N * sizeof(double)));
    if (!bytes_form && f32 && !s.f32.xphi32) TCK(ws_alloc(c, s, (void**)&s.f32.xphi32, 2 * cap * N * sizeof(float)));
    return 0;
}
// what every entry point checks before anything else: a call on n > 0 images has been given them
static int images_given(tnml_ctx* c, const StreamCall& k) {
    return k.n > 0 && !k.has_images() ? tnml_fail(c, "%s: null argument", k.who) : 0;
}
// The refusals every streamed call goes on with, in this order.  fp64_only: what the call computes when it serves predict_dtype = 0 alone
// (null: tnml_predict_* / tnml_evaluate_*, which take fp32 too); *maxbond: the largest bond of W
// grad: the call follows option gradient_dtype (the gradient, backward and step calls); under fp32 its bond cap is the fp32 chain kernel's
static int streamed_refusals(tnml_ctx* c, const StreamCall& k, const char* fp64_only, int* maxbond, bool grad = false) {
    const char* who = k.who;
    const int64_t n = k.n;
    if (!c) return tnml_fail(c, "%s: null argument", who);
    if (n < 0) return tnml_fail(c, "%s: n = %lld, must be >= 0", who, (long long)n);
    if (c->pend_count > 0) return tnml_fail(c, "%s: a bond update is in flight (tnml_bond_update_end first)", who);
    TCK(ho_locked(c, who));                                     // attached as a held-out set: its W is rewritten from the training context's stream, as tnml_classify refuses it
    TCK(check_W(c));
    int mb = 1;
    for (int j = 1; j <= c->N; ++j) mb = std::max(mb, std::max(c->W[j].ml, c->W[j].mr));
    const bool f32 = (!fp64_only && c->predict_dtype == TNML_PREDICT_F32) || (grad && c->gradient_dtype == TNML_GRADIENT_F32);
    if (f32 && mb > TNML_CHAIN32_MAXM)
        return tnml_fail(c, "%s: W has a bond of dimension %d, the fp32 chain kernel serves bond dimensions up to %d: use tnml_classify on a context that holds the images", who, mb, TNML_CHAIN32_MAXM);
    if (!f32 && mb > TNML_CHAIN_MAXM)
        return tnml_fail(c, "%s: W has a bond of dimension %d, the chain kernel serves bond dimensions up to %d: use tnml_classify on a context that holds the images", who, mb, TNML_CHAIN_MAXM);
    if (fp64_only && c->predict_dtype != TNML_PREDICT_F64)
        return tnml_fail(c, "%s: option predict_dtype = %d (fp32): %s are computed in fp64 only (set predict_dtype = 0)", who, c->predict_dtype, fp64_only);
    *maxbond = mb;
    return 0;
}
// the site table of W as it is now, on its way to s.tab: the caller synchronises before tab leaves scope
static int upload_sites(tnml_ctx* c, const StreamWs& s, std::vector<ChainSite<double>>& tab) {
    tab.resize(c->N);
    for (int j = 1; j <= c->N; ++j) tab[j - 1] = ChainSite<double>{c->W[j].a, c->W[j].ml, c->W[j].mr};
    HIPCK(c, hipMemcpyAsync(s.tab, tab.data(), sizeof(ChainSite<double>) * c->N, hipMemcpyHostToDevice, c->stream));
    return 0;
}
// what the kernels of element type E read in a workspace: the site table, the input map's table and the site-first features of a chunk --
// the fp64 ones, or those of the fp32 side
template <typename E> static const ChainSite<E>* sites(const StreamWs& s) { if constexpr (sizeof(E) == sizeof(float)) return s.f32.tab32; else return s.tab; }
template <typename E> static const E* table(const StreamWs& s) { if constexpr (sizeof(E) == sizeof(float)) return s.f32.mtab32; else return s.mtab; }
template <typename E> static E* xphi(const StreamWs& s) { if constexpr (sizeof(E) == sizeof(float)) return s.f32.xphi32; else return s.xphi; }
// what a chain kernel takes from the context and the workspace: the centre tnml_classify takes, the results of a chunk and the source of the
// features -- block sums with the table (input map), bytes, or staged features; fp32: the range flag
template <typename E>
static void chain_args(const tnml_ctx* c, const StreamWs& s, bool bytes_form, ChainArgs<E>& a) {
    a.sites = sites<E>(s); a.N = c->N; a.cs = c->single() ? 1 : c->c0; a.nl = c->nl(); a.single = c->single() ? 1 : 0;
    a.ld = s.cap; a.wout = s.w; a.pred = s.pred;
    a.xT = nullptr; a.phiT = nullptr;
    if (bytes_form && c->im_set) { a.codeT = s.codes; a.table = table<E>(s); }
    else if (bytes_form) a.xT = s.x8;
    else a.phiT = xphi<E>(s);
    if constexpr (sizeof(E) == sizeof(float)) a.flag = s.f32.flag;
}
// the shared part of the range-flag refusal of the fp32 calls (option: predict_dtype or gradient_dtype): the flag goes down again, the
// call fails.  Where the flag is read back is the caller's: predict reads it with the chunk's results, the gradient loop before dphi leaves
static int left_fp32_range(tnml_ctx* c, const StreamWs& s, const char* who, const char* option, int64_t off, int cnt) {
    HIPCK(c, hipMemsetAsync(s.f32.flag, 0, sizeof(int), c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return tnml_fail(c, "%s: %s = 1 (fp32): a weight of images %lld..%lld is not finite, the chain has left the fp32 range: use fp64 (%s = 0)", who, option, (long long)off, (long long)off + cnt - 1, option);
}
// tape regions (kernels_response.hip, kernels_sitegrad.hip): the vector on bond b = 0..N (dimension 1 at the two ends) starts at row
// rowoff[b]; rowoff[N + 1] and the return value: the rows so far
static int tape_rows(const tnml_ctx* c, std::vector<int>& rowoff) {
    int rows = 0;
    for (int b = 0; b <= c->N; ++b) { rowoff[b] = rows; rows += ru16(b == 0 ? 1 : c->W[b].mr); }
    return rowoff[c->N + 1] = rows;
}
// the end of a chunk: weights and pred of images off .. off + cnt - 1 to the caller, then the synchronisation after which the staging buffers are reused
// (device-resident arrays: the kernels have written them where the caller wants them, see chunk_dest)
static int chunk_results(tnml_ctx* c, const StreamWs& s, const StreamCall& k, int64_t off, int cnt) {
    const int nl = c->nl();
    if (k.dev) { SYNCK(c, c->stream); return 0; }
    if (k.weights) HIPCK(c, hipMemcpyAsync(k.weights + (size_t)off * nl, s.w, sizeof(double) * (size_t)cnt * nl, hipMemcpyDeviceToHost, c->stream));
    if (k.pred) HIPCK(c, hipMemcpyAsync(k.pred + off, s.pred, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
    SYNCK(c, c->stream);
    return 0;
}
// where the kernels of a chunk leave weights and pred: the workspace, or -- device-resident arrays -- the caller's arrays at the chunk's offset
static void chunk_dest(const tnml_ctx* c, const StreamWs& s, const StreamCall& k, int64_t off, double** wout, int** pout) {
    *wout = k.dev && k.weights ? k.weights + (size_t)off * c->nl() : s.w;
    *pout = k.dev && k.pred ? k.pred + off : s.pred;
}
// One chunk's way from the caller's arrays into the staging buffers of a workspace: copy in, then the input map's block sums (sg: its
// geometry) or one transposing pre-kernel; images off .. off + cnt - 1.  Device-resident arrays: no copy, the same kernel reads the
// caller's array at the chunk's offset
template <typename E>
static int stage_chunk(tnml_ctx* c, const StreamWs& b, const StreamCall& k, const StageGeom& sg, int64_t off, int cnt) {
    const bool bytes_form = k.bytes_form(), mapped = bytes_form && c->im_set;
    const size_t per_img = mapped ? (size_t)sg.S : (size_t)c->N * (bytes_form ? 1 : 2 * sizeof(double));
    if (k.dev) {
        if (mapped) { ProfScope ps(c, KC_PACK); return launch_stage_codes(c, k.pixels + (size_t)off * per_img, sg, cnt, b.cap, b.codes); }
        const size_t at = (size_t)off * c->N * 2;
        return launch_chain_stage<E>(c, bytes_form ? k.pixels + (size_t)off * c->N : nullptr, k.phi ? k.phi + at : nullptr, c->N, cnt, b.cap, b.x8, xphi<E>(b), k.phi32 ? k.phi32 + at : nullptr);
    }
    if (mapped) {
        HIPCK(c, hipMemcpyAsync(b.mraw, k.pixels + (size_t)off * per_img, per_img * cnt, hipMemcpyHostToDevice, c->stream));
        ProfScope ps(c, KC_PACK);
        return launch_stage_codes(c, b.mraw, sg, cnt, b.cap, b.codes);
    }
    if (bytes_form) HIPCK(c, hipMemcpyAsync(b.raw8, k.pixels + (size_t)off * c->N, per_img * cnt, hipMemcpyHostToDevice, c->stream));
    else            HIPCK(c, hipMemcpyAsync(b.rawphi, k.phi + (size_t)off * c->N * 2, per_img * cnt, hipMemcpyHostToDevice, c->stream));
    return launch_chain_stage<E>(c, bytes_form ? b.raw8 : nullptr, bytes_form ? nullptr : b.rawphi, c->N, cnt, b.cap, b.x8, xphi<E>(b));
}

// ---- device-resident arguments: what a tnml_*_dev call does where the host-pointer call walks its arrays on the CPU ----------
// The arguments of the call as the runtime must know them (dev_check_args: nothing is launched or allocated before every one has
// passed), then the entry wait on the caller's stream, then ONE k_check_batch launch over labels / coef / which -- every call makes
// it, so that a device call is the host call's launches plus exactly this one; with none of the three arrays it has nothing to walk and
// its block is not read back -- and the refusal in the host path's words.  The block is made by the first call, after the pointer checks.
static size_t sitegrad_layout(tnml_ctx* c, long long* off);
static int dev_enter(tnml_ctx* c, StreamCall& k) {
    if (k.entered) return 0;
    const char* who = k.who;
    const int32_t *labels = k.labels, *which = k.which;
    const double* coef = k.coef;
    const size_t N = c->N, nl = c->nl(), un = (size_t)k.n;
    const size_t per_img = c->im_set ? (size_t)c->im.src_rows * c->im.src_cols : N;
    TCK(dev_check_args(c, who, {
        {"pixels", k.pixels, un * per_img, 1, false}, {"phi", k.phi, un * N * 2 * sizeof(double), 8, false}, {"phi32", k.phi32, un * N * 2 * sizeof(float), 4, false},
        {"labels", labels, un * sizeof(int32_t), 4, false}, {"coef", coef, un * nl * sizeof(double), 8, false}, {"which", which, un * sizeof(int32_t), 4, false},
        {"weights", k.weights, un * nl * sizeof(double), 8, true}, {"pred", k.pred, un * sizeof(int32_t), 4, true}, {"resp", k.resp, un * N * 2 * sizeof(double), 8, true},
        {"grad", k.grad, k.grad ? sitegrad_layout(c, nullptr) * sizeof(double) : 0, 8, true}, {"dphi", k.dphi, un * N * 2 * sizeof(double), 8, true},
        {"dphi32", k.dphi32, un * N * 2 * sizeof(float), 4, true}}));
    TCK(dev_entry_wait(c, who, k.stream));
    k.entered = true;
    if (!c->io_blk) TCK(dalloc(c, (void**)&c->io_blk, 3 * sizeof(unsigned long long)));
    HIPCK(c, hipMemsetAsync(c->io_blk, 0xff, 3 * sizeof(unsigned long long), c->stream));
    TCK(launch_check_batch(c, labels, coef, which, k.n, (int)nl, c->io_blk));
    if (!labels && !coef && !which) return 0;
    unsigned long long h[3];
    HIPCK(c, hipMemcpyAsync(h, c->io_blk, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    SYNCK(c, c->stream);
    if (labels && h[0] != ~0ull) {
        int32_t v = 0;
        HIPCK(c, hipMemcpy(&v, labels + h[0], sizeof(v), hipMemcpyDeviceToHost));
        return tnml_fail(c, "%s: label %d of image %lld out of range", who, v, (long long)h[0]);
    }
    if (coef && h[1] != ~0ull) return tnml_fail(c, "%s: coefficient %d of image %lld is not finite", who, (int)(h[1] % nl), (long long)(h[1] / nl));
    if (which && h[2] != ~0ull) {
        int32_t v = 0;
        HIPCK(c, hipMemcpy(&v, which + h[2], sizeof(v), hipMemcpyDeviceToHost));
        return tnml_fail(c, "%s: which = %d of image %lld out of range 0..%d", who, v, (long long)h[2], (int)nl - 1);
    }
    return 0;
}

// ---- streamed inference (kernels_chain.hip): ONE k_chain launch per chunk ----------
// the workspace: the shared part, the parked vectors, the staging of the input form (the map's part counted in pk.map_bytes, the site-first
// features in the element type of option predict_dtype) and, for tnml_evaluate_*, 4 C + sizeof(EvalAcc) bytes: the labels of a chunk and the tallies of a call
static int predict_workspace(tnml_ctx* c, const StreamCall& k, bool f32, bool evaluate) {
    PredictWs& s = c->pk;
    bool fresh;
    int rc = ws_remake(c, s, c->predict_chunk, predict_release, &fresh);
    if (!rc && fresh) {
        s.park_elems = (size_t)s.cap * ru16(std::min(c->maxm, TNML_CHAIN_MAXM));
        rc = ws_alloc(c, s, (void**)&s.park, s.park_elems * sizeof(double));
    }
    const int64_t before = s.bytes;
    if (!rc) rc = ws_staging(c, s, k, f32);
    if (k.bytes_form() && c->im_set) s.map_bytes += s.bytes - before;
    if (!rc && evaluate && !s.lab) rc = ws_alloc(c, s, (void**)&s.lab, (size_t)s.cap * sizeof(int));
    if (!rc && evaluate && !s.acc) rc = ws_alloc(c, s, (void**)&s.acc, sizeof(EvalAcc));
    if (rc) predict_release(c);
    return rc;
}
// The fp32 side of a streamed workspace s: its site table, the range flag, the copy of W (grown when W has grown) and, under an input map,
// the table rounded to fp32.  Then the copy is made: W may have changed since the last call.  release: of s, on an error; who / who_u8:
// the caller in the messages
static int workspace32(tnml_ctx* c, StreamWs& s, void (*release)(tnml_ctx*), const char* who, const char* who_u8, bool mapped, const std::vector<ChainSite<double>>& tab) {
    StreamWs32& f = s.f32;
    int rc = 0;
    if (!f.tab32) rc = ws_alloc(c, s, (void**)&f.tab32, (size_t)c->N * sizeof(ChainSite<float>));
    if (!rc && !f.flag) {
        rc = ws_alloc(c, s, (void**)&f.flag, sizeof(int));
        if (!rc && hipMemsetAsync(f.flag, 0, sizeof(int), c->stream) != hipSuccess) rc = tnml_fail(c, "%s: memset failed", who);
    }
    std::vector<size_t> off(c->N);
    size_t total = 0, largest = 0;
    for (int j = 1; j <= c->N; ++j) {
        const size_t e = (size_t)2 * tab[j - 1].ml * tab[j - 1].mr * (j == c->c0 ? c->nl() : 1);
        off[j - 1] = total; total += (e + 3) / 4 * 4; largest = std::max(largest, e);
    }
    if (!rc && total > f.w32_cap) {
        if (f.w32) {
            if (hipStreamSynchronize(c->stream) != hipSuccess) return tnml_fail(c, "%s: hipStreamSynchronize failed", who);
            (void)hipFree(f.w32); f.w32 = nullptr;
            c->bytes -= (int64_t)(f.w32_cap * sizeof(float)); s.bytes -= (int64_t)(f.w32_cap * sizeof(float)); f.w32_cap = 0;
        }
        rc = ws_alloc(c, s, (void**)&f.w32, total * sizeof(float));
        if (!rc) f.w32_cap = total;
    }
    if (!rc && mapped && !f.mtab32) {
        std::vector<float> t32(c->im_table.size());
        for (size_t i = 0; i < t32.size(); ++i) t32[i] = (float)c->im_table[i];
        const int64_t before = s.bytes;
        rc = ws_alloc(c, s, (void**)&f.mtab32, t32.size() * sizeof(float));
        if (!rc) f.mtab32_bytes = s.bytes - before;
        if (!rc && hipMemcpyAsync(f.mtab32, t32.data(), t32.size() * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = tnml_fail(c, "%s: copy of the input map's table failed", who_u8);
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = tnml_fail(c, "%s: hipStreamSynchronize failed", who_u8);
    }
    if (rc) { release(c); return rc; }
    std::vector<ChainSite<float>> t32(c->N);
    for (int j = 1; j <= c->N; ++j) t32[j - 1] = ChainSite<float>{f.w32 + off[j - 1], tab[j - 1].ml, tab[j - 1].mr};
    HIPCK(c, hipMemcpyAsync(f.tab32, t32.data(), sizeof(ChainSite<float>) * c->N, hipMemcpyHostToDevice, c->stream));
    TCK(launch_chain_pack32(c, s.tab, f.tab32, c->N, c->c0, c->nl(), largest));
    HIPCK(c, hipStreamSynchronize(c->stream));                  // (t32 leaves scope with this call)
    return 0;
}
// the chunk loop of predict_impl in the element type E of option predict_dtype: per chunk stage (map, bytes or phi), ONE chain launch, copy back;
// k.labels (tnml_evaluate_*): the chunk's labels are staged with its images and ONE k_eval_tally launch behind the chain adds its tallies to pk.acc
template <typename E>
static int predict_chunks(tnml_ctx* c, const StreamCall& k, int maxbond) {
    constexpr bool f32 = sizeof(E) == sizeof(float);
    const PredictWs& s = c->pk;
    const StageGeom sg = k.bytes_form() && c->im_set ? stage_geom(c) : StageGeom{};   // the input map: S bytes per image -> block sums -> table look-ups inside the chain kernel
    ChainArgs<E> a;
    chain_args(c, s, k.bytes_form(), a);
    // fp32: the scratch of the parked vectors is the fp64 path's: cap x ru16(min(maxm, 512)) doubles hold cap x ru16(min(maxm, 1024)) floats
    const size_t park_elems = s.park_elems * (sizeof(double) / sizeof(E));
    for (int64_t off = 0; off < k.n; off += c->predict_chunk) {
        a.cnt = (int)std::min<int64_t>(c->predict_chunk, k.n - off);
        TCK(stage_chunk<E>(c, s, k, sg, off, a.cnt));
        chunk_dest(c, s, k, off, &a.wout, &a.pred);
        if (k.labels) HIPCK(c, hipMemcpyAsync(s.lab, k.labels + off, sizeof(int32_t) * (size_t)a.cnt, k.in(), c->stream));
        TCK(launch_chain<E>(c, a, maxbond, chain_tile<E>(c, maxbond, a.cnt), (E*)s.park, park_elems));
        if (k.labels) TCK(launch_eval_tally(c, a.wout, a.pred, s.lab, a.cnt, a.nl, a.single, c->target(), s.acc, c->loss, c->loss_beta));
        int flag = 0;
        if (f32) HIPCK(c, hipMemcpyAsync(&flag, s.f32.flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        TCK(chunk_results(c, s, k, off, a.cnt));                // (the synchronisation the flag rides on)
        if (flag) return left_fp32_range(c, s, k.who, "predict_dtype", off, a.cnt);
    }
    return 0;
}
// the report of n images from the tallies the k_eval_tally launches of a call have added up (cost: the label costs in index order)
static tnml_eval_report eval_report_of(const EvalAcc& h, int64_t n) {
    tnml_eval_report r;
    memset(&r, 0, sizeof(r));
    r.n = n;
    int64_t wrong = 0;
    for (int l = 0; l < TNML_NL; ++l) {
        r.label_cost[l] = h.label_cost[l]; r.cost += h.label_cost[l];
        r.count[l] = h.count[l]; r.nincorrect[l] = h.nincorrect[l]; wrong += h.nincorrect[l];
        for (int p = 0; p < TNML_NL; ++p) r.confusion[l][p] = h.confusion[l][p];
    }
    r.ncorrect = n - wrong;
    return r;
}
// evaluate: the call is tnml_evaluate_* (labels and rep are then required when n > 0); *rep is written once, after everything has succeeded
static int predict_impl(tnml_ctx* c, StreamCall& k, bool evaluate = false, tnml_eval_report* rep = nullptr) {
    int maxbond = 1;
    TCK(images_given(c, k));
    TCK(streamed_refusals(c, k, nullptr, &maxbond));
    if (k.n == 0) { if (rep) memset(rep, 0, sizeof(*rep)); return 0; }
    if (evaluate) {
        if (!k.labels || !rep) return tnml_fail(c, "%s: null argument (labels and rep are required)", k.who);
        if (!k.dev)
            for (int64_t i = 0; i < k.n; ++i)
                if (k.labels[i] < 0 || k.labels[i] >= TNML_NL) return tnml_fail(c, "%s: label %d of image %lld out of range", k.who, k.labels[i], (long long)i);
    }
    if (k.dev) TCK(dev_enter(c, k));
    HIPCK(c, hipSetDevice(c->cfg.device));
    const bool f32 = c->predict_dtype == TNML_PREDICT_F32;
    TCK(predict_workspace(c, k, f32, evaluate));
    if (evaluate) HIPCK(c, hipMemsetAsync(c->pk.acc, 0, sizeof(EvalAcc), c->stream));
    std::vector<ChainSite<double>> tab;
    TCK(upload_sites(c, c->pk, tab));
    HIPCK(c, hipStreamSynchronize(c->stream));                  // (tab leaves scope with this call)
    if (f32) TCK(workspace32(c, c->pk, predict_release, "tnml_predict", "tnml_predict_u8", k.bytes_form() && c->im_set, tab));
    TCK(f32 ? predict_chunks<float>(c, k, maxbond) : predict_chunks<double>(c, k, maxbond));
    if (!evaluate) return 0;
    EvalAcc h;                                                  // the one copy of the tallies: every chunk has been added (the loop ends on a synchronisation)
    HIPCK(c, hipMemcpyAsync(&h, c->pk.acc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    SYNCK(c, c->stream);
    *rep = eval_report_of(h, k.n);
    return 0;
}
int tnml_predict_u8(tnml_ctx* c, int64_t n, const uint8_t* pixels, double* weights, int32_t* pred) {
    StreamCall k{"tnml_predict_u8", n, pixels};
    k.weights = weights; k.pred = pred;
    return predict_impl(c, k);
}
int tnml_predict_phi(tnml_ctx* c, int64_t n, const double* phi, double* weights, int32_t* pred) {
    StreamCall k{"tnml_predict_phi", n, nullptr, phi};
    k.weights = weights; k.pred = pred;
    return predict_impl(c, k);
}
int tnml_evaluate_u8(tnml_ctx* c, int64_t n, const uint8_t* pixels, const int32_t* labels, tnml_eval_report* rep, double* weights, int32_t* pred) {
    StreamCall k{"tnml_evaluate_u8", n, pixels};
    k.labels = labels; k.weights = weights; k.pred = pred;
    return predict_impl(c, k, true, rep);
}
int tnml_evaluate_phi(tnml_ctx* c, int64_t n, const double* phi, const int32_t* labels, tnml_eval_report* rep, double* weights, int32_t* pred) {
    StreamCall k{"tnml_evaluate_phi", n, nullptr, phi};
    k.labels = labels; k.weights = weights; k.pred = pred;
    return predict_impl(c, k, true, rep);
}

// ---- streamed site responses (kernels_response.hip): every site's effect on an image's output ---------------------
// Per chunk of option response_chunk ONE k_response launch walks the chain inward and outward, the result [N][2][C] is turned into
// [C][N][2] on the device and copied back.
// rows: the rows of a workgroup's tape slice that W asks for now
static int response_workspace(tnml_ctx* c, const StreamCall& k, size_t rows) {
    ResponseWs& s = c->rs;
    bool fresh;
    int rc = ws_remake(c, s, c->response_chunk, response_release, &fresh);
    const size_t cap = s.cap;
    if (!rc && fresh) {
        rc = ws_alloc(c, s, (void**)&s.which, cap * sizeof(int));
        if (!rc) rc = ws_alloc(c, s, (void**)&s.rowoff, (size_t)(c->N + 4) * sizeof(int));
        if (!rc) rc = ws_alloc(c, s, (void**)&s.out, 2 * c->N * cap * sizeof(double));
    }
    if (!rc && !k.dev && !s.outT) rc = ws_alloc(c, s, (void**)&s.outT, 2 * c->N * cap * sizeof(double));    // (device-resident resp: the transposition writes the caller's array)
    if (!rc) rc = ws_grow(c, s, rows, &s.tape_rows, cap * sizeof(double), {&s.tape});
    if (!rc) rc = ws_staging(c, s, k);
    if (rc) response_release(c);
    return rc;
}
static int response_impl(tnml_ctx* c, StreamCall& k) {
    int maxbond = 1;
    TCK(images_given(c, k));
    TCK(streamed_refusals(c, k, "site responses", &maxbond));
    if (k.n == 0) return 0;
    if (!k.resp) return tnml_fail(c, "%s: null argument", k.who);
    const int nl = c->nl();
    if (k.dev) TCK(dev_enter(c, k));
    else if (k.which)
        for (int64_t i = 0; i < k.n; ++i)
            if (k.which[i] < 0 || k.which[i] >= nl) return tnml_fail(c, "%s: which = %d of image %lld out of range 0..%d", k.who, k.which[i], (long long)i, nl - 1);
    HIPCK(c, hipSetDevice(c->cfg.device));
    const ResponseWs& s = c->rs;
    const int N = c->N, cs = c->single() ? 1 : c->c0;
    // the tape: the regions of the bonds, then X and Y of the centre (kernels_response.hip)
    std::vector<int> rowoff(N + 4);
    int rows = tape_rows(c, rowoff);
    rows += ru16(c->W[cs].ml);
    rowoff[N + 2] = rows; rows += ru16(c->W[cs].mr);
    rowoff[N + 3] = rows;
    TCK(response_workspace(c, k, (size_t)rows));
    std::vector<ChainSite<double>> tab;
    TCK(upload_sites(c, s, tab));
    HIPCK(c, hipMemcpyAsync(s.rowoff, rowoff.data(), sizeof(int) * (N + 4), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));                  // (tab and rowoff leave scope with this call)
    const StageGeom sg = k.bytes_form() && c->im_set ? stage_geom(c) : StageGeom{};
    RespArgs a;
    chain_args(c, s, k.bytes_form(), a.ch);
    a.which = k.which ? s.which : nullptr; a.rowoff = s.rowoff; a.tape = s.tape; a.resp = s.out;
    const size_t tape_elems = s.tape_rows * (size_t)s.cap;
    for (int64_t off = 0; off < k.n; off += c->response_chunk) {
        a.ch.cnt = (int)std::min<int64_t>(c->response_chunk, k.n - off);
        double* const resp = k.resp + (size_t)off * N * 2;
        TCK(stage_chunk<double>(c, s, k, sg, off, a.ch.cnt));
        chunk_dest(c, s, k, off, &a.ch.wout, &a.ch.pred);
        if (k.which) HIPCK(c, hipMemcpyAsync(s.which, k.which + off, sizeof(int32_t) * (size_t)a.ch.cnt, k.in(), c->stream));
        TCK(launch_response(c, a, maxbond, chain_tile<double>(c, maxbond, a.ch.cnt), rows, tape_elems, k.dev ? resp : s.outT));
        if (!k.dev) HIPCK(c, hipMemcpyAsync(resp, s.outT, sizeof(double) * (size_t)a.ch.cnt * N * 2, hipMemcpyDeviceToHost, c->stream));
        TCK(chunk_results(c, s, k, off, a.ch.cnt));
    }
    return 0;
}
int tnml_response_u8(tnml_ctx* c, int64_t n, const uint8_t* pixels, const int32_t* which, double* resp, double* weights, int32_t* pred) {
    StreamCall k{"tnml_response_u8", n, pixels};
    k.which = which; k.resp = resp; k.weights = weights; k.pred = pred;
    return response_impl(c, k);
}
int tnml_response_phi(tnml_ctx* c, int64_t n, const double* phi, const int32_t* which, double* resp, double* weights, int32_t* pred) {
    StreamCall k{"tnml_response_phi", n, nullptr, phi};
    k.which = which; k.resp = resp; k.weights = weights; k.pred = pred;
    return response_impl(c, k);
}

// ---- streamed site gradients (kernels_sitegrad.hip): dC/dA of every site, on images the context does not hold ----------------
// Per chunk of option gradient_chunk ONE k_site_backward launch walks the chain inward and outward and leaves two tapes, ONE k_site_grad
// launch adds the chunk's outer products to the gradient, which stays on the device until the last chunk and is copied back once.
// rows: the rows of a workgroup's tape slice that W asks for now; elems: the elements of the gradient of W as it is now
// f32 (option gradient_dtype = 1): the tapes hold floats -- a change of the option frees the two tapes and makes them again in the new
// element size, and touches nothing else --, the site-first features of the phi form are the fp32 ones; the fp32 copy of W follows in
// workspace32.  The first call that asks for input gradients adds their result as the kernel leaves it and as a host caller gets it
static int sitegrad_workspace(tnml_ctx* c, const StreamCall& k, size_t rows, size_t elems, bool f32) {
    GradientWs& s = c->sg;
    const int nl = c->nl();
    bool fresh;
    int rc = ws_remake(c, s, c->gradient_chunk, sitegrad_release, &fresh);
    const size_t cap = s.cap, esz = f32 ? sizeof(float) : sizeof(double);
    if (!rc && s.tape_rows && (size_t)s.esz != esz) {
        if (hipStreamSynchronize(c->stream) != hipSuccess) rc = tnml_fail(c, "%s: hipStreamSynchronize failed", k.who);
        for (double** p : {&s.tape, &s.tape2})
            if (*p) { (void)hipFree(*p); *p = nullptr; c->bytes -= (int64_t)(s.tape_rows * cap * s.esz); s.bytes -= (int64_t)(s.tape_rows * cap * s.esz); }
        s.tape_rows = 0;
    }
    s.esz = (int)esz;
    if (!rc && fresh) {
        rc = ws_alloc(c, s, (void**)&s.coef, cap * nl * sizeof(double));
        if (!rc) rc = ws_alloc(c, s, (void**)&s.lab, cap * sizeof(int));
        if (!rc) rc = ws_alloc(c, s, (void**)&s.rowoff, (size_t)(c->N + 2) * sizeof(int));
        if (!rc) rc = ws_alloc(c, s, (void**)&s.goff, (size_t)(c->N + 1) * sizeof(long long));
        if (!rc) rc = ws_alloc(c, s, (void**)&s.blk0, (size_t)(c->N + nl) * sizeof(int));
    }
    if (!rc) rc = ws_grow(c, s, rows, &s.tape_rows, cap * esz, {&s.tape, &s.tape2});
    if (!rc) rc = ws_grow(c, s, elems, &s.grad_elems, sizeof(double), {&s.grad});
    if (!rc) rc = ws_staging(c, s, k, f32);
    if (!rc && k.want_dphi() && !s.dphi) rc = ws_alloc(c, s, (void**)&s.dphi, (size_t)2 * c->N * cap * sizeof(double));
    if (!rc && k.want_dphi() && !k.dev && !s.dphiT) rc = ws_alloc(c, s, (void**)&s.dphiT, (size_t)2 * c->N * cap * sizeof(double));
    if (rc) sitegrad_release(c);
    return rc;
}
// elements of the gradient and where every site starts (off: N + 1 entries or null); W is complete
static size_t sitegrad_layout(tnml_ctx* c, long long* off) {
    size_t e = 0;
    for (int j = 1; j <= c->N; ++j) {
        if (off) off[j - 1] = (long long)e;
        e += (size_t)2 * c->W[j].ml * c->W[j].mr * c->W[j].L;
    }
    if (off) off[c->N] = (long long)e;
    return e;
}
int tnml_site_gradient_size(tnml_ctx* c, int64_t* elems, int64_t* offsets) {
    if (!c || !elems) return tnml_fail(c, "tnml_site_gradient_size: null argument");
    TCK(check_W(c));
    std::vector<long long> off(c->N + 1);
    *elems = (int64_t)sitegrad_layout(c, off.data());
    if (offsets) for (int j = 0; j <= c->N; ++j) offsets[j] = off[j];
    return 0;
}
// what a gradient call with n > 0 asks of its arrays: exactly one of labels and coef, labels in range, finite coefficients
// device-resident arrays: the same through dev_enter, once per call
static int sitegrad_inputs(tnml_ctx* c, StreamCall& k) {
    const int nl = c->nl();
    if ((k.labels != nullptr) == (k.coef != nullptr)) return tnml_fail(c, "%s: exactly one of labels and coef must be given (%s are)", k.who, k.labels ? "both" : "neither");
    if (k.dev) return dev_enter(c, k);
    if (k.labels)
        for (int64_t i = 0; i < k.n; ++i)
            if (k.labels[i] < 0 || k.labels[i] >= TNML_NL) return tnml_fail(c, "%s: label %d of image %lld out of range", k.who, k.labels[i], (long long)i);
    if (k.coef)
        for (int64_t i = 0; i < k.n * nl; ++i)
            if (!std::isfinite(k.coef[i])) return tnml_fail(c, "%s: coefficient %d of image %lld is not finite", k.who, (int)(i % nl), (long long)(i / nl));
    return 0;
}
// what sitegrad_device works out for its chunk loop, and what its caller asks for beside the arrays: acc (tnml_site_step_* in the labels
// mode), a device accumulator block that gets one k_eval_tally launch per chunk; want_grad false leaves k_site_grad out
struct SiteGradPlan { EvalAcc* acc; bool want_grad; int maxbond, rows, nblocks; };
// the chunk loop of sitegrad_device in the element type E of option gradient_dtype; the tables are on the device
template <typename E>
static int sitegrad_chunks(tnml_ctx* c, const StreamCall& k, const SiteGradPlan& g) {
    constexpr bool f32 = sizeof(E) == sizeof(float);
    GradientWs& s = c->sg;
    const int N = c->N, nl = c->nl(), cs = c->single() ? 1 : c->c0;
    const StageGeom sg = k.bytes_form() && c->im_set ? stage_geom(c) : StageGeom{};
    SiteGradArgsT<E> a;
    chain_args(c, s, k.bytes_form(), a.ch);
    a.rowoff = s.rowoff; a.tape = (E*)s.tape; a.tape2 = (E*)s.tape2;
    a.lab = k.labels ? s.lab : nullptr; a.target = c->target(); a.coef = s.coef;
    a.grad = s.grad; a.goff = s.goff; a.blk0 = s.blk0;
    a.loss = k.labels ? c->loss : TNML_LOSS_QUADRATIC; a.beta = c->loss_beta;      // (coefficients as given know no loss)
    const size_t tape_elems = s.tape_rows * (size_t)s.cap;
    for (int64_t off = 0; off < k.n; off += c->gradient_chunk) {
        a.ch.cnt = (int)std::min<int64_t>(c->gradient_chunk, k.n - off);
        TCK(stage_chunk<E>(c, s, k, sg, off, a.ch.cnt));
        chunk_dest(c, s, k, off, &a.ch.wout, &a.ch.pred);
        if (k.labels) HIPCK(c, hipMemcpyAsync(s.lab, k.labels + off, sizeof(int32_t) * (size_t)a.ch.cnt, k.in(), c->stream));
        else          HIPCK(c, hipMemcpyAsync(s.coef, k.coef + (size_t)off * nl, sizeof(double) * (size_t)a.ch.cnt * nl, k.in(), c->stream));
        const int T = chain_tile<E>(c, g.maxbond, a.ch.cnt);
        TCK(launch_site_gradient<E>(c, a, g.maxbond, T, g.rows, tape_elems, g.nblocks, g.want_grad));
        if constexpr (f32) {                                       // the range flag, before anything of the chunk reaches the caller
            int flag = 0;
            HIPCK(c, hipMemcpyAsync(&flag, s.f32.flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
            SYNCK(c, c->stream);
            if (flag) return left_fp32_range(c, s, k.who, "gradient_dtype", off, a.ch.cnt);
        }
        if (k.want_dphi()) {
            InputGradArgsT<E> ig;
            ig.sites = sites<E>(s); ig.N = N; ig.cs = cs; ig.nl = nl; ig.ld = s.cap; ig.cnt = a.ch.cnt;
            ig.rowoff = s.rowoff; ig.tape = (const E*)s.tape; ig.tape2 = (const E*)s.tape2; ig.coef = s.coef; ig.dphi = s.dphi;
            const size_t at = (size_t)off * N * 2;
            if (k.dev) TCK(launch_input_grad<E>(c, ig, g.maxbond, T, g.rows, tape_elems, k.dphi ? k.dphi + at : nullptr, k.dphi ? nullptr : k.dphi32 + at));
            else {
                TCK(launch_input_grad<E>(c, ig, g.maxbond, T, g.rows, tape_elems, s.dphiT));
                HIPCK(c, hipMemcpyAsync(k.dphi + at, s.dphiT, sizeof(double) * (size_t)a.ch.cnt * N * 2, hipMemcpyDeviceToHost, c->stream));
            }
        }
        if (g.acc && k.labels) TCK(launch_eval_tally(c, a.ch.wout, a.ch.pred, s.lab, a.ch.cnt, nl, a.ch.single, c->target(), g.acc, c->loss, c->loss_beta));
        s.last_cnt = a.ch.cnt;
        TCK(chunk_results(c, s, k, off, a.ch.cnt));
    }
    return 0;
}
// W as the gradient kernels need it known: the Label site's extent, the gradient's layout -> goff (N + 1 entries), its elements
static int sitegrad_shape(tnml_ctx* c, const char* who, std::vector<long long>& goff, size_t* elems) {
    const int nl = c->nl(), cs = c->single() ? 1 : c->c0;
    if (c->W[cs].L != nl) return tnml_fail(c, "%s: the Label site %d of W carries %d labels, the context has %d", who, cs, c->W[cs].L, nl);
    goff.resize(c->N + 1);
    *elems = sitegrad_layout(c, goff.data());
    return 0;
}
// What a call on n > 0 images sets up in the gradient workspace before its chunk loop: the plan's rows and output blocks, the workspace
// itself, the site table and the three small tables on the device, the gradient zeroed, the fp32 side under gradient_dtype = 1.  The
// live ticket of a taped forward dies here: its tape is about to be written.
static int sitegrad_prepare(tnml_ctx* c, const StreamCall& k, SiteGradPlan& g, const std::vector<long long>& goff, size_t elems) {
    const int N = c->N, nl = c->nl(), cs = c->single() ? 1 : c->c0;
    tape_kill(c, k.who);
    HIPCK(c, hipSetDevice(c->cfg.device));
    const GradientWs& s = c->sg;
    std::vector<int> rowoff(N + 2);                             // both tapes share the region table (kernels_sitegrad.hip)
    g.rows = tape_rows(c, rowoff);
    // output blocks of 32 x 32 per virtual site: the sites in order, the Label site once per label
    std::vector<int> blk0(N + nl);
    int v = 0;
    for (int j = 1; j <= N; ++j) {
        const int nb = ((c->W[j].ml + 31) / 32) * ((c->W[j].mr + 31) / 32);
        for (int l = 0; l < (j == cs ? nl : 1); ++l) { blk0[v++] = g.nblocks; g.nblocks += nb; }
    }
    blk0[v] = g.nblocks;
    const bool f32 = c->gradient_dtype == TNML_GRADIENT_F32;
    TCK(sitegrad_workspace(c, k, (size_t)g.rows, elems, f32));
    std::vector<ChainSite<double>> tab;
    TCK(upload_sites(c, s, tab));
    HIPCK(c, hipMemcpyAsync(s.rowoff, rowoff.data(), sizeof(int) * (N + 2), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(s.goff, goff.data(), sizeof(long long) * (N + 1), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(s.blk0, blk0.data(), sizeof(int) * (N + nl), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemsetAsync(s.grad, 0, elems * sizeof(double), c->stream));       // the sum starts from zero: grad is overwritten
    if (g.acc) HIPCK(c, hipMemsetAsync(g.acc, 0, sizeof(EvalAcc), c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));                  // (the tables leave scope with this call)
    if (f32) TCK(workspace32(c, c->sg, sitegrad_release, k.who, k.who, k.bytes_form() && c->im_set, tab));
    return 0;
}
// The part the gradient calls and the step calls share: refusals, staging, tables and the chunk loop.  It leaves the gradient of the n
// images in c->sg.grad (*elems_out of them) with the stream synchronised behind the last chunk; n = 0: nothing is launched, *elems_out
// alone is set.  A call that would leave nothing anywhere (tnml_site_gradient_* without grad) is refused.  acc is zeroed here.
// tnml_backward_*: k.dphi (or k.dphi32) receives the input gradients [n][N][2] chunk by chunk, from ONE k_input_grad launch behind the
// chunk's k_site_backward; device-resident arrays receive the transposition directly.  k.grad enters the pointer checks only: the sum
// is made in sg.grad as ever, and the caller copies it out.
static int sitegrad_device(tnml_ctx* c, StreamCall& k, EvalAcc* acc, bool want_grad, size_t* elems_out) {
    SiteGradPlan g{acc, want_grad, 1, 0, 0};
    TCK(streamed_refusals(c, k, "site gradients", &g.maxbond, true));
    if (!k.grad && !k.want_dphi() && !acc) return tnml_fail(c, "%s: null argument", k.who);
    std::vector<long long> goff;
    TCK(sitegrad_shape(c, k.who, goff, elems_out));
    if (k.n == 0) return 0;
    TCK(sitegrad_inputs(c, k));
    TCK(sitegrad_prepare(c, k, g, goff, *elems_out));
    return c->gradient_dtype == TNML_GRADIENT_F32 ? sitegrad_chunks<float>(c, k, g) : sitegrad_chunks<double>(c, k, g);
}
static int sitegrad_impl(tnml_ctx* c, StreamCall& k) {
    size_t elems = 0;
    TCK(images_given(c, k));
    TCK(sitegrad_device(c, k, nullptr, true, &elems));
    if (k.n == 0) { memset(k.grad, 0, elems * sizeof(double)); return 0; }
    HIPCK(c, hipMemcpyAsync(k.grad, c->sg.grad, elems * sizeof(double), hipMemcpyDeviceToHost, c->stream));   // the one copy of the gradient
    SYNCK(c, c->stream);
    return 0;
}
int tnml_site_gradient_u8(tnml_ctx* c, int64_t n, const uint8_t* pixels, const int32_t* labels, const double* coef, double* grad, double* weights, int32_t* pred) {
    StreamCall k{"tnml_site_gradient_u8", n, pixels};
    k.labels = labels; k.coef = coef; k.grad = grad; k.weights = weights; k.pred = pred;
    return sitegrad_impl(c, k);
}
int tnml_site_gradient_phi(tnml_ctx* c, int64_t n, const double* phi, const int32_t* labels, const double* coef, double* grad, double* weights, int32_t* pred) {
    StreamCall k{"tnml_site_gradient_phi", n, nullptr, phi};
    k.labels = labels; k.coef = coef; k.grad = grad; k.weights = weights; k.pred = pred;
    return sitegrad_impl(c, k);
}

// ---- streamed input gradients (kernels_inputgrad.hip): dC/dphi of every site of every image, beside or instead of dC/dA ----------------
// The gradient call's refusals, workspace, staging and k_site_backward launch; per chunk k_site_grad runs when grad is asked for and ONE
// k_input_grad launch on the two tapes when dphi is, its result transposed on the device and copied back with the chunk.
static int backward_impl(tnml_ctx* c, StreamCall& k) {
    TCK(images_given(c, k));
    if (c && !k.grad && !k.want_dphi()) return tnml_fail(c, "%s: grad and dphi are both NULL: the call would compute nothing", k.who);
    size_t elems = 0;
    TCK(sitegrad_device(c, k, nullptr, k.grad != nullptr, &elems));
    double* const grad = k.grad;
    if (k.n == 0) {
        if (grad && !k.dev) memset(grad, 0, elems * sizeof(double));
        if (grad && k.dev) {                                    // (no chunk has run: the checks of the one array the call touches, made here)
            TCK(dev_check_args(c, k.who, {{"grad", grad, elems * sizeof(double), 8, true}}));
            TCK(dev_entry_wait(c, k.who, k.stream));
            HIPCK(c, hipMemsetAsync(grad, 0, elems * sizeof(double), c->stream));
            SYNCK(c, c->stream);
        }
        return 0;
    }
    if (!grad) return 0;                                        // (the chunk loop ends on a synchronisation)
    HIPCK(c, hipMemcpyAsync(grad, c->sg.grad, elems * sizeof(double), k.dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    SYNCK(c, c->stream);
    return 0;
}
int tnml_backward_u8(tnml_ctx* c, int64_t n, const uint8_t* pixels, const int32_t* labels, const double* coef, double* grad, double* dphi, double* weights, int32_t* pred) {
    StreamCall k{"tnml_backward_u8", n, pixels};
    k.labels = labels; k.coef = coef; k.grad = grad; k.dphi = dphi; k.weights = weights; k.pred = pred;
    return backward_impl(c, k);
}
int tnml_backward_phi(tnml_ctx* c, int64_t n, const double* phi, const int32_t* labels, const double* coef, double* grad, double* dphi, double* weights, int32_t* pred) {
    StreamCall k{"tnml_backward_phi", n, nullptr, phi};
    k.labels = labels; k.coef = coef; k.grad = grad; k.dphi = dphi; k.weights = weights; k.pred = pred;
    return backward_impl(c, k);
}

// ---- gradient steps on the device (kernels_sitestep.hip): the gradient above, then ONE optimiser step on W where it lies ----------------
// The optimiser state (the st_ fields of tnml_ctx) is no part of the workspace `sg`: tnml.h has its size.
void step_release(tnml_ctx* c) {
    for (void** p : {(void**)&c->st_m, (void**)&c->st_v, (void**)&c->st_bsum, (void**)&c->st_res, (void**)&c->st_wg0, (void**)&c->st_acc})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    c->bytes -= c->st_bytes;
    c->st_bytes = 0; c->st_method = -1; c->st_shape.clear(); c->st_elems = 0; c->st_nblk = 0; c->st_nwg = 0;
    c->st_t = 0; c->st_p1 = 1.; c->st_p2 = 1.;
}
int tnml_site_step_reset(tnml_ctx* c) {
    if (!c) return tnml_fail(c, "tnml_site_step_reset: null argument");
    if (c->st_method < 0) return 0;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipStreamSynchronize(c->stream));
    step_release(c);
    return 0;
}
static const char* step_method_name(int m) { return m == TNML_STEP_ADAM ? "adam" : "sgd"; }
// The state for `method` and W as it is now (complete): made by the first step, zeroed; afterwards the method and every site's shape must be those it was made for
static int step_state_for(tnml_ctx* c, const char* who, int method) {
    const int N = c->N;
    if (c->st_method >= 0) {
        if (c->st_method != method)
            return tnml_fail(c, "%s: the optimiser state was made for method %s, this step asks for %s (tnml_site_step_reset first)", who, step_method_name(c->st_method), step_method_name(method));
        for (int j = 1; j <= N; ++j)
            if (c->st_shape[3 * (j - 1)] != c->W[j].ml || c->st_shape[3 * (j - 1) + 1] != c->W[j].mr || c->st_shape[3 * (j - 1) + 2] != c->W[j].L)
                return tnml_fail(c, "%s: site %d of W is %d x 2 x %d now, the optimiser state was made for %d x 2 x %d (tnml_site_step_reset first)", who, j,
                                 c->W[j].ml, c->W[j].mr, c->st_shape[3 * (j - 1)], c->st_shape[3 * (j - 1) + 1]);
        return 0;
    }
    std::vector<int> wg0(N + 1);
    int nwg = 0;
    for (int j = 1; j <= N; ++j) {
        wg0[j - 1] = nwg;
        nwg += (int)(((size_t)2 * c->W[j].ml * c->W[j].mr * c->W[j].L + STEP_WG_ELEMS - 1) / STEP_WG_ELEMS);
    }
    wg0[N] = nwg;
    const size_t E = sitegrad_layout(c, nullptr);
    const int nblk = (int)((E + STEP_NORM_BLOCK - 1) / STEP_NORM_BLOCK);
    auto alloc = [&](void** p, size_t bytes) { int rc = dalloc(c, p, bytes); if (!rc) c->st_bytes += (int64_t)bytes; return rc; };
    int rc = 0;
    if (method == TNML_STEP_ADAM) rc = alloc((void**)&c->st_m, E * sizeof(double));
    if (!rc) rc = alloc((void**)&c->st_v, E * sizeof(double));
    if (!rc) rc = alloc((void**)&c->st_bsum, (size_t)nblk * sizeof(double));
    if (!rc) rc = alloc((void**)&c->st_wg0, (size_t)(N + 1) * sizeof(int));
    if (!rc) rc = alloc((void**)&c->st_res, SR_N * sizeof(double));
    if (!rc) rc = alloc((void**)&c->st_acc, sizeof(EvalAcc));
    hipError_t e = hipSuccess;
    if (!rc && c->st_m) e = hipMemsetAsync(c->st_m, 0, E * sizeof(double), c->stream);
    if (!rc && e == hipSuccess) e = hipMemsetAsync(c->st_v, 0, E * sizeof(double), c->stream);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(c->st_wg0, wg0.data(), sizeof(int) * (N + 1), hipMemcpyHostToDevice, c->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(c->stream);                    // (wg0 leaves scope with this call)
    if (!rc && e != hipSuccess) rc = tnml_fail(c, "%s: setting up the optimiser state failed: %s", who, hipGetErrorString(e));
    if (rc) { step_release(c); return rc; }
    c->st_method = method; c->st_elems = E; c->st_nblk = nblk; c->st_nwg = nwg;
    c->st_shape.resize(3 * (size_t)N);
    for (int j = 1; j <= N; ++j) { c->st_shape[3 * (j - 1)] = c->W[j].ml; c->st_shape[3 * (j - 1) + 1] = c->W[j].mr; c->st_shape[3 * (j - 1) + 2] = c->W[j].L; }
    return 0;
}
static int step_check_params(tnml_ctx* c, const char* who, const tnml_step_params* p) {
    if (!p) return tnml_fail(c, "%s: null argument (the step parameters p)", who);
    if (p->method != TNML_STEP_SGD && p->method != TNML_STEP_ADAM) return tnml_fail(c, "%s: method = %d, must be TNML_STEP_SGD (0) or TNML_STEP_ADAM (1)", who, p->method);
    if (!(std::isfinite(p->lr) && p->lr > 0.)) return tnml_fail(c, "%s: lr = %g, must be finite and > 0", who, p->lr);
    if (!(std::isfinite(p->clip) && p->clip >= 0.)) return tnml_fail(c, "%s: clip = %g, must be finite and >= 0 (0: no clipping)", who, p->clip);
    if (!(std::isfinite(p->scale) && p->scale != 0.)) return tnml_fail(c, "%s: scale = %g, must be finite and non-zero", who, p->scale);
    if (p->method == TNML_STEP_SGD) {
        if (!(p->momentum >= 0. && p->momentum < 1.)) return tnml_fail(c, "%s: momentum = %g, must lie in [0, 1)", who, p->momentum);
    } else {
        if (!(p->beta1 >= 0. && p->beta1 < 1.)) return tnml_fail(c, "%s: beta1 = %g, must lie in [0, 1)", who, p->beta1);
        if (!(p->beta2 >= 0. && p->beta2 < 1.)) return tnml_fail(c, "%s: beta2 = %g, must lie in [0, 1)", who, p->beta2);
        if (!(std::isfinite(p->eps) && p->eps > 0.)) return tnml_fail(c, "%s: eps = %g, must be finite and > 0", who, p->eps);
    }
    return 0;
}
static int sitestep_impl(tnml_ctx* c, StreamCall& k, const tnml_step_params* p, tnml_step_report* rep) {
    const char* who = k.who;
    const int32_t* labels = k.labels;
    const int64_t n = k.n;
    int maxbond = 1;
    TCK(images_given(c, k));
    TCK(streamed_refusals(c, k, "site gradients", &maxbond, true));
    TCK(ho_locked(c, who, true));                               // as tnml_set_site: W of a training context with a held-out context attached changes in bond updates only
    if (c->cfg.nranks != 1) return tnml_fail(c, "%s: the context is rank %d of %d: a step enters no collective, the replicas of W would part (one rank only)", who, c->cfg.rank, c->cfg.nranks);
    TCK(step_check_params(c, who, p));
    if (n == 0) { if (rep) memset(rep, 0, sizeof(*rep)); return 0; }
    const int cs = c->single() ? 1 : c->c0;
    if (c->W[cs].L != c->nl()) return tnml_fail(c, "%s: the Label site %d of W carries %d labels, the context has %d", who, cs, c->W[cs].L, c->nl());
    TCK(sitegrad_inputs(c, k));                                 // (before the state is made: a refused call leaves nothing behind)
    HIPCK(c, hipSetDevice(c->cfg.device));
    TCK(step_state_for(c, who, p->method));
    size_t elems = 0;
    TCK(sitegrad_device(c, k, c->st_acc, true, &elems));
    if (elems != c->st_elems) return tnml_fail(c, "%s: the gradient has %zu elements, the optimiser state %zu (tnml_site_step_reset first)", who, elems, c->st_elems);
    SiteStepArgs a;
    a.sites = c->sg.tab; a.goff = c->sg.goff; a.wg0 = c->st_wg0; a.N = c->N;
    a.grad = c->sg.grad; a.elems = elems; a.m = c->st_m; a.v = c->st_v; a.bsum = c->st_bsum; a.nblk = c->st_nblk; a.res = c->st_res;
    a.method = p->method; a.lr = p->lr; a.mu = p->momentum; a.beta1 = p->beta1; a.beta2 = p->beta2; a.eps = p->eps; a.clip = p->clip; a.scale = p->scale;
    // Adam's powers: one multiplication per step, kept only when the step is applied
    const double p1 = c->st_p1 * p->beta1, p2 = c->st_p2 * p->beta2;
    a.o1 = 1. - p->beta1; a.o2 = 1. - p->beta2; a.c1 = 1. - p1; a.c2 = 1. - p2;
    w_written(c, who);
    TCK(launch_site_step(c, a, c->st_nwg));
    double res[SR_N];
    EvalAcc h;
    HIPCK(c, hipMemcpyAsync(res, c->st_res, sizeof(res), hipMemcpyDeviceToHost, c->stream));            // the report: all that crosses the bus
    if (labels) HIPCK(c, hipMemcpyAsync(&h, c->st_acc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    SYNCK(c, c->stream);
    if (res[SR_APPLIED] == 0.)
        return tnml_fail(c, "%s: the gradient is out of range (sum of squares %g, norm %g): no step was taken, W and the optimiser state are as they were", who, res[SR_TOTAL], res[SR_NORM]);
    c->st_t += 1;
    if (p->method == TNML_STEP_ADAM) { c->st_p1 = p1; c->st_p2 = p2; }
    // W has changed under the context, as by tnml_set_site on every site
    for (int j = 1; j <= c->N; ++j) c->W[j].placed = false;
    c->currb = -1; c->p_valid = false; c->sweep_start = false;
    for (auto& bh : c->bond_hist) bh = tnml_ctx::BondHist();
    if (rep) {
        memset(rep, 0, sizeof(*rep));
        rep->t = c->st_t; rep->grad_norm = res[SR_NORM]; rep->factor = res[SR_FACTOR]; rep->clipped = res[SR_CLIPPED] != 0.;
        if (labels) rep->eval = eval_report_of(h, n); else rep->eval.n = n;
    }
    return 0;
}
int tnml_site_step_u8(tnml_ctx* c, int64_t n, const uint8_t* pixels, const int32_t* labels, const double* coef, const tnml_step_params* p, tnml_step_report* rep) {
    StreamCall k{"tnml_site_step_u8", n, pixels};
    k.labels = labels; k.coef = coef;
    return sitestep_impl(c, k, p, rep);
}
int tnml_site_step_phi(tnml_ctx* c, int64_t n, const double* phi, const int32_t* labels, const double* coef, const tnml_step_params* p, tnml_step_report* rep) {
    StreamCall k{"tnml_site_step_phi", n, nullptr, phi};
    k.labels = labels; k.coef = coef;
    return sitestep_impl(c, k, p, rep);
}
int tnml_site_gradient_coef(tnml_ctx* c, double* out, int64_t count) {
    if (!c || !out) return tnml_fail(c, "tnml_site_gradient_coef: null argument");
    if (c->sg.last_cnt < 0 || !c->sg.coef) return tnml_fail(c, "tnml_site_gradient_coef: no gradient or step call has been made since the workspace was made (count = %lld)", (long long)count);
    const int64_t have = (int64_t)c->sg.last_cnt * c->nl();
    if (count != have) return tnml_fail(c, "tnml_site_gradient_coef: the last chunk has %d x %d coefficients, count = %lld", c->sg.last_cnt, c->nl(), (long long)count);
    HIPCK(c, hipSetDevice(c->cfg.device));
    SYNCK(c, c->stream);
    HIPCK(c, hipMemcpy(out, c->sg.coef, sizeof(double) * (size_t)have, hipMemcpyDeviceToHost));
    return 0;
}
int tnml_site_step_state(tnml_ctx* c, const char* which, double* out, int64_t count) {
    if (!c || !which || !out) return tnml_fail(c, "tnml_site_step_state: null argument");
    if (c->st_method < 0) return tnml_fail(c, "tnml_site_step_state: no step has been taken since the state was reset");
    const double* src = !strcmp(which, "v") ? c->st_v : !strcmp(which, "m") ? c->st_m : nullptr;
    if (strcmp(which, "v") && strcmp(which, "m")) return tnml_fail(c, "tnml_site_step_state: unknown array \"%s\" (m, v)", which);
    if (!src) return tnml_fail(c, "tnml_site_step_state: method %s keeps no array \"%s\"", step_method_name(c->st_method), which);
    if (count != (int64_t)c->st_elems) return tnml_fail(c, "tnml_site_step_state: %s has %lld elements, count = %lld", which, (long long)c->st_elems, (long long)count);
    HIPCK(c, hipSetDevice(c->cfg.device));
    SYNCK(c, c->stream);
    HIPCK(c, hipMemcpy(out, src, sizeof(double) * c->st_elems, hipMemcpyDeviceToHost));
    return 0;
}

// ---- device-resident arguments: the tnml_*_dev entry points (tnml.h) ----------
// Each is the host-pointer call of its name on the same *_impl, with the memory space of the arrays set to the device.
// The record of a device-resident call from its batch and its outputs (o may be null).  takes: what the call takes beside the images,
// weights and pred; the other fields of b and o are not looked at, as tnml.h promises.
enum { IN_LABELS = 1, IN_COEF = 2, IN_WHICH = 4, OUT_RESP = 8, OUT_GRADS = 16 };
static int dev_call(tnml_ctx* c, const char* who, const tnml_dev_batch* b, const tnml_dev_out* o, int takes, StreamCall& k) {
    if (!c || !b) return tnml_fail(c, "%s: null argument", who);
    const int given = (b->pixels != nullptr) + (b->phi != nullptr) + (b->phi32 != nullptr);
    if (given > 1) return tnml_fail(c, "%s: exactly one of pixels, phi and phi32 must be given (%d are)", who, given);
    if (b->n > 0 && !given) return tnml_fail(c, "%s: null argument", who);
    k = StreamCall{who, b->n, b->pixels, b->phi, b->phi32};
    if (takes & IN_LABELS) k.labels = b->labels;
    if (takes & IN_COEF) k.coef = b->coef;
    if (takes & IN_WHICH) k.which = b->which;
    if (o) { k.weights = o->weights; k.pred = o->pred; }
    if (o && (takes & OUT_RESP)) k.resp = o->resp;
    if (o && (takes & OUT_GRADS)) { k.grad = o->grad; k.dphi = o->dphi; k.dphi32 = o->dphi32; }
    k.dev = true; k.stream = b->stream;
    return 0;
}
int tnml_predict_dev(tnml_ctx* c, const tnml_dev_batch* b, const tnml_dev_out* o) {
    StreamCall k;
    TCK(dev_call(c, "tnml_predict_dev", b, o, 0, k));
    return predict_impl(c, k);
}
int tnml_evaluate_dev(tnml_ctx* c, const tnml_dev_batch* b, const tnml_dev_out* o, tnml_eval_report* rep) {
    StreamCall k;
    TCK(dev_call(c, "tnml_evaluate_dev", b, o, IN_LABELS, k));
    return predict_impl(c, k, true, rep);
}
int tnml_response_dev(tnml_ctx* c, const tnml_dev_batch* b, const tnml_dev_out* o) {
    StreamCall k;
    TCK(dev_call(c, "tnml_response_dev", b, o, IN_WHICH | OUT_RESP, k));
    return response_impl(c, k);
}
int tnml_backward_dev(tnml_ctx* c, const tnml_dev_batch* b, const tnml_dev_out* o) {
    StreamCall k;
    TCK(dev_call(c, "tnml_backward_dev", b, o, IN_LABELS | IN_COEF | OUT_GRADS, k));
    if (k.dphi && k.dphi32) return tnml_fail(c, "tnml_backward_dev: dphi and dphi32 are both given: at most one of the two");
    return backward_impl(c, k);
}
int tnml_site_step_dev(tnml_ctx* c, const tnml_dev_batch* b, const tnml_step_params* p, tnml_step_report* rep) {
    StreamCall k;
    TCK(dev_call(c, "tnml_site_step_dev", b, nullptr, IN_LABELS | IN_COEF, k));
    return sitestep_impl(c, k, p, rep);
}
// ---- backward from the forward's tape (tnml.h): tnml_forward_taped_* keeps what tnml_backward_taped* starts from ----------------
// The forward is the gradient call's setup (refusals, workspace, staging, tables, the fp32 side) and ONE k_forward_taped launch on one
// chunk; the context then holds a ticket for the inward tape.  The backward checks the ticket and makes the outward half alone.
// The ticket `t` is the live one and nothing has happened that takes its tape; otherwise it dies here, with the name of what took it
static bool tape_live(tnml_ctx* c, int64_t t) {
    if (t <= 0 || !c->tape.id || t != c->tape.id) return false;
    if (c->tape.w_epoch != c->w_epoch) tape_kill(c, c->w_writer);
    else if (c->tape.chunk != c->gradient_chunk) tape_kill(c, "a change of option gradient_chunk");
    else if (c->tape.esz != (c->gradient_dtype == TNML_GRADIENT_F32 ? 4 : 8)) tape_kill(c, "a change of option gradient_dtype");
    else if (!c->sg.tape || c->sg.cap != c->tape.cap) tape_kill(c, "a release of the gradient workspace");
    return c->tape.id != 0;
}
template <typename E>
static int forward_taped_chunk(tnml_ctx* c, const StreamCall& k, const SiteGradPlan& g, int* T_out) {
    constexpr bool f32 = sizeof(E) == sizeof(float);
    GradientWs& s = c->sg;
    const StageGeom sg = k.bytes_form() && c->im_set ? stage_geom(c) : StageGeom{};
    SiteGradArgsT<E> a;
    chain_args(c, s, k.bytes_form(), a.ch);
    a.rowoff = s.rowoff; a.tape = (E*)s.tape; a.tape2 = (E*)s.tape2;
    a.lab = nullptr; a.target = c->target(); a.coef = s.coef; a.grad = s.grad; a.goff = s.goff; a.blk0 = s.blk0;
    a.ch.cnt = (int)k.n;
    TCK(stage_chunk<E>(c, s, k, sg, 0, a.ch.cnt));
    chunk_dest(c, s, k, 0, &a.ch.wout, &a.ch.pred);
    const int T = chain_tile<E>(c, g.maxbond, a.ch.cnt);
    TCK(launch_forward_taped<E>(c, a, g.maxbond, T, g.rows, s.tape_rows * (size_t)s.cap));
    int flag = 0;
    if (f32) HIPCK(c, hipMemcpyAsync(&flag, s.f32.flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    TCK(chunk_results(c, s, k, 0, a.ch.cnt));                   // (the synchronisation the flag rides on)
    if (flag) return left_fp32_range(c, s, k.who, "gradient_dtype", 0, a.ch.cnt);
    *T_out = T;
    return 0;
}
static int forward_taped_impl(tnml_ctx* c, StreamCall& k, int64_t* ticket) {
    if (!c || !ticket) return tnml_fail(c, "%s: null argument", k.who);
    *ticket = 0;
    TCK(images_given(c, k));
    SiteGradPlan g{nullptr, false, 1, 0, 0};
    TCK(streamed_refusals(c, k, "site gradients", &g.maxbond, true));
    if (k.n > c->gradient_chunk)
        return tnml_fail(c, "%s: n = %lld images, option gradient_chunk = %d: a tape belongs to one chunk (raise gradient_chunk, or use tnml_predict_* and tnml_backward_*)", k.who, (long long)k.n, c->gradient_chunk);
    std::vector<long long> goff;
    size_t elems = 0;
    TCK(sitegrad_shape(c, k.who, goff, &elems));
    if (k.n == 0) return 0;
    if (k.dev) TCK(dev_enter(c, k));
    TCK(sitegrad_prepare(c, k, g, goff, elems));
    const bool f32 = c->gradient_dtype == TNML_GRADIENT_F32;
    int T = 0;
    TCK(f32 ? forward_taped_chunk<float>(c, k, g, &T) : forward_taped_chunk<double>(c, k, g, &T));
    TapeTicket& t = c->tape;
    t = TapeTicket();
    t.id = c->next_ticket++; t.n = k.n; t.T = T; t.esz = f32 ? 4 : 8; t.cap = c->sg.cap; t.chunk = c->gradient_chunk; t.bytes_form = k.bytes_form();
    t.maxbond = g.maxbond; t.rows = g.rows; t.nblocks = g.nblocks; t.elems = elems; t.w_epoch = c->w_epoch;
    *ticket = t.id;
    return 0;
}
int tnml_forward_taped_u8(tnml_ctx* c, int64_t n, const uint8_t* pixels, double* weights, int32_t* pred, int64_t* ticket) {
    StreamCall k{"tnml_forward_taped_u8", n, pixels};
    k.weights = weights; k.pred = pred;
    return forward_taped_impl(c, k, ticket);
}
int tnml_forward_taped_phi(tnml_ctx* c, int64_t n, const double* phi, double* weights, int32_t* pred, int64_t* ticket) {
    StreamCall k{"tnml_forward_taped_phi", n, nullptr, phi};
    k.weights = weights; k.pred = pred;
    return forward_taped_impl(c, k, ticket);
}
int tnml_forward_taped_dev(tnml_ctx* c, const tnml_dev_batch* b, const tnml_dev_out* o, int64_t* ticket) {
    StreamCall k;
    TCK(dev_call(c, "tnml_forward_taped_dev", b, o, 0, k));
    return forward_taped_impl(c, k, ticket);
}
int tnml_tape_ticket(tnml_ctx* c, int64_t* ticket, int64_t* n) {
    if (!c || !ticket || !n) return tnml_fail(c, "tnml_tape_ticket: null argument");
    const bool live = tape_live(c, c->tape.id);
    *ticket = live ? c->tape.id : 0; *n = live ? c->tape.n : 0;
    return 0;
}
// the kernels of a backward from the tape in the element type E the forward ran in; k: coef, grad, dphi / dphi32 and the memory space
template <typename E>
static int backward_taped_kernels(tnml_ctx* c, const StreamCall& k) {
    GradientWs& s = c->sg;
    const TapeTicket& t = c->tape;
    const int N = c->N, nl = c->nl(), cnt = (int)t.n;
    SiteGradArgsT<E> a;
    chain_args(c, s, t.bytes_form, a.ch);
    a.ch.cnt = cnt;
    a.rowoff = s.rowoff; a.tape = (E*)s.tape; a.tape2 = (E*)s.tape2;
    a.lab = nullptr; a.target = c->target(); a.coef = s.coef; a.grad = s.grad; a.goff = s.goff; a.blk0 = s.blk0;
    const size_t tape_elems = s.tape_rows * (size_t)s.cap;
    HIPCK(c, hipMemcpyAsync(s.coef, k.coef, sizeof(double) * (size_t)cnt * nl, k.in(), c->stream));
    if (k.grad) HIPCK(c, hipMemsetAsync(s.grad, 0, t.elems * sizeof(double), c->stream));
    TCK(launch_site_outward<E>(c, a, t.maxbond, t.T, t.rows, tape_elems, t.nblocks, k.grad != nullptr));
    if (k.want_dphi()) {
        InputGradArgsT<E> ig;
        ig.sites = sites<E>(s); ig.N = N; ig.cs = a.ch.cs; ig.nl = nl; ig.ld = s.cap; ig.cnt = cnt;
        ig.rowoff = s.rowoff; ig.tape = (const E*)s.tape; ig.tape2 = (const E*)s.tape2; ig.coef = s.coef; ig.dphi = s.dphi;
        if (k.dev) TCK(launch_input_grad<E>(c, ig, t.maxbond, t.T, t.rows, tape_elems, k.dphi, k.dphi ? nullptr : k.dphi32));
        else {
            TCK(launch_input_grad<E>(c, ig, t.maxbond, t.T, t.rows, tape_elems, s.dphiT));
            HIPCK(c, hipMemcpyAsync(k.dphi, s.dphiT, sizeof(double) * (size_t)cnt * N * 2, hipMemcpyDeviceToHost, c->stream));
        }
    }
    s.last_cnt = cnt;
    if (k.grad) HIPCK(c, hipMemcpyAsync(k.grad, s.grad, t.elems * sizeof(double), k.dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    SYNCK(c, c->stream);
    return 0;
}
static int backward_taped_impl(tnml_ctx* c, int64_t ticket, StreamCall& k) {
    const char* who = k.who;
    if (!c) return tnml_fail(c, "%s: null argument", who);
    if (!k.grad && !k.want_dphi()) return tnml_fail(c, "%s: grad and dphi are both NULL: the call would compute nothing", who);
    if (k.dphi && k.dphi32) return tnml_fail(c, "%s: dphi and dphi32 are both given: at most one of the two", who);
    if (c->pend_count > 0) return tnml_fail(c, "%s: a bond update is in flight (tnml_bond_update_end first)", who);
    TCK(ho_locked(c, who));
    if (!tape_live(c, ticket)) {
        if (ticket > 0 && ticket < c->next_ticket)
            return tnml_fail(c, "%s: ticket %lld is not live: its tape was taken by %s (tnml_forward_taped_* again, or tnml_backward_* on the images)", who, (long long)ticket,
                             ticket == c->next_ticket - 1 && !c->tape.id ? c->tape_killer.c_str() : "a later tnml_forward_taped call, if nothing before it (the context keeps the name for its last ticket only)");
        return tnml_fail(c, "%s: ticket %lld was never given out by this context", who, (long long)ticket);
    }
    if (!k.coef) return tnml_fail(c, "%s: null argument (coef)", who);
    const TapeTicket& t = c->tape;
    const int N = c->N, nl = c->nl();
    const size_t un = (size_t)t.n;
    k.n = t.n;
    if (k.dev) {                                                // what dev_enter does for a batch: the checks of the arrays this call has
        TCK(dev_check_args(c, who, {{"coef", k.coef, un * nl * sizeof(double), 8, false}, {"grad", k.grad, t.elems * sizeof(double), 8, true},
                                    {"dphi", k.dphi, un * N * 2 * sizeof(double), 8, true}, {"dphi32", k.dphi32, un * N * 2 * sizeof(float), 4, true}}));
        TCK(dev_entry_wait(c, who, k.stream));
        if (!c->io_blk) TCK(dalloc(c, (void**)&c->io_blk, 3 * sizeof(unsigned long long)));
        HIPCK(c, hipMemsetAsync(c->io_blk, 0xff, 3 * sizeof(unsigned long long), c->stream));
        TCK(launch_check_batch(c, nullptr, k.coef, nullptr, t.n, nl, c->io_blk));
        unsigned long long h[3];
        HIPCK(c, hipMemcpyAsync(h, c->io_blk, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        SYNCK(c, c->stream);
        if (h[1] != ~0ull) return tnml_fail(c, "%s: coefficient %d of image %lld is not finite", who, (int)(h[1] % nl), (long long)(h[1] / nl));
    } else {
        for (int64_t i = 0; i < t.n * nl; ++i)
            if (!std::isfinite(k.coef[i])) return tnml_fail(c, "%s: coefficient %d of image %lld is not finite", who, (int)(i % nl), (long long)(i / nl));
        HIPCK(c, hipSetDevice(c->cfg.device));
    }
    GradientWs& s = c->sg;                                      // the first call that asks for input gradients adds their two results, as sitegrad_workspace does
    int rc = 0;
    if (k.want_dphi() && !s.dphi) rc = ws_alloc(c, s, (void**)&s.dphi, (size_t)2 * N * s.cap * sizeof(double));
    if (!rc && k.want_dphi() && !k.dev && !s.dphiT) rc = ws_alloc(c, s, (void**)&s.dphiT, (size_t)2 * N * s.cap * sizeof(double));
    if (rc) { sitegrad_release(c); return rc; }
    return t.esz == 4 ? backward_taped_kernels<float>(c, k) : backward_taped_kernels<double>(c, k);
}
int tnml_backward_taped(tnml_ctx* c, int64_t ticket, const double* coef, double* grad, double* dphi) {
    StreamCall k{"tnml_backward_taped"};
    k.coef = coef; k.grad = grad; k.dphi = dphi;
    return backward_taped_impl(c, ticket, k);
}
int tnml_backward_taped_dev(tnml_ctx* c, int64_t ticket, const double* coef_dev, const tnml_dev_out* o, void* stream) {
    StreamCall k{"tnml_backward_taped_dev"};
    k.coef = coef_dev;
    if (o) { k.grad = o->grad; k.dphi = o->dphi; k.dphi32 = o->dphi32; }
    k.dev = true; k.stream = stream;
    return backward_taped_impl(c, ticket, k);
}
// test entry: sizeof and the field offsets, in declaration order, of the two structs of this section as this library was compiled
int tnml_abi_layout(const char* name, int64_t* sizes_out) {
    if (!name || !sizes_out) return -1;
    if (!strcmp(name, "tnml_dev_batch")) {
        const size_t v[] = {sizeof(tnml_dev_batch), offsetof(tnml_dev_batch, n), offsetof(tnml_dev_batch, pixels), offsetof(tnml_dev_batch, phi), offsetof(tnml_dev_batch, phi32),
                            offsetof(tnml_dev_batch, labels), offsetof(tnml_dev_batch, coef), offsetof(tnml_dev_batch, which), offsetof(tnml_dev_batch, stream)};
        for (size_t k = 0; k < sizeof(v) / sizeof(v[0]); ++k) sizes_out[k] = (int64_t)v[k];
        return (int)(sizeof(v) / sizeof(v[0]));
    }
    if (!strcmp(name, "tnml_dev_out")) {
        const size_t v[] = {sizeof(tnml_dev_out), offsetof(tnml_dev_out, weights), offsetof(tnml_dev_out, pred), offsetof(tnml_dev_out, resp), offsetof(tnml_dev_out, grad),
                            offsetof(tnml_dev_out, dphi), offsetof(tnml_dev_out, dphi32)};
        for (size_t k = 0; k < sizeof(v) / sizeof(v[0]); ++k) sizes_out[k] = (int64_t)v[k];
        return (int)(sizeof(v) / sizeof(v[0]));
    }
    return -1;
}
