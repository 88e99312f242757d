// tnml_host.h -- the host orchestration layer of libtnml.so: what the tnml_*.hip sources (one subsystem each) share, and the layout of
// the two pinned host blocks they and svd.hip address.  Host code only; the kernel sources keep to tnml_internal.h
// (svd.hip and kernels_sgemm.hip take the layout's names from here, nothing else).
#pragma once
#include "tnml_internal.h"

// ---- pinned host layouts ----------------------------------------------------------------------
// One slot of tnml_ctx::hrep, the report block of a bond update in flight (doubles; two slots):
//   [ eigenvalue mirror: svd_n | check words: HC_RESERVED | scal + trace: HREP_TRACE_N | norm partial pairs: 2 HREP_DN_PAIRS | carried block: HREP_CARRY_N ]
// A split of matrix side n <= svd_n mirrors its n ascending eigenvalues to the head of the slot and its check words right behind
// them, at [n + HC_*): the check words of the largest split end where the [scal | trace] mirror begins.
enum {
    HC_DEV0 = 0,        // max |Q^T Q - I| of the kept basis before the first polish step
    HC_CHOLFAIL = 1,    // the Cholesky factorisation of the Cholesky QR failed (dependent vectors)
    HC_CHOLQR = 2,      // a Cholesky QR was needed (the basis of the inverse iteration was not orthonormal as it came)
    HC_DEV_IN = 3,      // max |S - I| of the basis that went into the Cholesky QR (diagnostic)
    HC_BAD = 4,         // the check failed: !(HC_DEV0 < 1e-6) or HC_CHOLFAIL (k_dgemm_small's epilogue / k_split_check_mirror)
    HC_MKEPT = 5,       // predicted split: the column count the truncation rule keeps, as k_truncate_verdict computes it
    HC_WRONG = 6,       // predicted split: that count is not the predicted one
    HC_N = 7,
    HC_SYNC_N = 4,      // the words a synchronous split copies behind its eigenvalues (HC_DEV0..HC_DEV_IN)
    HC_RESERVED = 8
};
enum {
    HREP_TRACE_N = SC_N + 4 * TNML_MAX_PASS,   // the CG scalars, then the per-pass trace (the device's tnml_ctx::scal, one copy)
    HREP_DN_PAIRS = 256,                       // norm partial pairs (|newB|^2, |newB - B|^2) of launch_diffnorm_host
    HREP_CARRY_N = 64,                         // the carried block: slot k mirrors tail[k] (TNML_CARRY.., TNML_FPSLOT.., TNML_SPECSLOT, TNML_PREDSLOT) ...
    HREP_FP = 48                               // ... and the eight fingerprint sums of check_replicas = 2 land here
};
static_assert(HC_N <= HC_RESERVED, "the check words of a split must fit the room reserved behind the eigenvalue mirror");
static_assert(HC_WRONG == HC_MKEPT + 1, "k_truncate_verdict writes the count and its verdict side by side");
static_assert(TNML_CARRY + TNML_CARRYN <= HREP_FP && TNML_FPSLOT + 8 <= HREP_FP, "the carried slots end before the fingerprint landing area");
static_assert(HREP_FP + 8 <= HREP_CARRY_N, "the fingerprint landing area must lie inside the carried block");
inline size_t hrep_off_trace(const tnml_ctx* c) { return (size_t)c->svd_n + HC_RESERVED; }
inline size_t hrep_off_dn(const tnml_ctx* c) { return hrep_off_trace(c) + HREP_TRACE_N; }
inline size_t hrep_off_carry(const tnml_ctx* c) { return hrep_off_dn(c) + 2 * HREP_DN_PAIRS; }
inline size_t hrep_slot_doubles(const tnml_ctx* c) { return hrep_off_carry(c) + HREP_CARRY_N; }      // = tnml_ctx::hrep_stride
inline double* hrep_eig(tnml_ctx* c, int slot) { return c->hrep + (size_t)slot * c->hrep_stride; }   // [n] ascending eigenvalues of the split
inline double* hrep_check(tnml_ctx* c, int slot, int n) { return hrep_eig(c, slot) + n; }            // [HC_*] behind the n eigenvalues
inline double* dn_host(tnml_ctx* c, int slot) { return hrep_eig(c, slot) + hrep_off_dn(c); }
inline double* pend_host(tnml_ctx* c, int slot) { return hrep_eig(c, slot) + hrep_off_carry(c); }
// tnml_ctx::h_scal, the pinned block of the synchronous paths (doubles):
//   [ eigenvalues + check words of a synchronous split, and other small results: 2 svd_n + 32 | its check words, kept past the host's
//     decision: 32 | scal + trace: HREP_TRACE_N | spare: HSCAL_SPARE ]
enum { HSCAL_KEPT_N = 32, HSCAL_SPARE = 2 * 64 };
inline double* hscal_eig(tnml_ctx* c) { return c->h_scal; }
inline size_t hscal_off_kept(const tnml_ctx* c) { return 2 * (size_t)c->svd_n + 32; }
inline size_t hscal_off_trace(const tnml_ctx* c) { return hscal_off_kept(c) + HSCAL_KEPT_N; }
inline size_t hscal_doubles(const tnml_ctx* c) { return hscal_off_trace(c) + HREP_TRACE_N + HSCAL_SPARE; }
inline double* hscal_kept(tnml_ctx* c) { return c->h_scal + hscal_off_kept(c); }
inline double* hscal_trace(tnml_ctx* c) { return c->h_scal + hscal_off_trace(c); }
// the [scal | trace] mirror of a bond update in flight (slot >= 0), or the one of the synchronous entry points
inline double* trace_host(tnml_ctx* c, int slot) { return slot >= 0 ? hrep_eig(c, slot) + hrep_off_trace(c) : hscal_trace(c); }

// ---- scopes and guards of the entry points ----------------------------------------------------
// Entry points every rank calls in step (they contain all-reduces) hold one of these: a failure inside aborts an in-process communicator.
struct CollScope { tnml_ctx* c; explicit CollScope(tnml_ctx* c_) : c(c_) { ++c->coll_depth; } ~CollScope() { --c->coll_depth; } };
// Held-out evaluation (tnml_heldout_attach): an attached held-out context refuses what would change its W, environments, data or bond
// (train_too: and a training context with a held-out context refuses what would change its W or environments outside a bond update)
inline int ho_locked(tnml_ctx* c, const char* who, bool train_too = false) {
    if (c->held) return tnml_fail(c, "%s: the context is attached as a held-out set (tnml_heldout_detach first)", who);
    if (train_too && c->ho) return tnml_fail(c, "%s: a held-out context is attached to this context (tnml_heldout_detach first)", who);
    return 0;
}
struct EnvProtect {                                     // the operands of one operation: resident and not evictable while it is set up
    tnml_ctx* c; int keep[4];
    EnvProtect(tnml_ctx* c_, int a, int b = 0, int d = 0, int e = 0) : c(c_) { for (int k = 0; k < 4; ++k) keep[k] = c->env_protect[k]; c->env_protect[0] = a; c->env_protect[1] = b; c->env_protect[2] = d; c->env_protect[3] = e; }
    ~EnvProtect() { for (int k = 0; k < 4; ++k) c->env_protect[k] = keep[k]; }
};
static inline int ru16(int x) { return (x + 15) / 16 * 16; }
// Every place that writes W says so here, with the name a refused tnml_backward_taped* then gives: the one counter a tape's ticket is held to
inline void w_written(tnml_ctx* c, const char* who) { ++c->w_epoch; c->w_writer = who; }
// the live ticket dies (none: nothing happens); `who` took its tape
inline void tape_kill(tnml_ctx* c, const char* who) { if (c->tape.id) { c->tape = TapeTicket(); c->tape_killer = who; } }

// ---- tnml_core.hip ----------------------------------------------------------------------------
int dalloc(tnml_ctx* c, void** p, size_t bytes);

// ---- tnml_comm.hip ----------------------------------------------------------------------------
// sum over ranks of a fp64 device buffer, in stream order (replaces stdx::accumulate, fixedL.cc:385,402,421,427)
int allreduce(tnml_ctx* c, double* buf, size_t count);
int allreduce_packed(tnml_ctx* c, size_t n);            // the packed buffer [tail | G] of the current bond (n = elements of G)
int carry_deliver(tnml_ctx* c);
int replica_fingerprint(tnml_ctx* c, int j0, int j1, double* out8);
bool fingerprint_agrees(const double* sums8, int nranks);

// ---- tnml_data.hip ----------------------------------------------------------------------------
StageGeom stage_geom(const tnml_ctx* c);
int check_W(tnml_ctx* c);

// The arrays of one streamed call (tnml_infer.hip): every entry point fills one record with what its call takes and hands it to its *_impl,
// so a null field is an array the call was not given or does not produce.  What is no array travels beside it.
struct StreamCall {
    const char* who = nullptr; int64_t n = 0;          // the entry point, for the messages; the images of the call
    // the images, exactly one: bytes [n][N] ([n][S] under an input map), features [n][N][2], or (tnml_*_dev only) fp32 features, widened exactly while staging
    const uint8_t* pixels = nullptr; const double* phi = nullptr; const float* phi32 = nullptr;
    const int32_t* labels = nullptr; const double* coef = nullptr; const int32_t* which = nullptr;   // [n], [n][nl], [n]
    double* weights = nullptr; int32_t* pred = nullptr; double* resp = nullptr; double* grad = nullptr;   // [n][nl], [n], [n][N][2]; every site in tnml_get_site's layout
    double* dphi = nullptr; float* dphi32 = nullptr;   // the input gradients [n][N][2]; dphi32 (tnml_*_dev only): rounded once to fp32, instead of dphi
    bool dev = false; void* stream = nullptr;          // the tnml_*_dev calls (tnml.h): the arrays are device memory, last written by this hipStream_t,
    bool entered = false;                              // and the pointer checks, the entry wait and the value check of this call have been made
    hipMemcpyKind in() const { return dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; }
    bool bytes_form() const { return pixels != nullptr; }
    bool has_images() const { return pixels || phi || phi32; }
    bool want_dphi() const { return dphi || dphi32; }
};
struct DevArg { const char* name; const void* p; size_t bytes; size_t align; bool out; };
// Every argument with p non-null: device memory of the context's device as the runtime describes it, aligned, [p, p + bytes) inside
// its allocation, no output range overlapping another argument's.  Nothing is dereferenced, launched or allocated.
int dev_check_args(tnml_ctx* c, const char* who, const std::vector<DevArg>& args);
// hipSetDevice, then the context's stream waits for what `stream` holds now (the one event of the context, made by the first call)
int dev_entry_wait(tnml_ctx* c, const char* who, void* stream);

// ---- tnml_env.hip -----------------------------------------------------------------------------
void slot_release(tnml_ctx* c, EnvSlot& e);
// consumer: the stream whose work will touch the new unit first (it waits for a copy to the host that may still be reading the slab)
int slot_acquire(tnml_ctx* c, EnvSlot& e, int m, int L, hipStream_t consumer = nullptr);
int env_ensure(tnml_ctx* c, int j);
int env_lookahead(tnml_ctx* c, int b, int ha);
const void* phi_site(const tnml_ctx* c, int j);
int shift_core(tnml_ctx* c, int cs, bool from_left, const void* src, int Le, void* dst, bool acc_out, int* Lout_p);
int env_init_impl(tnml_ctx* c);
int shift_env_impl(tnml_ctx* c, int b, int from_left);

// ---- tnml_infer.hip ---------------------------------------------------------------------------
// the streamed workspaces (tnml_ctx::pk, rs, sg); synchronise first
void predict_release_map(tnml_ctx* c);                 // of tnml_predict_*, the part that follows the input map
void predict_release(tnml_ctx* c); void response_release(tnml_ctx* c); void sitegrad_release(tnml_ctx* c);
void io_release(tnml_ctx* c);                          // what the tnml_*_dev calls keep: the check block and the entry event; synchronise first
void step_release(tnml_ctx* c);                        // the optimiser state of tnml_site_step_* (the st_ fields); synchronise first

// ---- tnml_bond.hip ----------------------------------------------------------------------------
PackDesc bond_pack_desc(const BondPlan& p);
int set_bond_impl(tnml_ctx* c, int b);
int forward_pass(tnml_ctx* c, const double* vec, int mode, double* tail, bool want_P, bool reduce = true);      // !reduce: the partial sums stay in c->partials[c->part_n][12]
int cgrad_device(tnml_ctx* c, int npass, double lambda, double cconv, bool outputs_current = false);
int cgrad_trace_enqueue(tnml_ctx* c, int slot = -1);
void cgrad_trace_parse(tnml_ctx* c, int npass, tnml_cg_trace* tr, int slot = -1);
void quadcost_parse(tnml_ctx* c, const double* t, double lambda, double* cost, double* label_cost, double* reg_cost, int64_t* ncorrect);
int quadcost_device(tnml_ctx* c, double lambda, double* cost, double* label_cost, double* reg_cost, int64_t* ncorrect, bool want_P);
int exact_device(tnml_ctx* c, double lambda, double pcut);

// ---- tnml_update.hip --------------------------------------------------------------------------
void heldout_release(tnml_ctx* c);
