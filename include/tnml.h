/*
 * tnml.h -- C-ABI of the MI355X-native fixedL hot path (libtnml.so).
 *
 * The reference (emstoudenmire/TNML) has no plugin/FFI surface: fixedL.cc is one translation unit
 * whose functions take ITensor objects.  This ABI is the seam cut exactly where
 * mldmrg() (fixedL.cc:451-570) calls into TrainStates / cgrad / quadcost / ITensor svd, so a host
 * driver that keeps the reference's CLI and sweep loop binds these entry points instead.  Each
 * function cites the reference interface it replaces.
 *
 * Conventions
 *  - every call returns 0 on success, non-zero on error; tnml_last_error(ctx) gives the message
 *    (the reference's Error()/EXIT become status codes -- nothing throws across the ABI);
 *  - tensors cross the ABI as raw fp64 (the reference's Real) column-major arrays in ITensor index
 *    order, first index fastest:
 *        site tensor  A_j [ml][2][mr]     (+[10] last, only on the label site c0 = N/2)
 *        bond tensor  B   [mL][2][2][mR]  (+[10] last, only when c0 is b or b+1)
 *        environment  E_j [m] or [m][10]  per image
 *    sites/bonds are 1-indexed as in the reference;
 *  - one context per GPU / per rank; calls on a context are serialised by the caller; the
 *    collective calls (tnml_gradient, tnml_quadcost, tnml_cgrad, tnml_bond_update) must be entered
 *    by every rank of the communicator;
 *  - the context owns all device memory (features, labels, environments, W replica, workspaces),
 *    its HIP stream, rocBLAS/rocSOLVER handles and the RCCL communicator.  There is no CPU
 *    fallback: without a usable HIP device tnml_create fails.
 */
#ifndef TNML_H
#define TNML_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TNML_NL 10           /* label dimension, fixedL.cc:15 */
#define TNML_MAX_PASS 64
enum { TNML_LOSS_QUADRATIC = 0, TNML_LOSS_SOFTMAX = 1 };   /* option "loss": the loss of tnml_evaluate_* and of the labels mode of tnml_site_gradient_* / tnml_site_step_* */
enum { TNML_PREDICT_F64 = 0, TNML_PREDICT_F32 = 1 };   /* option "predict_dtype": arithmetic of tnml_predict_u8 / tnml_predict_phi */
enum { TNML_GRADIENT_F64 = 0, TNML_GRADIENT_F32 = 1 }; /* option "gradient_dtype": arithmetic of tnml_site_gradient_* / tnml_backward_* / tnml_site_step_* */
#define TNML_PREDICT_CHUNK_DEFAULT 8192   /* option "predict_chunk": images per chunk of tnml_predict_u8 / tnml_predict_phi */

typedef struct tnml_ctx tnml_ctx;

/* arithmetic and storage type of the per-image path:
   TNML_F64      everything in fp64, as the reference: features, environments, v_mfma_f64_16x16x4_f64
                 contractions, CG and SVD algebra.  The default and the parity mode.
   TNML_F64_E32  fp64 MFMA contractions and fp64 CG/SVD algebra over environments and features STORED in fp32:
                 half the HBM footprint and env traffic, ~9 % faster at maxm=120.  A single evaluation agrees with
                 the reference to ~1e-6, but the rounding of the environments (1e-7) is amplified by the CG, so a
                 sweep follows the fp64 trajectory only loosely (DESIGN.md "fp32 environments").
   TNML_F32      v_mfma_f32_16x16x4_f32, exact-fp32 arithmetic -- 2x the MFMA rate, for the tolerance study only:
                 the reference's CG is not reproducible in fp32 (DESIGN.md "why fp64 MFMA").
   TNML_BF16     as TNML_F32 (fp32 storage, fp32 CG / label dot / shifts) with the two image-proportional GEMMs of the bond
                 contraction -- the feature GEMM of B*t.v and the gradient GEMM dP*dag(t.v) -- on v_mfma_f32_16x16x32_bf16:
                 operands rounded to bf16 while staging, fp32 accumulation (BASELINE config 5's "bf16 MFMA bond
                 contraction"; report-don't-gate).  Option bf16_grad = 0 keeps the gradient GEMM on the fp32 kernel.
   TNML_BF16X3   the same with every operand split hi + lo (x = bf16(x) + bf16(x - bf16(x))) and three bf16 MFMAs per product
                 (hi*hi + hi*lo + lo*hi): ~16 mantissa bits */
enum { TNML_F32 = 0, TNML_F64_E32 = 1, TNML_F64 = 2, TNML_BF16 = 3, TNML_BF16X3 = 4 };
/* eigensolver of the Gram matrix inside tnml_svd_split (n = smaller side of the matricised bond tensor):
   TNML_SVD_SYEVD      in-house: one-workgroup tridiagonalisation, bisection + inverse iteration, back
                       transform, Newton-Schulz polish; verified per call, falls back to rocSOLVER dstedc
                       for the tridiagonal stage when the check fails (n <= 240; larger matrices use
                       TNML_SVD_ROCSOLVER automatically)
   TNML_SVD_ROCSOLVER  stock rocSOLVER dsyevd
   TNML_SVD_STEDC      in-house tridiagonalisation + rocSOLVER dstedc */
enum { TNML_SVD_SYEVD = 0, TNML_SVD_ROCSOLVER = 1, TNML_SVD_STEDC = 2 };
/* which sweep of the reference the context serves:
   TNML_MODE_FIXEDL  fixedL.cc: one weight MPS with a 10-valued Label index on site N/2, targets delta_{l,l_n}
   TNML_MODE_SINGLE  single.cc / single.h: a plain weight MPS (no Label index, tnml_set_site has_label = 0 on every
                     site), scalar output f(x_n) regressed on y_n = [l_n == target_label] (single.h:103,193).  The
                     same kernels run with a label extent of 1; tnml_forward / tnml_classify return one value per
                     image, label_cost[] buckets the cost by the true label of the image, ncorrect counts
                     (f > 1/2) == y (the reference prints no accuracy in this variant). */
enum { TNML_MODE_FIXEDL = 0, TNML_MODE_SINGLE = 1 };

typedef struct {
    int device;          /* HIP device ordinal */
    int rank, nranks;    /* data-parallel rank / world size (images are sharded by rank) */
    int N;               /* number of sites (fixedL.cc:615) */
    int NT_local;        /* training images owned by this rank */
    int64_t NT_total;    /* training images over all ranks (costs are reported un-normalised) */
    int maxm;            /* largest bond dimension that will occur (workspace sizing) */
    int dtype;           /* TNML_F64 (default choice), TNML_F64_E32, TNML_F32, TNML_BF16 or TNML_BF16X3 */
    int svd_backend;     /* TNML_SVD_* */
    int mode;            /* TNML_MODE_FIXEDL (0, default) or TNML_MODE_SINGLE */
    int target_label;    /* TNML_MODE_SINGLE: the selected label L (single.cc:19); the target is y_n = [l_n == L] */
} tnml_config;

/* mirrors the prints of fixedL.cc:391,429-439 */
typedef struct {
    int npass_done;
    int converged;                         /* 1: |r| < cconv hit after a pass (fixedL.cc:432, single.h:273); 2: TNML_MODE_SINGLE only,
                                              |r| < cconv at entry, "not optimizing", B untouched (single.h:202-206) */
    double cost[TNML_MAX_PASS];            /* un-normalised C printed at :429 (index pass-1) */
    double rnorm[TNML_MAX_PASS];           /* |r| printed at :434/:439 */
    double pAp[TNML_MAX_PASS];
    double alpha[TNML_MAX_PASS];
} tnml_cg_trace;

/* knobs of one bond update: Sweeps(Nsweep,minm,maxm,cutoff) fixedL.cc:749 + Args :751-759 */
typedef struct {
    int maxm, minm;
    double cutoff;
    int npass;
    double lambda;       /* used by cgrad (fixedL.cc:356) */
    double lambda_cost;  /* used by the "After SVD" quadcost (cargs copy, fixedL.cc:467) */
    double cconv;
    int report_costs;    /* also evaluate the cost of the old bond tensor and of the optimised one before the split
                            (single.h:621-622 "Cost = %.10f --> %.10f"): two more forward passes */
} tnml_sweep_params;

/* mirrors the prints of fixedL.cc:490,523-533,341-342 */
typedef struct {
    int bond, half, c;
    int mL, mR, label_on_B;                /* outer link dimensions of the bond tensor; Label on B? */
    int origm, newm;
    double truncerr;
    double norm_newB, diff_B_newB;
    double cost_after_svd;                 /* un-normalised */
    double label_cost[TNML_NL];
    double reg_cost;
    int64_t ncorrect;
    tnml_cg_trace cg;
    double cost_old, cost_cg, reg_cost_cg; /* report_costs: quadcost(oB), quadcost(B) and lambda|B|^2 before the split */
    double norm_oB;                        /* norm of the old bond tensor (single.h:572) */
} tnml_bond_report;

/* ---- lifetime ------------------------------------------------------------------------- */
int tnml_create(tnml_ctx** out, const tnml_config* cfg);
int tnml_destroy(tnml_ctx* ctx);
const char* tnml_last_error(const tnml_ctx* ctx);      /* ctx may be NULL: error of the failed create */
/* last non-fatal notice of ctx ("" if none): e.g. the split clamped maxm to the context's maxm and so truncates harder than asked */
const char* tnml_last_warning(const tnml_ctx* ctx);

/* RCCL communicator over xGMI.  Rank 0 obtains a 128-byte unique id, the host transports it to
   the other ranks (any channel), every rank then calls tnml_comm_init.  Replaces the host-side
   stdx::accumulate over per-thread partials, fixedL.cc:333,339,385,402,421,427. */
int tnml_comm_unique_id(void* id128);
int tnml_comm_init(tnml_ctx* ctx, const void* id128);
/* In-process communicator for n ranks that share ONE device (RCCL refuses two ranks on a GPU): ctxs[r] must have been
   created as rank r of n on the same device; call once, from one thread, before the ranks start.  Afterwards every
   collective entry point must be driven by one host thread per rank (they meet in a host barrier).  Same results as
   RCCL (rank-ordered sums, bit-identical on every rank); a correctness vehicle for one-GPU boxes, not a fast path. */
int tnml_comm_init_local(tnml_ctx** ctxs, int n);
/* One-shot all-reduce for the ranks of ONE process on several devices (one host thread per rank, as the fixedL driver runs them):
   every rank writes its packed [scalars | gradient] buffer straight into its slot of every peer's receive region (peer stores over the
   direct xGMI links, one hop), the streams meet through events, every rank sums its own n slots in rank order -- bit-identical sums
   everywhere (replaces the ring all-reduce for the latency-bound 461 KB payloads of fixedL.cc:385,402,421,427).
   Ranks may also share a device (how it is tested on one GPU).  Same calling rules as tnml_comm_init_local. */
int tnml_comm_init_oneshot(tnml_ctx** ctxs, int n);
/* which collective path this context uses: 0 none (one rank), 1 RCCL, 2 in-process staging buffer, 3 one-shot peer write */
/* One-shot all-reduce ACROSS PROCESSES (one process per GPU -- how `python bench.py --gpus N --allreduce oneshot` and any
   torch.distributed / MPI launch run; replaces stdx::accumulate, fixedL.cc:385,402,421,427, like tnml_comm_init): every rank exports an
   IPC handle of its receive region (tnml_oneshot_export), the caller gathers the nranks handles over its own control plane in rank
   order and hands all of them to every rank (tnml_oneshot_connect).  From then on every collective of the library is ONE kernel per
   rank -- peer stores into the mapped regions, device-side arrival flags, an ordered local sum (the same bits on every rank) -- with no
   host synchronisation between the ranks (tnml_ctx option comm_timeout_s bounds the device-side wait; tnml_synchronize reports a
   time-out).  Needs HSA_ENABLE_IPC_MODE_LEGACY=0 and peer access between the ranks' devices; ranks may share a device (tests). */
#define TNML_ONESHOT_HANDLE_BYTES 64
int tnml_oneshot_export(tnml_ctx* ctx, void* handle64);
int tnml_oneshot_connect(tnml_ctx* ctx, const void* handles /* nranks * TNML_ONESHOT_HANDLE_BYTES, rank order */);
/* memory kind of this rank's receive region: 1 fine-grained, 2 uncached, 0 no cross-process transport.  (tnml_oneshot_export fails
   rather than fall back to coarse-grained memory, which is coherent at kernel boundaries only.)  A collective whose device-side wait
   timed out fills its buffer with NaNs and every later entry point that synchronises with the stream returns an error. */
int tnml_oneshot_mem_kind(tnml_ctx* ctx);
/* bytes of the receive region tnml_oneshot_export will allocate for this configuration ([2 parities][nranks][10 Kmax^2 + 48] doubles + flags);
   tnml_estimate_bytes / tnml_plan_maxm do not know the transport and do not count it: subtract it from the budget when planning maxm */
int64_t tnml_oneshot_region_bytes(const tnml_config* cfg);
/* transport in use: 0 none, 1 RCCL, 2 in-process staging buffer, 3 in-process one-shot, 4 cross-process one-shot */
int tnml_collective_mode(tnml_ctx* ctx);
/* Collective.  Verifies that the communicator really spans cfg.nranks ranks (ncclCommCount) and that every rank holds a
   bit-identical replica of the weight MPS (a 64-bit fingerprint of all site tensors, max/min-reduced over the ranks);
   non-zero + tnml_last_error on a mismatch.  The replicated CG/SVD algebra relies on identical replicas the way the
   reference relies on one shared W (fixedL.cc:451); tnml_bond_update runs the same check on the two site tensors it
   rewrites after every split (TNML_CHECK_REPLICAS=0 disables that).  nranks_in_comm (nullable) receives the communicator size. */
int tnml_replica_check(tnml_ctx* ctx, int* nranks_in_comm);
int64_t tnml_replica_repairs(tnml_ctx* ctx);           /* re-broadcasts so far in check_replicas mode 2 */
/* collectives this rank has entered so far: sum all-reduces (the payload: gradient / A p + scalars) and broadcasts (rank 0's
   eigenvalues in the split) */
int tnml_collective_stats(tnml_ctx* ctx, int64_t* allreduces, int64_t* broadcasts);

/* ---- training set: TState ctor fixedL.cc:28-47 + feature map :637-642 -------------------- */
/* raw bytes [NT_local][N] with the reference's feature map phi = [1, byte/(255*255*4)]; under an input map (below)
   [NT_local][src_rows*src_cols] bytes with the map's block sums and table */
int tnml_set_data_u8(tnml_ctx* ctx, const uint8_t* pixels, const int32_t* labels);
/* arbitrary d=2 local features phi[NT_local][N][2] (TState::data layout) */
int tnml_set_data_phi(tnml_ctx* ctx, const double* phi, const int32_t* labels);

/* ---- input map: raw bytes -> local features for any feature map and any block-sum reduction ------------------------
 * Every d=2 feature map of a byte image is a table: a site's features depend on its pixel value only, and after a block x block
 * mean that value is code / block^2 with `code` the integer sum of the block's bytes (0 .. 255 block^2).  While a map is set,
 * tnml_set_data_u8 and tnml_predict_u8 read src_rows*src_cols bytes per image (not N), the device sums the blocks, looks the two
 * features of every site up in `table` and transposes to its site-first layouts; a table filled with the host's own feature
 * expression (tnmlh_feature_table) gives bit for bit the features of the fp64 path (tnml_set_data_phi / tnml_predict_phi).
 * fp32-storage contexts round table[code][s] once to float for the stored features, as tnml_set_data_phi rounds phi; the chain
 * kernel of tnml_predict_u8 always reads the fp64 table.
 * The map is consulted only when bytes arrive: features stored by an earlier tnml_set_data_* call stay as they are, whatever map
 * is set or removed afterwards.  Without a map every call does, bit for bit, what it did before this entry point existed.
 * Refused (the message names the field; the previous map stays in force) when block is outside 1..8, ncodes is not
 * 255 block^2 + 1, out_rows*out_cols is not cfg.N, a block leaves the source image (row0 / col0 negative, or
 * row0 + block out_rows > src_rows, col0 + block out_cols > src_cols), table is NULL or holds a value that is not finite, the
 * context is attached as a held-out set, or a bond update is in flight. */
typedef struct {
    int src_rows, src_cols;     /* raw image handed to tnml_set_data_u8 / tnml_predict_u8: [src_rows][src_cols] bytes, row-major */
    int block;                  /* 1..8: a site is the SUM of a block x block square of bytes */
    int row0, col0;             /* top-left corner of the first block (reduce(): side % bsize) */
    int out_rows, out_cols;     /* sites in row-major order of the reduced image; out_rows*out_cols == cfg.N */
    int ncodes;                 /* must be 255*block*block + 1 */
    const double* table;        /* [ncodes][2]: the two local features of a site whose block sum is `code`; copied by the call */
} tnml_input_map;
int tnml_set_input_map(tnml_ctx* ctx, const tnml_input_map* map);   /* NULL: back to the built-in map */
int tnml_get_input_map(tnml_ctx* ctx, tnml_input_map* out);         /* geometry only (table = NULL); block = 0 when none is set */

/* ---- weight MPS replica (W.A(j) / W.Aref(j)) ------------------------------------------- */
int tnml_set_site(tnml_ctx* ctx, int j, int ml, int mr, int has_label, const double* A);
int tnml_site_dims(tnml_ctx* ctx, int j, int* ml, int* mr, int* has_label);
int tnml_get_site(tnml_ctx* ctx, int j, double* A);

/* ---- MPS algebra on the device: the sum of weight MPS behind the W0..W9 start (fixedL.cc:682-701,729) ----------
 * sum(ipsis,{"Cutoff",1E-10}) is a direct sum of the parts (block-diagonal links; the Label index, a physical index, is shared)
 * followed by orthogonalize(args).  A context used only for this needs no image data (NT_local = 1, no tnml_set_data_* call).
 *
 * tnml_mps_place: one block of the direct sum.  The first placement on site j (since W was last set, split, compressed or used by tnml_env_init /
 * tnml_mps_overlap, or with other outer dimensions) shapes the site as an ML x 2 x MR tensor (x 10 on the Label site c0) and zeroes it on the device; every
 * placement then ADDS the ml x 2 x mr block A (ITensor layout, no Label index) at link offsets (row0, col0), into label slot `label` on
 * site c0 (in.Aref(c) *= setElt(Lval(n)), fixedL.cc:693) and with label = -1 on every other site.  The block travels at its own size;
 * the zero-padded site never crosses the bus.  Refused as tnml_set_site is (range, maxm, edge dimensions, held-out lock), and when the
 * block leaves the site, when a label slot is named off c0 (or none on c0), or while a bond update is in flight. */
int tnml_mps_place(tnml_ctx* ctx, int j, int ML, int MR, int row0, int col0, int ml, int mr, int label, const double* A);
typedef struct {
    int maxm_before, maxm_after;   /* largest bond dimension before / after */
    int nbonds;                    /* N - 1: entries written to newm / truncerr */
    double truncerr_sum;           /* sum over the bonds of the relative truncation errors of the second pass */
    int64_t fallbacks;             /* eigensolver fallbacks to rocSOLVER taken inside this call (tnml_svd_stats counts them too) */
    int* newm;                     /* in: caller's array of N - 1 ints or NULL; [b-1] = new dimension of bond b */
    double* truncerr;              /* in: caller's array of N - 1 doubles or NULL; [b-1] = relative truncation error of bond b */
} tnml_compress_report;
/* orthogonalize(args) behind sum(psis,args): a right-to-left pass brings sites 2..N into right-orthonormal form without discarding weight
 * (every bond drops to its rank bound min(rows, columns) at most), a left-to-right pass truncates each bond with
 * tnml_truncate(p, n, maxm, 1, cutoff); the orthogonality centre ends on site N.  maxm <= 0: no Maxm (the context's maxm bounds it).
 * Device resident: per bond the product A_b A_{b+1} and the split of tnml_svd_split; only eigenvalues and check values reach the host.
 * One rank only: refused with a communicator, with a bond update in flight, or with a held-out context attached.  Afterwards
 * environments, bond plan and cached outputs are invalid: call tnml_env_init before anything that uses them.  report may be NULL. */
int tnml_mps_compress(tnml_ctx* ctx, double cutoff, int maxm, tnml_compress_report* report);
/* overlap(W,W) (fixedL.cc:729) by the O(m^3) transfer chain E <- sum_{s,l} A_{s,l}^T E A_{s,l} on the context's stream */
int tnml_mps_overlap(tnml_ctx* ctx, double* ovl);

/* ---- TrainStates::init / setBond / shiftE  (fixedL.cc:122-157, :159-190, :192-233) ------- */
int tnml_env_init(tnml_ctx* ctx);
int tnml_set_bond(tnml_ctx* ctx, int b);               /* selects env buffers; t.v is never formed */
int tnml_shift_env(tnml_ctx* ctx, int b, int from_left);
int tnml_env_dims(tnml_ctx* ctx, int j, int* m, int* has_label);
int tnml_get_env(tnml_ctx* ctx, int j, double* E);     /* [NT_local][m(*10)], for parity tests */
/* The host tier of the environments (the reference's Nbatch / proj_images spill, fixedL.cc:115-120,153,177-178,216,231, with host
   memory in the place of its disk files).  tnml_set_option(ctx, "env_budget_mb", MB) caps the environment slabs held on the device
   (0, the default: no cap -- everything stays in HBM); an environment that does not fit is copied to host memory, farthest from
   the current bond first, and copied back when setBond / shiftE needs it.  Results do not depend on the budget.  Also taken when
   hipMalloc of a new slab fails.  tnml_env_stats: copies to the host / back so far, slabs on the device, bytes currently on the host. */
int tnml_env_stats(tnml_ctx* ctx, int64_t* spills, int64_t* fetches, int64_t* slabs_on_device, int64_t* host_bytes);

/* ---- bond tensor oB = W.A(b)*W.A(b+1)  (fixedL.cc:494,527,745) --------------------------- */
int tnml_bond_dims(tnml_ctx* ctx, int b, int* mL, int* mR, int* label_on_B);
int tnml_bond_tensor(tnml_ctx* ctx, int b, double* B);

/* ---- per-image contractions of the current bond ------------------------------------------ */
/* P_n = B*t.v (fixedL.cc:318,377,399,416): P[NT_local][10] */
int tnml_forward(tnml_ctx* ctx, const double* B, double* P);
/* sum_n dP_n*dag(t.v) over ALL ranks (fixedL.cc:375-385): G has the layout of B */
int tnml_gradient(tnml_ctx* ctx, const double* B, double* G);
/* quadcost (fixedL.cc:280-344): *cost = sum_l C_l + lambda|B|^2, un-normalised, over all ranks */
/* <p|A|p> = sum_n |p*t.v_n|^2 + lambda |p|^2 of a direction p (the pAp pass of cgrad, fixedL.cc:394-403); collective */
int tnml_pAp(tnml_ctx* ctx, const double* p, double lambda, double* pAp);
int tnml_quadcost(tnml_ctx* ctx, const double* B, double lambda, double* cost,
                  double label_cost[TNML_NL], double* reg_cost, int64_t* ncorrect);
/* cgrad (fixedL.cc:349-445): B is updated in place */
int tnml_cgrad(tnml_ctx* ctx, double* B, int npass, double lambda, double cconv, tnml_cg_trace* trace);
/* test entry: a copy of what the last tnml_cgrad left on the device, for the per-pass tests of the CG.  which = "R", "Pv", "G": the fp64
   CG vectors (residual, direction, image sum) in the host layout of B; "P", "Pp", "dP": the model outputs, p*t.v of the last pAp pass and the
   residuals tgt - P as [NT padded to 256][10] doubles (a label extent of 1 in TNML_MODE_SINGLE), padded rows included, widened from the
   context's type.  count: the number of doubles `out` holds, which has to be that size.  Changes no state. */
int tnml_cg_state(tnml_ctx* ctx, const char* which, double* out, int64_t count);

/* exact (single.h:117-160; TNML_MODE_SINGLE, TNML_F64, one rank): B = y Phi^+ through the SVD of the D x NT design matrix of the
   v_n (D = 4 mL mR <= 4096; its rows come from D forward passes of unit tensors, the SVD is a one-sided Jacobi on the host so
   that small singular values stay accurate), with the reference's filtered inverse s/(s^2 + lambda) for s > pcut.
   B (ITensor layout, D doubles) is output only.  Meant for small problems, like the reference's (single.h:114). */
int tnml_exact(tnml_ctx* ctx, double* B, double lambda, double pcut);
/* pinv of the per-label variant (single.h:404-517; TNML_MODE_SINGLE, one rank, after tnml_set_bond): a subspace iteration on sum_n v_n v_n^T
   from the start V0 (D x r column-major, D = 4 mL mR in ITensor order, r = the reference's Ntarget <= 64), V <- polar factor of E = V^T A
   until V*E moves by less than 1E-4 or npass passes, then B = yUS * F pseudoInv(D) G.  In the reference the start is random and time-seeded and
   the result only has its cost printed (single.h:596-601; the update that follows is cgrad): a diagnostic.  ve[0..npass]: the V*E trace,
   Dsv[r]: the singular values of the last E. */
int tnml_pinv(tnml_ctx* ctx, const double* V0, int r, int npass, double lambda, double pcut, double* B, double* ve, int* npass_done, double* Dsv);

/* ---- svd(B, W.Aref(c), S, W.Aref(c+dc)); W.Aref(c+dc) *= S  (fixedL.cc:519-521) ---------- */
/* ha = 1: c = b (sweeping right), ha = 2: c = b+1 (sweeping left).  Updates the W replica.
   sv (nullable, capacity >= min(rows,cols)) receives all singular values, descending. */
int tnml_svd_split(tnml_ctx* ctx, const double* B, int b, int ha, double cutoff, int maxm, int minm,
                   double* truncerr, int* newm, double* sv, int* nsv);

/* ---- one iteration of the mldmrg loop body, device resident (fixedL.cc:478-540) ----------- */
/* setBond -> oB -> cgrad -> svd -> newB -> quadcost -> shiftE without tensors leaving the GPU */
int tnml_bond_update(tnml_ctx* ctx, int b, int ha, const tnml_sweep_params* p, tnml_bond_report* rep);
/* The same bond update in two halves, for a sweep loop that keeps the GPU queue full across bond boundaries (mldmrg's loop
   body ends with prints only, fixedL.cc:523-561): _begin enqueues the whole update -- it blocks once, inside the split, for
   the eigenvalues that decide the new bond dimension -- and returns; _end waits for the end-of-bond scalars (cost, #correct,
   norms; multi-rank: the replica fingerprint) and fills the report.  bond k+1 may be begun before bond k is ended (at most
   two in flight; reports come back in order), in which case _end does not wait at all.  tnml_bond_update = _begin + _end. */
int tnml_bond_update_begin(tnml_ctx* ctx, int b, int ha, const tnml_sweep_params* p);
int tnml_bond_update_end(tnml_ctx* ctx, tnml_bond_report* rep);

/* ---- host-side rules (no GPU needed) ------------------------------------------------------ */
/* ---- inference (fulltest.cc:7-100; util.h:19-40 toverlap, util.h:123-200 fullTest) ------------------
 * Full contraction of every local image with the weight MPS held by the context:
 *   weights[n][l] = W_l(image n)  ([NT_local][10], may be NULL),
 *   pred[n]       = argmax_l |W_l|, first maximum on ties (util.h:42-57,160-163; may be NULL),
 *   count[l] / nincorrect[l] = images of label l / of those, wrongly predicted (local images; a multi-rank
 *   caller sums them -- no collective is entered).  The images are the ones given to tnml_set_data_*;
 *   a test set gets its own context.  Training environments held by the context are not modified. */
int tnml_classify(tnml_ctx* ctx, double* weights, int32_t* pred, int64_t count[TNML_NL], int64_t nincorrect[TNML_NL]);

/* ---- inference on images the context does not hold (util.h:19-40 toverlap + argmax, util.h:42-57) ------------
 * The same contraction and decision rule as tnml_classify (first maximum of |W_l|; f > 1/2 in the per-label variant), for n images
 * handed to the call instead of the ones given to tnml_set_data_*: weights[n][nl] (nl = 10, or 1 in TNML_MODE_SINGLE) and pred[n],
 * either may be NULL.  tnml_predict_u8 applies the feature map of tnml_set_data_u8 to raw bytes (the input map when one is set: pixels is
 * then [n][src_rows*src_cols]), tnml_predict_phi takes features.
 * Any context whose W is complete works, also one created without image data (NT_local = 1, no tnml_set_data_* call).  The host loop
 * cuts n into chunks of option "predict_chunk" images; a chunk is staged, contracted by ONE launch of the chain kernel
 * (kernels_chain.hip: a workgroup carries a tile of 64, 32 or 16 images through all N sites with the chain vectors in LDS; fp64 MFMA
 * on the fp64 master W whatever cfg.dtype is; an image's result does not depend on n, on the chunk or on the tile it lands in) and
 * copied back.  Reads W only: training data, environments, the bond plan and the cached outputs stay as they are, no collective is
 * entered, and the call is allowed on a training context while a held-out context is attached to it.  Refused on a context that is
 * itself attached as a held-out set (the training context's bond updates rewrite its W; tnml_classify refuses it too), while a bond update is in flight, and when W has a
 * bond dimension above 512 (use tnml_classify on a context that holds the images).  n = 0 succeeds and does nothing.
 * Workspace: allocated by the first call (tnml_estimate_bytes does not count it), independent of n, counted by tnml_device_bytes,
 * freed by tnml_destroy (re-made when predict_chunk changes).  With C = predict_chunk rounded up to 64 and M = min(maxm, 512) rounded
 * up to 16:   16 N + 8 nl C + 4 C + 8 M C   bytes (site table, results, parked chain vectors)
 *           + 2 N C                         bytes from the first tnml_predict_u8 on (bytes as given and site-first)
 *           + S C + 2 N C + 16 ncodes       bytes instead, from the first tnml_predict_u8 under an input map on (S = src_rows src_cols
 *                                           bytes as given, 16-bit block sums site-first, the fp64 table); released by every
 *                                           tnml_set_input_map call and re-made by the next tnml_predict_u8 under a map
 *           + 32 N C                        bytes from the first tnml_predict_phi on (features as given and site-first).
 * Option "predict_dtype" = TNML_PREDICT_F32 selects the fp32 chain kernel (k_chain<float>, kernels_chain.hip; v_mfma_f32_16x16x4_f32, tiles of 64
 * images up to bond 256, 32 up to 512, 16 up to 1 024) for the calls that follow; TNML_PREDICT_F64 (the default) is the path above, bit
 * for bit.  Under fp32 W is rounded to fp32 once per call, the features are formed in fp64 as above and rounded once, every product
 * and sum is IEEE fp32 in a fixed order (the kernel's header states it; per image independent of n, chunk and tile), weights receives
 * the fp32 results widened, and pred follows the same rule on the fp32 values (|w| first maximum; w > 0.5f).  Bond dimensions up to
 * 1 024 are served (above: refused as above, tnml_classify); 513..1 024 stay refused under fp64.  A weight that is not finite -- the
 * chain has left the fp32 range -- fails the call with a message that names predict_dtype (use fp64); the context stays usable.
 * Workspace of fp32, allocated by the first fp32 call on top of the above, independent of n, counted and freed the same way:
 *             16 N + 4 + 4 E                bytes (site table of the fp32 copy of W, range flag, the copy: E = the sum over the sites of
 *                                           2 ml mr (x nl on the Label site), each rounded up to 4; grown when W has grown)
 *           + 8 ncodes                      bytes from the first fp32 tnml_predict_u8 under an input map on (the table in fp32; released
 *                                           with the map's workspace)
 *           + 16 N C + 8 N C                bytes from the first fp32 tnml_predict_phi on, in place of the 32 N C above (features as
 *                                           given, and site-first in fp32; the 16 N C are shared with the fp64 path). */
int tnml_predict_u8(tnml_ctx* ctx, int64_t n, const uint8_t* pixels /*[n][N]*/, double* weights /*[n][nl] or NULL*/, int32_t* pred /*[n] or NULL*/);
int tnml_predict_phi(tnml_ctx* ctx, int64_t n, const double* phi /*[n][N][2]*/, double* weights, int32_t* pred);

/* ---- streamed evaluation: tnml_predict_* on labelled images, with the numbers of a held-out report -------------
 * The path of tnml_predict_u8 / tnml_predict_phi, unchanged: the same contraction, input forms (the input map is honoured), chunking
 * ("predict_chunk"), tile choice and "predict_dtype", the same chain kernel on the same staging buffers, the same refusals in the same
 * words.  weights and pred, when asked for, are bit for bit those of tnml_predict_* on the same images and options; when both are
 * NULL nothing per-image is copied back, only the report crosses the bus.  After the chain launch of a chunk one launch of
 * k_eval_tally (kernels_eval.hip) adds the chunk's tallies into a device accumulator block, which is read once at the end of the call.
 * Targets: y_nl = [l == label_n]; in TNML_MODE_SINGLE y_n = [label_n == target_label], label_cost bucketed by the true label.  Under
 * predict_dtype = 1 the cost is formed in fp64 from the widened fp32 weights and pred follows the fp32 rule.
 * label_cost[l] collects the images of true label l in both modes, as tnml_heldout_report and tnml_bond_report do.
 * The cost has a fixed summation order (one workgroup; thread t sums its images t, t + 256, ... in ascending order, label by label; a
 * fixed tree over the threads; chunks in chunk order; cost = label_cost[0] + ... + label_cost[9] in index order): the report is bit-identical on
 * repeats and independent of predict_tile, its integers are independent of predict_chunk, the last bits of the costs may depend on
 * predict_chunk.
 * Read-only like tnml_predict_*: reads W, enters no collective, allowed on a training context, also while a held-out context is attached
 * to it.  Also refused: labels or rep NULL when n > 0, a label outside 0..9 (the message names the image).  A refused call leaves *rep
 * untouched; n = 0 succeeds with a zeroed report.
 * Workspace: that of tnml_predict_* for the input form, plus -- from the first tnml_evaluate_* call on, counted by tnml_device_bytes and
 * freed with the predict workspace (re-made with it when predict_chunk changes) --
 *             4 C + 1040                    bytes (the labels of a chunk; the accumulator block: label_cost, count, nincorrect, confusion).
 * Option "loss" = TNML_LOSS_SOFTMAX (refused in TNML_MODE_SINGLE) changes what k_eval_tally forms from an image's weights, and nothing
 * else: the image's term is the softmax cross-entropy C = log sum_l exp(beta (W_l - max W)) - beta (W_y - max W), beta = "loss_beta",
 * in the fixed arithmetic of tnml_amd/csrc/loss_dev.h (DESIGN.md states it; under predict_dtype = 1 in fp64 from the widened fp32
 * weights), summed in the order stated above; ncorrect, nincorrect and confusion count the signed decision d = the first maximum of
 * W_l.  The pred array the call returns stays tnml_predict_*'s, bit for bit (the first maximum of |W_l|, the reference's rule), and so
 * do weights: the two decisions differ on an image whose largest |W_l| is a negative output, which a softmax loss rewards for a wrong
 * label and the |W| rule then picks.  Chain launches, chunking, workspace and refusals are untouched. */
typedef struct {
    int64_t n;                               /* images evaluated */
    int64_t ncorrect;                        /* decision rule of tnml_classify for the context's mode */
    double  cost;                            /* sum over images and labels of (W_l(x_n) - y_nl)^2; un-normalised, no regulariser */
    double  label_cost[TNML_NL];             /* as tnml_heldout_report::label_cost in both modes */
    int64_t count[TNML_NL];                  /* images of true label l            (tnml_classify) */
    int64_t nincorrect[TNML_NL];             /* of those, wrongly predicted        (tnml_classify) */
    int64_t confusion[TNML_NL][TNML_NL];     /* [true label][pred]; TNML_MODE_SINGLE: pred is 0 or 1, columns 2..9 stay 0 */
} tnml_eval_report;
int tnml_evaluate_u8 (tnml_ctx* ctx, int64_t n, const uint8_t* pixels, const int32_t* labels,
                      tnml_eval_report* rep, double* weights /*[n][nl] or NULL*/, int32_t* pred /*[n] or NULL*/);
int tnml_evaluate_phi(tnml_ctx* ctx, int64_t n, const double* phi, const int32_t* labels,
                      tnml_eval_report* rep, double* weights, int32_t* pred);

/* ---- streamed site responses: every site's effect on an image's output ---------------------------------------
 * The output of the network is linear in every site's feature vector.  For image n and label l = which[n]
 *     resp[n][j][s] = the contraction of W with label index l and the features of image n on every site but j, site j getting e_s,
 * so that  W_l(x_n with site j's feature replaced by psi) = psi_0 resp[n][j][0] + psi_1 resp[n][j][1]  exactly, for any psi; with
 * psi = phi(x_nj) that is W_l(x_n) itself, at every site.  Saliency and occlusion maps, pixel gradients (resp . dphi/dx) and
 * single-pixel checks are host arithmetic on this array.
 * Inputs as tnml_predict_*: bytes through the built-in expression or the input map in force (pixels is then [n][src_rows*src_cols]),
 * or features; any context with a complete W, data-less ones included.  which[n] in 0..nl-1 names the label (a value outside is
 * refused, the message names the image); NULL: the image's own prediction (first maximum of |W_l|).  In TNML_MODE_SINGLE there is one
 * output (nl = 1, site 1 plays the centre) and which must be NULL or all zero.  weights and pred, either may be NULL, are bit for bit
 * those of tnml_predict_* under predict_dtype = 0 on the same images.
 * The host loop cuts n into chunks of option "response_chunk" images (default 1 024); a chunk is staged as tnml_predict_* stages it,
 * ONE launch of k_response (kernels_response.hip) walks the chain inward, keeping every chain vector on a tape in device memory, and
 * outward from the Label site, and the result is copied back: about two chain passes instead of the 2 N contractions per image that
 * 2 N tnml_predict_phi calls on modified images take.  fp64 only: under predict_dtype = 1 the call is refused with a message that
 * names predict_dtype.  resp is summed in a fixed order (the kernel's header states it), without atomics: an image's values do not
 * depend on n, on the chunk, on the tile width ("predict_tile" is honoured) or on the tile it lands in, and repeats are bit-identical.
 * Reads W only and enters no collective, like tnml_predict_*, and is refused as tnml_predict_* is, in the same words: on a context
 * attached as a held-out set, while a bond update is in flight, when W is incomplete and when W has a bond dimension above 512.
 * n = 0 succeeds and does nothing.  Chains of N = 2 and N = 3 sites do not reach these calls: tnml_create refuses N < 4 with a
 * message (N = 4, with one site left of the Label site, is the shortest chain served).
 * Workspace: its own (the predict workspace keeps its bytes), allocated by the first call, counted by tnml_device_bytes, re-made when
 * response_chunk changes, released by tnml_set_input_map and freed by tnml_destroy.  With C = response_chunk rounded up to 64 and
 * B = 32 + the sum over the N - 1 inner bonds of W as it is now of ru16(bond) + ru16(ml) + ru16(mr) of the Label site (site 1 in
 * TNML_MODE_SINGLE):
 *             16 N + 8 nl C + 8 C + 4 (N + 4) + 32 N C    bytes (site table, weights, pred and which, tape regions, the result as the
 *                                                         kernel leaves it [N][2][C] and as the caller gets it [C][N][2])
 *           + 8 B C                                       bytes of tape (grown when W has grown; 0.8 GB at N = 784, m = 120, C = 1 024)
 *           + 2 N C  /  S C + 2 N C + 16 ncodes  /  32 N C   bytes of staging from the first call of that input form on, as predict's. */
#define TNML_RESPONSE_CHUNK_DEFAULT 1024   /* option "response_chunk" */
int tnml_response_u8 (tnml_ctx* ctx, int64_t n, const uint8_t* pixels, const int32_t* which /*[n] or NULL*/,
                      double* resp /*[n][N][2]*/, double* weights /*[n][nl] or NULL*/, int32_t* pred /*[n] or NULL*/);
int tnml_response_phi(tnml_ctx* ctx, int64_t n, const double* phi /*[n][N][2]*/, const int32_t* which,
                      double* resp, double* weights, int32_t* pred);

/* ---- streamed site gradients: dC/dA of every site tensor, on images the context does not hold ----------------------
 * For n images and coefficients c[n][l] = dC/dW_l(x_n) (nl = 10; nl = 1 in TNML_MODE_SINGLE, where site 1 plays the Label site)
 *     G_j[a,s,r]   = sum_n sum_l c_nl dW_l(x_n)/dA_j[a,s,r]          (j not the Label site)
 *     G_c[a,s,r,l] = sum_n       c_nl dW_l(x_n)/dA_c[a,s,r,l]        (the Label site),
 * the gradient with respect to W of any function C of the outputs (a vector-Jacobian product).  Exactly one of coef and labels is
 * non-NULL: coef [n][nl] gives c directly; labels [n] makes the call form c_nl = 2 (W_l(x_n) - y_nl) on the device from its own inward
 * pass, with the targets of tnml_evaluate_* (y_nl = [l == label_n]; TNML_MODE_SINGLE: y_n = [label_n == target_label]), so that G is
 * dC/dA of the cost tnml_evaluate_* reports on the same images.  Mini-batch gradient descent on data that does not fit on the card,
 * or fine-tuning a trained W, is host arithmetic on this array and tnml_set_site.
 * grad receives the sites concatenated in site order, each in the layout of tnml_get_site for W as it is now ([ml][2][mr], x nl on
 * the Label site, first index fastest); tnml_site_gradient_size gives the element count and, when offsets is non-NULL, the N + 1
 * starts (offsets[N] = elems).  grad is overwritten, not added to; it is copied back once, at the end of the call; weights and pred,
 * either may be NULL, are bit for bit those of tnml_predict_* under predict_dtype = 0 and are copied back chunk by chunk.
 * Inputs as tnml_response_*: bytes through the built-in expression or the input map in force, or features; any context with a complete
 * W, data-less ones included.  Reads W only and enters no collective.
 * The host loop cuts n into chunks of option "gradient_chunk" images (default 512).  Per chunk ONE launch of k_site_backward
 * (kernels_sitegrad.hip) walks the chain inward as k_response does, keeping every chain vector on a tape, forms the coefficients at
 * the Label site and walks outward, keeping every outward vector on a second tape; ONE launch of k_site_grad then adds, for every site,
 * the outer products over the chunk's images with v_mfma_f64_16x16x4_f64.  The sum has a fixed order (the kernel file's header states
 * it; no atomics): grad is bit-identical on repeats and independent of the tile width ("predict_tile" is honoured); its last bits
 * may depend on gradient_chunk.
 * Refused as tnml_response_* is, in the same words: on a context attached as a held-out set, while a bond update is in flight, when W
 * is incomplete, when W has a bond dimension above 512, under predict_dtype = 1.  Also refused: both or neither of labels and coef, a
 * label outside 0..9 and a coefficient that is not finite (the message names the image).  A refused call leaves grad untouched; n = 0
 * succeeds and zeroes grad.
 * Workspace: its own, allocated by the first call, counted by tnml_device_bytes, re-made when gradient_chunk changes, released by
 * tnml_set_input_map and freed by tnml_destroy.  With C = gradient_chunk rounded up to 64, B = 32 + the sum over the N - 1 inner bonds
 * of W as it is now of ru16(bond), and E = the elements of grad:
 *             16 N + 16 nl C + 8 C + 4 (N + 2) + 8 (N + 1) + 4 (N + nl)   bytes (site table, weights and coefficients, pred and labels,
 *                                                         tape regions, site starts, output blocks)
 *           + 8 E                                         bytes, the gradient until it is copied back (grown when W has grown)
 *           + 16 B C                                      bytes of the two tapes (grown when W has grown; 0.8 GB at N = 784, m = 120, C = 512)
 *           + 2 N C  /  S C + 2 N C + 16 ncodes  /  32 N C   bytes of staging from the first call of that input form on, as predict's.
 * Option "loss" = TNML_LOSS_SOFTMAX changes the labels mode alone: the thread that owns the image forms, from its ten weights,
 * c_nl = beta (softmax_l(beta W(x_n)) - [l == label_n]) in the fixed arithmetic of tnml_amd/csrc/loss_dev.h (beta = "loss_beta"), so that G is
 * dC/dA of the cost tnml_evaluate_* reports under the same option.  The coef mode, weights, pred, both walks, the GEMM, its order,
 * the workspace and every refusal are untouched; a weight that is not finite makes the image's coefficients NaN.
 * tnml_site_gradient_coef is a test entry like tnml_cg_state: the coefficients [cnt][nl] of the LAST chunk of the last gradient or
 * step call, as given or as formed; count must be cnt nl; refused before any such call since the workspace was made.
 * Option "gradient_dtype" = TNML_GRADIENT_F32 runs tnml_site_gradient_*, tnml_backward_*, tnml_site_step_* and their _dev forms in fp32
 * (the float instantiations of k_site_backward, k_site_grad and k_input_grad: v_mfma_f32_16x16x4_f32, tiles of 64 images up to bond 256,
 * 32 up to 512, 16 up to 1 024) and nothing else; it is independent of "predict_dtype", under which = 1 these calls stay refused.
 * Bonds up to 1 024 are served (above: refused in tnml_predict_*'s words under predict_dtype = 1).  W is rounded to fp32 once per call,
 * features are formed in fp64 and rounded once, given coefficients are rounded once.  The inward pass is the fp32 chain kernel's:
 * weights and pred are bit for bit those of tnml_predict_* under predict_dtype = 1.  In the labels mode c is formed in fp64 from the
 * widened weights by the expressions above and rounded once; tnml_site_gradient_coef returns the rounded values.  Seeds, outward walk
 * and both tapes are fp32.  k_site_grad<float> sums a chunk's images in fp32 from zero and adds the chunk's sum to the fp64 gradient
 * with one fp64 addition per element, so chunk sums add up in fp64 and grad, the norm pass and the optimiser read fp64 as before: a step
 * is mixed precision (fp32 gradient, fp64 master W and state).  dphi receives fp32 values widened exactly (dphi32 of tnml_dev_out: no
 * second rounding).  Order and independence properties are those of the fp64 path (DESIGN.md "Streamed gradients in fp32").
 * A weight that is not finite fails the call with a message that names gradient_dtype: nothing of that chunk or a later one reaches
 * weights, pred or dphi, grad stays untouched, a step applies nothing, the context stays usable.
 * Workspace under gradient_dtype = 1, with W32 = the sum over the sites of their elements rounded up to a multiple of 4:
 *             the first line and 8 E as above
 *           + 8 B C                                       bytes of the two tapes (floats: half)
 *           + 4 W32 + 16 N + 4                            bytes: the fp32 copy of W (grown when W has grown), its site table, the range flag
 *           + 2 N C  /  S C + 2 N C + 16 ncodes + 8 ncodes  /  16 N C + 8 N C   bytes of staging (bytes / input map with its table in fp64
 *                                                         and fp32 / features as given and site-first in fp32).
 * A change of the option frees the two tapes and makes them again in the new element size; what the other value allocated (the fp32
 * copy and table, the site-first features of either type) stays until the workspace is released; the optimiser state is not touched. */
#define TNML_GRADIENT_CHUNK_DEFAULT 512    /* option "gradient_chunk" */
int tnml_site_gradient_size(tnml_ctx* ctx, int64_t* elems, int64_t* offsets /*[N+1] or NULL*/);
int tnml_site_gradient_u8 (tnml_ctx* ctx, int64_t n, const uint8_t* pixels, const int32_t* labels /*[n] or NULL*/, const double* coef /*[n][nl] or NULL*/,
                           double* grad /*[elems]*/, double* weights /*[n][nl] or NULL*/, int32_t* pred /*[n] or NULL*/);
int tnml_site_gradient_phi(tnml_ctx* ctx, int64_t n, const double* phi /*[n][N][2]*/, const int32_t* labels, const double* coef,
                           double* grad, double* weights, int32_t* pred);
int tnml_site_gradient_coef(tnml_ctx* ctx, double* out /*[cnt][nl]*/, int64_t count);

/* ---- streamed input gradients: dC/dphi of every site's feature, beside or instead of dC/dA -----------------------------
 * The other half of a backward pass.  For n images and the coefficients c[n][l] = dC/dW_l(x_n) of tnml_site_gradient_*
 *     dphi[n][j][s] = sum_l c_nl dW_l(x_n)/dphi_{n,j}[s],
 * the vector-Jacobian product with respect to the inputs.  W is linear in the feature of each site, so dphi[n][j] is also the pair of
 * outputs sum_l c_nl W_l(x_n with phi_j := e_s), and sum_s phi_{n,j}[s] dphi[n][j][s] = sum_l c_nl W_l(x_n) at every site.
 * Inputs, the labels / coef rule, the options "loss" / "loss_beta", "gradient_chunk" and "predict_tile", the input map and the per-label
 * variant are those of tnml_site_gradient_*; the call shares that call's workspace and its k_site_backward launch.  Under an input map
 * dphi is the gradient with respect to the features of the N reduced sites (the table rows the block sums select).
 * grad non-NULL: k_site_grad runs and grad is bit for bit what tnml_site_gradient_* returns on the same arguments.  grad NULL: that launch
 * is left out.  dphi non-NULL: per chunk ONE launch of k_input_grad (kernels_inputgrad.hip) reads the two tapes and forms one bilinear
 * form per site, feature component and image with v_mfma_f64_16x16x4_f64, in a fixed order (the kernel file's header states it; no
 * atomics): an image's values do not depend on n, on the chunk, on the tile width or on the tile it lands in, and repeats are
 * bit-identical.  dphi is copied back chunk by chunk.  weights and pred, either may be NULL, are bit for bit those of tnml_predict_*.
 * Refused as tnml_site_gradient_* is, in the same words; also refused: grad and dphi both NULL.  A refused call leaves grad and dphi
 * untouched; n = 0 succeeds, zeroes grad (when given) and touches nothing else.  Reads W only and enters no collective.
 * Workspace: that of tnml_site_gradient_* (same formula, same bytes) and, from the first call that asks for dphi on,
 *             32 N C    bytes (dphi of a chunk as the kernel leaves it [N][2][C] and as the caller gets it [C][N][2]; C = gradient_chunk
 *                       rounded up to 64), counted by tnml_device_bytes, re-made when gradient_chunk changes, released by
 *                       tnml_set_input_map with the gradient workspace and freed by tnml_destroy.
 * tnml_forward_taped_* followed by tnml_backward_taped* (below) allocates exactly these bytes for the same input form and outputs:
 * the forward everything but the 32 N C (16 N C for device-resident outputs), the first backward that asks for dphi those.
 * tnml_set_sites_dev adds 32 N bytes (its table) from its first call on. */
int tnml_backward_u8 (tnml_ctx* ctx, int64_t n, const uint8_t* pixels, const int32_t* labels /*[n] or NULL*/, const double* coef /*[n][nl] or NULL*/,
                      double* grad /*[elems] or NULL*/, double* dphi /*[n][N][2] or NULL*/, double* weights /*[n][nl] or NULL*/, int32_t* pred /*[n] or NULL*/);
int tnml_backward_phi(tnml_ctx* ctx, int64_t n, const double* phi /*[n][N][2]*/, const int32_t* labels, const double* coef,
                      double* grad, double* dphi, double* weights, int32_t* pred);

/* ---- gradient steps on the device: SGD with momentum and Adam on the streamed site gradient ---------------------------
 * One call is one optimiser step on W.  The gradient G of the n images is summed on the device exactly as tnml_site_gradient_* sums
 * it (same inputs, labels / coef rule, gradient_chunk, predict_tile, input map, per-label variant and order: the same bits), then the
 * optimiser reads it where it lies and rewrites the site tensors in place.  Nothing of the size of W crosses the bus in either
 * direction: after the stream is synchronised only the report is copied back.  A context that holds no data can so be trained by
 * mini-batch SGD or Adam at the speed of its kernels.
 * The arithmetic (kernels_sitestep.hip states it in full; tests/sitestep_model.py restates it in numpy).  Every operation is one IEEE
 * fp64 rounding, nothing is contracted, quotient and root are the correctly rounded ones:
 *   total     = the sum of g^2 over the flat gradient as grad of tnml_site_gradient_* lays it out, in a fixed order: blocks of
 *               65 536 consecutive elements, one workgroup of 256 threads each (thread t adds elements t, t + 256, ... in ascending
 *               order, then the tree of k_eval_tally over the threads), the block sums added in block order by one thread; no atomics
 *   grad_norm = |scale| sqrt(total);  factor f = scale, or scale (clip / grad_norm) when clip > 0 and grad_norm > clip (clipped = 1)
 *   gh        = f g
 *   SGD:   v <- mu v + gh;  A <- A - lr v
 *   Adam:  p1 <- p1 beta1, p2 <- p2 beta2 (both start at 1: one multiplication per step, never a pow); c1 = 1 - p1, c2 = 1 - p2;
 *          m <- beta1 m + (1 - beta1) gh;  v <- beta2 v + ((1 - beta2) gh) gh;  A <- A - lr ((m / c1) / (sqrt(v / c2) + eps))
 * When total is not finite nothing is applied: W, the optimiser state and t stay bit for bit as they were, the call fails with a
 * message that gives the norm, and the context stays usable.  The decision is taken on the device (the update kernel reads the flag
 * the norm pass left).
 * The report: t, grad_norm, factor, clipped; eval -- in the labels mode the report tnml_evaluate_* gives for the batch at the W BEFORE
 * the step under predict_chunk = gradient_chunk (one k_eval_tally launch per chunk on the chunk's weights), in the coef mode zero but
 * for n.  rep may be NULL.
 * The optimiser state (v for SGD; m and v for Adam, each laid out like grad) is allocated by the first step, for that method and for
 * the site shapes of W at that moment; hyper-parameters may change from call to call.  A step under the other method, or on a W whose
 * site shapes have changed, is refused with a message that names the site and tnml_site_step_reset.  The state is counted by
 * tnml_device_bytes, freed by tnml_site_step_reset (t then starts over) and tnml_destroy, and is no part of the gradient workspace:
 * it survives a change of gradient_chunk and tnml_set_input_map.  With E = the elements of grad and k = 1 (SGD) or 2 (Adam):
 *             8 k E + 8 ceil(E / 65536) + 4 (N + 1) + 64 + 1040   bytes (the state, the block sums, the first update block of every
 *                                                         site, the norm pass's result, the tallies of the call)
 * on top of the workspace of tnml_site_gradient_* for the input form.
 * A step does to the context what tnml_set_site on every site does: environments, bond and outputs are no longer current
 * (tnml_env_init before the next bond update), placements and the bond histories start over.
 * Refused as tnml_site_gradient_* is, in the same words (in flight, attached as a held-out set, W incomplete, a bond above 512,
 * predict_dtype = 1, both or neither of labels and coef, a bad label, a coefficient that is not finite); as tnml_set_site is on a
 * training context with a held-out context attached; on a context of a multi-rank run (nranks != 1: no collective is entered, the
 * replicas would part); with p NULL or a parameter outside its range (the message names it).  n = 0 succeeds: no step is taken, the
 * report is zeroed.
 * Option "loss" = TNML_LOSS_SOFTMAX: in the labels mode the gradient is tnml_site_gradient_*'s under that option and eval is
 * tnml_evaluate_*'s under it (cross-entropy cost, signed decision).  The optimiser, the coef mode, the state and the refusals are
 * untouched; coefficients that are NaN (a weight that is not finite) make total not finite, and the step is refused as above.
 * tnml_site_step_state is a test entry like tnml_cg_state: "m" (Adam) or "v" (both methods), count = E doubles. */
#define TNML_STEP_SGD  0
#define TNML_STEP_ADAM 1
typedef struct {
    int    method;              /* TNML_STEP_SGD | TNML_STEP_ADAM */
    double lr;                  /* finite, > 0 */
    double momentum;            /* SGD:  mu in [0, 1) */
    double beta1, beta2, eps;   /* Adam: betas in [0, 1), eps > 0 */
    double clip;                /* > 0: bound on the norm of the scaled gradient; 0: none */
    double scale;               /* finite, non-zero: the gradient is multiplied by it (1/n, say) */
} tnml_step_params;
typedef struct {
    int64_t t;                  /* steps this state has taken, this one included */
    double  grad_norm;          /* |scale| ||G||_2 over all sites */
    double  factor;             /* f above: what G was multiplied by */
    int     clipped;
    tnml_eval_report eval;      /* labels mode: the batch at the W BEFORE the step; coef mode: zero but for n */
} tnml_step_report;
int tnml_site_step_u8 (tnml_ctx* ctx, int64_t n, const uint8_t* pixels, const int32_t* labels /*[n] or NULL*/, const double* coef /*[n][nl] or NULL*/,
                       const tnml_step_params* p, tnml_step_report* rep /* or NULL */);
int tnml_site_step_phi(tnml_ctx* ctx, int64_t n, const double* phi /*[n][N][2]*/, const int32_t* labels, const double* coef,
                       const tnml_step_params* p, tnml_step_report* rep);
int tnml_site_step_reset(tnml_ctx* ctx);                                                    /* frees the optimiser state; t starts over */
int tnml_site_step_state(tnml_ctx* ctx, const char* which /* "m" | "v" */, double* out, int64_t count);

/* ---- device-resident arguments: the streamed calls on arrays that already live on the device ---------------------------
 * tnml_predict_dev, tnml_evaluate_dev, tnml_response_dev, tnml_backward_dev (which covers tnml_site_gradient_*: give grad alone) and
 * tnml_site_step_dev are the host-pointer calls of their names with every array of the batch and every output in device memory of the
 * context's device: a tensor another library made there (a torch CUDA tensor's data_ptr(), say) is served without crossing the bus.
 * Same meaning: the labels / coef rule, "loss" / "loss_beta", the input map (pixels is then [n][src_rows*src_cols]), the per-label
 * variant, "predict_dtype" for predict and evaluate, the chunk options and "predict_tile", the refusals in the same words, n = 0 and
 * what a step does to the context are those of the host-pointer calls.  Same code, same kernels, same bits: both families run the
 * same chunk loop with the memory space as a parameter, and every output is bit for bit the host-pointer call's on the same values.
 * The batch: exactly one of pixels, phi and phi32.  phi32 holds fp32 features; k_chain_stage_phi widens them (exactly) while it
 * stages, so the results are those of phi on the widened values.  The outputs: any may be NULL; what a call does not produce is
 * ignored (predict / evaluate: weights, pred; response: resp, weights, pred; backward: grad, dphi or dphi32, weights, pred).  At most
 * one of dphi and dphi32; dphi32 is dphi rounded once to fp32 by the transposing kernel.  rep stays a host pointer.
 * What moves: nothing of the size of the images.  The stage kernels (k_chain_stage_u8, k_chain_stage_phi, k_stage_codes) read the
 * caller's array at the chunk's offset; the chain kernels write weights and pred into the caller's arrays at the chunk's offset; the
 * transposing kernel writes resp, dphi and dphi32 into the caller's arrays.  Device-to-device copies that remain, and why:
 *   labels, coef, which : a chunk's worth into the small staging arrays of the workspace (4 C, 8 nl C, 4 C bytes): the labels mode
 *                         overwrites the coefficients in that array, and tnml_site_gradient_coef reads it afterwards;
 *   grad                : ONE copy of 8 E bytes at the end of the call: the sum is made in the workspace's gradient, where
 *                         tnml_site_step_dev's optimiser reads it, so that the call's bits and launches are the host call's.
 * Stream contract.  batch->stream is the hipStream_t that last wrote the inputs (NULL: the null stream).  On entry the call records an
 * event on it and makes the context's stream wait for that event; the caller's stream is never synchronised by the host.  Before it
 * returns, the call synchronises the context's stream, as every streamed call does: on return the outputs are complete for any
 * stream, and no argument is read any more (an allocator may recycle it).  One event per context, made by the first _dev call with
 * timing disabled, released with the check block (below) and by tnml_destroy.
 * Pointer checks, made before hipSetDevice and before anything is launched or allocated.  Every non-NULL array of the batch and every
 * non-NULL output the call produces must be, as hipPointerGetAttributes and hipMemGetAddressRange describe it: device memory (what
 * the runtime does not know -- plain malloc memory --, managed memory and host memory registered with the runtime are refused and
 * never dereferenced); on the context's device; aligned to its element (8 bytes for doubles, 4 for int32 and float); with the bytes
 * the call needs lying inside its allocation (a pointer into the middle of an allocation is fine).  No output may share a byte with
 * an input or another output.  The message names the argument and the reason.
 * Value checks.  Where the host-pointer calls walk labels / coef / which on the CPU, these calls make ONE launch of k_check_batch
 * (kernels_iocheck.hip, profile class "io_check") over the whole batch before the chunk loop -- a call with none of the three arrays
 * makes the launch too, with nothing to walk, and does not read the block back --, read its 24-byte block once, and refuse in the host
 * path's words ("label %d of image %lld out of range",
 * "coefficient %d of image %lld is not finite", "which = %d of image %lld out of range 0..%d": the smallest offending index, as the
 * host loop finds it).  A refused call leaves every output untouched.  Beyond that launch the launches of a call, class by class,
 * are the host-pointer call's.
 * Workspace: the host-pointer call's formulas without the buffer the images are copied into (2 N C of the bytes form's 2 N C, S C of
 * the map form's, 16 N C of the features form's 32 N C; predict's fp32 features form: 16 N C of its 24 N C) and without the transposed
 * result (16 N C of response's and of backward's 32 N C); a later host-pointer call of that form adds them, and host-pointer calls
 * allocate exactly what they allocated before.  On top, made by the first _dev call (n > 0):
 *             24    bytes (the block of k_check_batch), counted by tnml_device_bytes.  The block and the event are released with the
 *                   workspaces -- when the last of the predict, response and gradient workspaces is released (a changed chunk option,
 *                   tnml_set_input_map, tnml_destroy) -- and made again by the next _dev call.
 * tnml_set_site_dev / tnml_get_site_dev are tnml_set_site / tnml_get_site (same rules, same words) on a device array in
 * tnml_get_site's layout: the same pointer checks, the same entry wait on `stream`, ONE device-to-device copy on the context's
 * stream and a synchronisation before they return.
 * tnml_abi_layout is a test entry: for name = "tnml_dev_batch" / "tnml_dev_out" it writes sizeof and then the offset of every field
 * in declaration order to sizes_out (16 entries suffice) and returns how many it wrote; -1 for another name. */
typedef struct {
    int64_t        n;
    const uint8_t* pixels;   /* device [n][N], or [n][S] under an input map */
    const double*  phi;      /* device [n][N][2] */
    const float*   phi32;    /* device [n][N][2], widened exactly to fp64 while staging */   /* exactly one of the three */
    const int32_t* labels;   /* device [n] or NULL */
    const double*  coef;     /* device [n][nl] or NULL */
    const int32_t* which;    /* device [n] or NULL (responses only) */
    void*          stream;   /* hipStream_t that last wrote the inputs; NULL = the null stream */
} tnml_dev_batch;
typedef struct { double* weights; int32_t* pred; double* resp; double* grad; double* dphi; float* dphi32; } tnml_dev_out;  /* device, any may be NULL */
int tnml_predict_dev  (tnml_ctx* ctx, const tnml_dev_batch* batch, const tnml_dev_out* out);
int tnml_evaluate_dev (tnml_ctx* ctx, const tnml_dev_batch* batch, const tnml_dev_out* out, tnml_eval_report* rep /* host */);
int tnml_response_dev (tnml_ctx* ctx, const tnml_dev_batch* batch, const tnml_dev_out* out);
int tnml_backward_dev (tnml_ctx* ctx, const tnml_dev_batch* batch, const tnml_dev_out* out);
int tnml_site_step_dev(tnml_ctx* ctx, const tnml_dev_batch* batch, const tnml_step_params* p, tnml_step_report* rep /* host, or NULL */);
int tnml_set_site_dev (tnml_ctx* ctx, int j, int ml, int mr, int has_label, const double* A_dev, void* stream);
int tnml_get_site_dev (tnml_ctx* ctx, int j, double* A_dev, void* stream);
int tnml_abi_layout(const char* name, int64_t* sizes_out);

/* ---- backward from the forward's tape: a training step that walks the chain inward once --------------------------------
 * tnml_predict_* followed by tnml_backward_*(coef = ...) walks the chain inward twice: the backward's first half is the forward again.
 * tnml_forward_taped_* is that first half alone, on the gradient workspace under option "gradient_dtype" (not "predict_dtype"): ONE
 * launch of k_forward_taped (kernels_sitegrad.hip, profile class "fwd_taped") that leaves weights, pred and the inward tape.  It
 * shares the refusals, the staging, the fp32 copy of W, "predict_tile" and the input map with tnml_backward_*, so weights and pred are
 * bit for bit those of tnml_predict_* under the matching "predict_dtype".  n must not exceed "gradient_chunk" (a tape belongs to one
 * chunk; a larger n is refused), n = 0 succeeds with *ticket = 0, which is never valid; under fp32 a weight outside the fp32 range
 * fails the call as it fails tnml_backward_*, and leaves no ticket.  On success *ticket is a positive number this context has never
 * given out before.
 * tnml_backward_taped / tnml_backward_taped_dev take the ticket and coefficients [n][nl] (no labels: an autograd caller has
 * grad_output), and return grad and / or dphi bit for bit as tnml_backward_* does for the same images and coefficients under the
 * same options.  Per call: one copy of the coefficients, the gradient zeroed when grad is asked for, ONE launch of k_site_outward
 * (class "site_out": the two outward walks in two workgroups per tile), k_site_grad when grad is asked for, k_input_grad when dphi
 * is, the copies out.  No site table, fp32 copy of W or image is staged again.  The rules are tnml_backward_*'s: a coefficient that
 * is not finite is refused (on the host, or by k_check_batch), grad and dphi both NULL is refused, and the _dev form makes the
 * pointer checks and keeps the stream contract and dphi32 of the device-resident calls.  A backward of either memory space serves
 * a forward of either.  The ticket stays valid after a backward: ten calls with unit coefficient rows give the Jacobian of one forward.
 * tnml_site_gradient_coef afterwards returns the coefficients as given, under fp32 too: as tnml_backward_* leaves them (the kernels
 * round them to fp32 as they read them).
 * A context has at most one live ticket.  It dies -- and the context keeps the name of what took the tape, which a refused backward
 * gives with the ticket -- with any other call that uses the gradient workspace on n > 0 images (tnml_site_gradient_*, tnml_backward_*,
 * tnml_site_step_*, their _dev forms, a new tnml_forward_taped_*), with anything that writes W (tnml_set_site, tnml_set_site_dev,
 * tnml_set_sites_dev, tnml_mps_place, tnml_mps_compress, a bond update, a step), and with a release or re-make of the workspace or
 * its tapes (a changed "gradient_chunk" or "gradient_dtype" when the ticket is next looked at, tnml_set_input_map).  "predict_tile",
 * "loss" and "predict_dtype" may change: the backward uses the tile width the forward ran with.  A refused backward leaves every output
 * untouched and the context usable.  tnml_tape_ticket gives the live ticket and its image count, 0 and 0 when there is none.
 * Workspace: forward and backward together allocate exactly what tnml_backward_* allocates for the same input form and outputs
 * (the formulas above; the 32 N C of dphi with the first backward that asks for it).
 * tnml_set_sites_dev is tnml_set_site_dev for count sites in the shapes W has now -- an optimiser step, not a change of bond
 * dimensions: sites[k] in 1..N, set, none named twice, A_dev[k] a device array in tnml_get_site's layout under the pointer checks of
 * the _dev calls.  Every check is made before anything is written.  Then one entry wait on `stream`, one upload of a table of
 * (source, destination, elements, first block), ONE launch of k_sites_gather (class "sites_copy") and one synchronisation.  count = 0
 * does nothing.  The table takes 32 N bytes from the first call on, counted by tnml_device_bytes and released with the check block. */
int tnml_forward_taped_u8 (tnml_ctx* ctx, int64_t n, const uint8_t* pixels, double* weights, int32_t* pred, int64_t* ticket);
int tnml_forward_taped_phi(tnml_ctx* ctx, int64_t n, const double* phi, double* weights, int32_t* pred, int64_t* ticket);
int tnml_forward_taped_dev(tnml_ctx* ctx, const tnml_dev_batch* batch, const tnml_dev_out* out /* weights, pred */, int64_t* ticket);
int tnml_backward_taped    (tnml_ctx* ctx, int64_t ticket, const double* coef /* host [n][nl] */, double* grad, double* dphi);
int tnml_backward_taped_dev(tnml_ctx* ctx, int64_t ticket, const double* coef_dev, const tnml_dev_out* out /* grad, dphi | dphi32 */, void* stream);
int tnml_tape_ticket(tnml_ctx* ctx, int64_t* ticket, int64_t* n);
int tnml_set_sites_dev(tnml_ctx* ctx, int count, const int32_t* sites, const double* const* A_dev, void* stream);

/* ---- held-out evaluation during training ----------------------------------------------------------
 * A held-out set is an ordinary context created for the held-out images (one rank: nranks = 1, its own shard of the set in
 * a multi-rank run).  Once attached to a training context, every bond update of `train` also moves the two site tensors it
 * rewrote to `heldout` and -- after the split is final (a speculative split once its deferred check has passed in
 * tnml_bond_update_end; nothing of a rolled-back split is kept) -- runs on heldout's own stream the forward pass at the new
 * bond tensor, the cost / #correct reduction and the environment shift that train does at the end of that bond update.
 * Training reports and W are bit-identical with and without a held-out context.  While attached, calls that would change
 * heldout's W, environments, data or bond are refused (read-only calls keep working), and so are the calls that would change
 * train's W or environments outside a bond update; tnml_destroy of either context detaches first. */
typedef struct {
    int bond, half;                /* the bond update these values follow; bond = 0: W as it was at attach time */
    int64_t count;                 /* held-out images of this context (local: no collective is entered) */
    int64_t ncorrect;              /* decision rule of tnml_classify for the context's mode */
    double cost;                   /* sum over images and labels of (W_l(x_n) - y_nl)^2; no regulariser */
    double label_cost[TNML_NL];    /* split per label as tnml_bond_report::label_cost is */
} tnml_heldout_report;
/* Refused, with a message naming the mismatch, unless: same device, N, mode, target_label and dtype; heldout's maxm >= train's,
   heldout has nranks = 1 and image data; no bond update of train in flight; train at a sweep start (environments as
   tnml_env_init left them, or the last bond update ended a sweep under tnml_sweepnext).  Copies train's W into heldout,
   builds heldout's environments and computes the bond-0 values. */
int tnml_heldout_attach(tnml_ctx* train, tnml_ctx* heldout);
int tnml_heldout_detach(tnml_ctx* train);
/* the values of the last bond update ended (tnml_bond_update_end), or of attach; waits for them if they are not ready yet */
int tnml_heldout_read(tnml_ctx* train, tnml_heldout_report* rep);

/* ITensor truncate(): p = sigma^2 descending; returns kept m */
int tnml_truncate(const double* p, int n, int maxm, int minm, double cutoff, double* truncerr);
/* ITensor sweepnext (fixedL.cc:478) */
void tnml_sweepnext(int* b, int* ha, int N);
/* contiguous image shard of `rank`: ParallelDo's chunking with GPUs as threads (paralleldo.h:32-43) */
void tnml_shard_bounds(int64_t NT_total, int nranks, int rank, int64_t* begin, int64_t* end);

/* ---- measurement -------------------------------------------------------------------------- */
/* per-kernel-class HIP-event timing on the context's stream (bench.py roofline figures) */
int tnml_profile_enable(tnml_ctx* ctx, int on);
/* restrict the timing to one kernel class (e.g. "fgemm_fwd") or a comma-separated list of classes, or NULL / "" for all classes: two event
   records per timed launch cost host time, so a throughput measurement should time only what it reports */
int tnml_profile_select(tnml_ctx* ctx, const char* class_name);
int tnml_profile_count(tnml_ctx* ctx);
int tnml_profile_get(tnml_ctx* ctx, int idx, char* name64, int64_t* launches, double* total_ms);
int tnml_profile_reset(tnml_ctx* ctx);
int tnml_synchronize(tnml_ctx* ctx);
/* run-time options; a value outside an option's range, or an unknown name, is refused.  Where an environment variable is named it
   supplies the default at tnml_create (and a bad value there makes tnml_create fail).  Bool options take any value, nonzero = on.
   The algebraic shortcuts and checks (defaults: all 1):
     "fast_cg"        (TNML_FAST_CG) P <- P + a (p*t.v) instead of re-running the forward GEMM inside cgrad (single.h:290-398 idea)
     "reuse_p"        (TNML_REUSE_P) the after-SVD quadcost of one bond update provides the first residuals of the next
     "fuse_z"         (TNML_FUSE_Z) the gradient GEMM builds Z = sum_l EL[l] dP[l] itself
     "merged_cg"      (TNML_MERGED_CG) one all-reduce per CG pass instead of two: the image sum of a pass is A p = sum_n (p.v_n) v_n, formed from the
                      pAp pass's own outputs, and travels with sum |p.v_n|^2; the residual follows r <- r - a (A p + lambda p)
                      (the structure of the reference's own fast_cgrad, single.h:347-379); needs fast_cg.  1 (default): on ranks that
                      have a communicator -- where it halves the collectives; a single rank keeps the reference's literal residual
                      (the recurrence moves the 4th step size of an ill-conditioned Label-on-B bond by 1e-3, the cost by 1e-10);
                      2: always; 0: never
     "defer_tail"     (TNML_DEFER_TAIL) multi-rank: the cost partials of the "after SVD" quadcost and the replica fingerprint ride in the first
                      all-reduce of the NEXT bond update (tnml_bond_update_end issues one small all-reduce when nothing followed);
                      with both on a bond update enters 5 payload all-reduces instead of 9 + 1 (default 1)
     "check_replicas" (TNML_CHECK_REPLICAS) multi-rank: fingerprint check of the two site tensors a split rewrote (1, default: folded into the packed
                      sum all-reduce as exact integer pieces, a mismatch is an error when the report is handed out; 2: checked at
                      once inside the bond update, before anything consumes the tensors -- one extra 8-double all-reduce and a
                      host synchronisation -- and on a mismatch rank 0's two tensors are re-broadcast, the sweep continues,
                      tnml_replica_repairs counts; 0: off)
     "fg64_cfg", "ldot_cfg"  (TNML_FG64_CFG, TNML_LDOT_CFG) force a tile configuration of the feature GEMM / the label dot that is
                      otherwise chosen by the image count (2 / 1 = the large-image-count forms bench.py times; parity tests run them at
                      small sizes; ldot_cfg 2 = the small-shard form)
     "fused_fwd"      (TNML_FUSED_FWD) the forward pass of a Label-on-environment bond at m = 120 as one persistent kernel (feature GEMM +
                      label dot of the previous tile, kernels_fused.hip): 1 = from 14 336 images per rank on (default),
                      0 = never, 2 = always (parity tests at small sizes), > 2 = always with that many workgroups at most
     "cg_method"      TNML_MODE_SINGLE only: 0 = conj (single.h:162-288, default), 1 = fast_conj (single.h:290-398: one image sum
                      per CG step, residual by recurrence, the reference's regulariser term as written, no cost in the trace),
                      2 = exact (single.h:117-160, see tnml_exact; "pcut" through tnml_set_option_real)
     "sytrd_exit"     the split's tridiagonalisation stops once the trailing block of the Gram matrix is numerically zero
                      (trace <= 1e-15 trace(G); default 1; 0 = all n-2 Householder steps)
   Kernel selection (0 never, 1 by shape and image count (default), 2 always):
     "fwd_res", "shift_res"  (TNML_FWD_RES, TNML_SHIFT_RES) the resident-operand forward pass / Label-carrying shift (kernels_res.hip);
                      fwd_res 3 = the general form on 120 x 120 bonds too
     "shift_skip"     (TNML_SHIFT_SKIP) the resident-operand shift walks a tile's images zero features first and leaves out the odd-row
                      products of 16-image groups whose phi[1] is 0 throughout (default 1; 0 = natural order, every product; same values)
     "fwd_skip"       (TNML_FWD_SKIP) the same in the GEMM waves of the resident-operand forward pass on 120 x 120 bonds: 32-image tiles,
                      the odd-row chain of a group left out (default 1; 0 = natural order, every product; same values)
     "grad_quad"      (TNML_GRAD_QUAD) the resident-accumulator gradient GEMM (kernels_grad.hip)
     "grad_pair"      (TNML_GRAD_PAIR) its pair form for bonds up to 64 x 64 (default 1; 0 = the quad form)
     "bgs_chol"       (TNML_BGS_CHOL) block Gram-Schmidt Cholesky QR of a kept basis of 129-384 columns (default 1; 0 = dpotrf + dtrsm)
     "spec_split"     (TNML_SPEC_SPLIT) the speculative split without its host synchronisation (default 1)
     "spec_predict"   (TNML_SPEC_PREDICT) truncating splits (minm < the columns the split may keep) take the speculative form too, on a
                      PREDICTED column count: the count the bond kept at its last two finished visits when both agree at the same matrix
                      side (otherwise the synchronous split).  A kernel applies the truncation rule to the eigenvalues on the device and
                      tnml_bond_update_end rolls a wrong guess back like a failed check, repeating with the synchronous split: every
                      number is that of a run without the option.  tnml_set_site clears the history of the two bonds of its site;
                      tnml_svd_split and tnml_mps_compress neither read nor write it (default 0; tnml_spec_predict_stats)
     "bf16_grad", "bf16_once"  the bf16 modes: gradient GEMM on the bf16 pipe / operands converted once (default 1 each)
   Tuning and test knobs (0: the default):
     "res_pace"       (TNML_RES_PACE) 0-4, pause pattern of the GEMM waves of k_fwd_res (0: the default of the form that runs -- natural
                      order and zero features first have their own)
     "res_grid"       workgroups of the resident-operand kernels
     "bgemm_wgs", "bgemm_per"  (TNML_BGEMM_WGS, TNML_BGEMM_PER) workgroups the gradient GEMM aims at / images per slab in units of 32
     "mc_spin_max"    polls before the workgroup cluster of the tridiagonalisation gives up (-1 default; 0 forces the fallback)
     "debug_fail_split"  k >= 0: the k-th speculative split reports a failed check (-1 off)
     "debug_mispredict"  k >= 0: the guess of the k-th predicted split of the context is moved by one column (down while that leaves one,
                      up otherwise) before anything is enqueued -- a host-side change, no kernel carries a switch (-1 off).  EVERY rank of
                      a communicator must set the same value: ranks that keep different column counts enter collectives of different sizes
     "debug_nudge_rank"  this rank's copy of a split site tensor is moved by one ulp (-1 off)
     "svd_print"      (TNML_SVD_PRINT) k >= 0: print the spectrum of the k-th split; -1: the check values of every split (-2 off)
     "predict_tile"   images per workgroup of the chain kernel of tnml_predict_*: 16, 32 or 64, capped by what the LDS holds at W's largest bond
                      dimension (64 up to 128, 32 up to 256, 16 up to 512; under predict_dtype = 1: 64 up to 256, 32 up to 512, 16 up to 1 024); 0: that cap, halved while workgroups are fewer than compute units
     "predict_dtype"  arithmetic of tnml_predict_*: 0 (TNML_PREDICT_F64, default) fp64 MFMA on the fp64 master W, bonds up to 512;
                      1 (TNML_PREDICT_F32) the fp32 chain kernel on an fp32 copy of W made per call, bonds up to 1 024; any other value is refused
   Memory and transport:
     "predict_chunk"  images per trip of the host loop of tnml_predict_* = per launch of the chain kernel (1..2^20, default 8192); sizes its workspace
     "response_chunk" images per trip of the host loop of tnml_response_* = per launch of k_response (1..2^20, default 1024); sizes its workspace
     "loss"           the loss of tnml_evaluate_* and of the labels mode of tnml_site_gradient_* / tnml_site_step_*: 0 (TNML_LOSS_QUADRATIC, default)
                      sum (W_l - y_l)^2; 1 (TNML_LOSS_SOFTMAX) softmax cross-entropy on the logits loss_beta W_l, refused in TNML_MODE_SINGLE; any other value is refused
     "gradient_chunk" images per trip of the host loop of tnml_site_gradient_* = per launch of k_site_backward and k_site_grad (1..2^20, default 512); sizes its workspace
     "gradient_dtype" arithmetic of tnml_site_gradient_* / tnml_backward_* / tnml_site_step_* and their _dev forms: 0 (TNML_GRADIENT_F64, default) fp64 on the
                      master W, bonds up to 512; 1 (TNML_GRADIENT_F32) the fp32 gradient kernels on an fp32 copy of W made per call, bonds up to 1 024, tapes of
                      half the bytes; any other value is refused.  No environment variable; independent of "predict_dtype"
     "env_budget_mb"  cap on the environment slabs held on the device, the rest spills to host memory (0: none)
     "env_async"      the host tier's copies beside the compute stream (default 1)
     "comm_timeout_s" how long a rank of an in-process or one-shot communicator waits for its peers (>= 1, default 120)
   fast_cg = reuse_p = 0 is the reference's literal evaluation order (fixedL.cc:374-421). */
int tnml_set_option(tnml_ctx* ctx, const char* name, int value);
/* real-valued options: "pcut" (PCut of the exact solver inside tnml_bond_update, single.cc:50, default 1E-8);
   "noise" (TNML_MODE_SINGLE, fp64 storage: the noise of the sweeps, single.cc:25,222 -- from 1E-14 on tnml_svd_split / tnml_bond_update split
   through the density matrix of site c plus noise * sum_n dr_n dr_n^dag, single.h:648-672: W_c = UU, W_{c+dc} = UU * B);
   "loss_beta" (the inverse temperature of option "loss" = TNML_LOSS_SOFTMAX: the logits are loss_beta W_l; default 1, must be finite and > 0.
   A W trained by the sweep has outputs in about [0, 1], where 1 gives nearly flat probabilities).  Neither "loss" nor "loss_beta" has an
   environment variable. */
int tnml_set_option_real(tnml_ctx* ctx, const char* name, double value);
/* The speculative split (minm >= the columns the split may keep: no host synchronisation inside tnml_bond_update_begin): how many splits
   ran speculatively, how many were ROLLED BACK by tnml_bond_update_end because their deferred orthogonality check failed (each repeats
   that bond update with the synchronous split, and the one begun after it), and the device time of the repeated work in ms (event-timed;
   call after tnml_synchronize for the full sum).  fixedL.cc:519-521 has no counterpart: ITensor's svd is synchronous. */
int tnml_split_stats(tnml_ctx* ctx, int64_t* spec_splits, int64_t* roll_backs, double* roll_back_ms);
/* Predicted splits (option "spec_predict"): how many splits ran the speculative form on a predicted column count, how many of them
   tnml_bond_update_end rolled back because the truncation rule kept another count, and the device time in ms of the work repeated for
   those (event-timed; call after tnml_synchronize for the full sum).  Predicted splits also count in tnml_split_stats' spec_splits,
   mispredictions in its roll_backs and roll_back_ms -- but never in tnml_svd_stats' fallbacks: the eigensolver did not fail. */
int tnml_spec_predict_stats(tnml_ctx* ctx, int64_t* predicted, int64_t* mispredicted, double* redo_ms);
/* TEST ENTRY: the device-side truncation rule of the predicted split (k_truncate_verdict) on a spectrum given by the host.
   evals_ascending[n] are eigenvalues as the eigensolver leaves them (ascending; values that are not > 0, NaN included, count as 0).
   *m = the count tnml_truncate keeps for (maxm, minm, cutoff) on the same values read largest first, *wrong = (*m != m_pred).
   Synchronises the stream; not for use while a bond update is in flight. */
int tnml_truncate_device(tnml_ctx* ctx, const double* evals_ascending, int n, int maxm, int minm, double cutoff, int m_pred, int* m, int* wrong);
/* The tile order tables of the resident-operand shift (option "shift_skip"; fp64 storage, TNML_MODE_FIXEDL, maxm >= 33), built when the data
   are set: for site 1..N the number of 16-image groups (padded image count / 16) and how many of them hold only images with phi[1] == 0
   once each 64-image tile is walked zero features first -- the groups whose odd-row products are left out. */
int tnml_shift_skip_stats(tnml_ctx* ctx, int site, int64_t* groups, int64_t* skipped);
/* The same for the tile order table of the resident-operand forward pass (option "fwd_skip"; the same contexts): the groups that hold only
   images with phi[1] == 0 once each 32-image tile is walked zero features first -- the groups whose odd-row chain is left out. */
int tnml_fwd_skip_stats(tnml_ctx* ctx, int site, int64_t* groups, int64_t* skipped);
/* health of the in-house eigensolver: number of fallbacks to rocSOLVER so far, number of splits whose kept basis
   held an eigenvalue cluster and was re-orthonormalised by Cholesky QR, and max|Q^T Q - I| of the kept basis
   before the first / second Newton-Schulz polish step of the last split */
int tnml_svd_stats(tnml_ctx* ctx, int64_t* fallbacks, int64_t* cluster_repairs, double* dev_before_polish, double* dev_after_first_polish);
int64_t tnml_device_bytes(tnml_ctx* ctx);              /* device memory currently owned by ctx */

/* ---- workspace planning (host arithmetic + hipMemGetInfo; used by the drivers before tnml_create) ---------------
 * The reference treats `maxm` (fixedL.cc:592, default 5000) as an upper bound only; a context sizes its workspaces and
 * environment slabs by cfg.maxm, so a driver asks for the largest bond dimension that (a) an MPS of N sites can reach
 * and (b) fits the device, and says so, instead of failing in hipMalloc. */
int64_t tnml_estimate_bytes(const tnml_config* cfg);  /* device bytes of a context after a sweep has built every environment; -1 on bad cfg */
int tnml_device_memory(int device, int64_t* free_bytes, int64_t* total_bytes);
/* largest maxm in [floor_m, wanted] reachable by an N-site MPS whose tnml_estimate_bytes fits budget_bytes (<= 0: no memory bound) */
int tnml_plan_maxm(const tnml_config* cfg, int wanted, int floor_m, int64_t budget_bytes);

/* ---- the linear classifier (linear.cc) -------------------------------------------------------------------------
 * Ridge regression per label column by the reference's CG (linear.cc:27-90), K label columns at once over one shared
 * data set (kernels_linear.hip).  Features v_n = [1, x_n1/4, ..., x_nN/4], x = byte/255. (linear.cc:118-121,133-139,
 * mllib/mnist.h:495 -- the single normalisation); targets y_nk = +1 if label_n == L_k else -1 (:132).
 * Vectors cross the ABI as V[k][N+1] (bias first).  Same error convention as tnml_ctx: 0 on success, the message from
 * tnml_lin_last_error (NULL context: the last tnml_lin_create failure).  The context owns its device memory and stream. */
#define TNML_LIN_MAX_COLS 16
typedef struct tnml_lin tnml_lin;
/* a context for N-pixel images on HIP device `device`; fails without a usable device (no CPU fallback) */
int tnml_lin_create(tnml_lin** out, int device, int N);
int tnml_lin_destroy(tnml_lin* ctx);
const char* tnml_lin_last_error(const tnml_lin* ctx);
/* the data set (replaces the previous one; the CG must be started again): raw bytes pixels[NT][N] decoded as
   fl(b/255.)/4 (linear.cc:133-139, readMNIST's vector of train/test images, :111-112), or fp64 feature values
   features[NT][N] (the x/4 components, for reduced images and tests); labels[NT] */
int tnml_lin_set_data_u8(tnml_lin* ctx, int NT, const uint8_t* pixels, const int32_t* labels);
int tnml_lin_set_data_f64(tnml_lin* ctx, int NT, const double* features, const int32_t* labels);
/* the label column of each of the K (1..TNML_LIN_MAX_COLS) independent regressions: column k is `label = L_k` (:114, :132) */
int tnml_lin_set_labels(tnml_lin* ctx, int K, const int32_t* labels);
/* cgrad's preamble (:37-48): W = V[K][N+1], r = sum_n (y_n - W.v_n) v_n / NT - lambda W, p = r */
int tnml_lin_cg_start(tnml_lin* ctx, const double* V, double lambda);
/* npass more passes of the same CG (:51-89, no convergence exit); costs[npass][K] receives each pass's
   C = sum_n e_n^2 / NT + lambda W.W (:76).  Chunked calls continue the recursion: run(10) + run(20) == run(30) bitwise */
int tnml_lin_cg_run(tnml_lin* ctx, int npass, double* costs);
/* the current W as V[K][N+1] (:166, writeToFile(Vname,V) at :191) */
int tnml_lin_get_v(tnml_lin* ctx, double* V);
/* evaluate (:169-187) V[K][N+1] on the loaded data: ncorrect[k] = #(f y > 0), cnl[k] = sum (f - y)^2 / NT; leaves the CG state alone */
int tnml_lin_evaluate(tnml_lin* ctx, const double* V, int64_t* ncorrect, double* cnl);

#ifdef __cplusplus
}
#endif
#endif
