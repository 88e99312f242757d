// kernels_linear.hip -- the `linear` driver's hot path: batched ridge-regression CG (linear.cc:27-90) for K label columns that share one
// data set, plus the evaluation of linear.cc:169-187, behind the tnml_lin_* entry points of include/tnml.h.
//
// Problem (per label column k, linear.cc:118-139): v_n = [1, x_n1/4, ..., x_nN/4] with x = byte/255. (mllib/mnist.h:495, the single
// normalisation), y_nk = +1 if label_n == L_k else -1, model f = W_k . v_n.  The design matrix is stored image-fastest, X[j][n] (j = 1..N,
// the layout of the rest of the library), as raw bytes (47 MB at 60 000 x 784) or as fp64 features; the constant feature 1 is implicit
// (row 0, 1 for real images and 0 for padding), and bytes are decoded through a 256-entry table fl(b/255.)/4 -- the reference's value exactly.
//
// One CG pass (linear.cc:51-89) is five launches on the context's stream, no host synchronisation:
//   k_lin_fwd    stream A: [f, q] = X^T [W, p] as one GEMM over the features (v_mfma_f64_16x16x4f64), f = W.v_n and q = p.v_n per image
//                into FQ, and per 256-image chunk the partials of sum_n q_n^2 (pAp)
//   k_lin_alpha  a_k = r.r / (sum q^2 / NT + lambda W.W)       (linear.cc:51-61; W.W of the OLD W, the reference's quirk, see below)
//   k_lin_bwd    stream B: e_nk = y_nk - (f_nk + a_k q_nk) once per workgroup into LDS (= y - W_new.v_n, linear.cc:66), per 1024-image chunk the partials of
//                sum e^2 and of nr = X e (sum over images of outer products, the shape of the gradient GEMM of kernels_grad.hip)
//   k_lin_reduce W += a p (linear.cc:62), nr = sum_chunks / NT - lambda W (:70-73), partial dot products nr.nr and W.W per 16 features
//   k_lin_p      beta = nr.nr / r.r, r = nr, p = r + beta p (:74-89), the pass's cost C = sum e^2 / NT + lambda W.W (:76) into costs[pass][k]
// Form chosen: the two-stream form.  f is recomputed from the current W at the top of every pass (stream A), so nothing is carried across
// passes as a recurrence; within the pass W_new.v = f + a q is exact algebra and saves a third stream over X.
//
// The reference quirk mirrored literally: pAp = sum_n (p.v_n)^2 / NT + lambda W.W -- W.W, not p.p (linear.cc:58).
//
// Determinism: no atomics.  Every reduction is per fixed-size chunk of images (256 for stream A, 1024 for stream B -- sizes that do not
// depend on the grid), then a fixed-order sum over the chunks, so a run is bitwise repeatable and run(10) + run(20) == run(30).  Every column
// goes through the same arithmetic whatever K is (the MFMA result of one output element does not depend on the other columns), so column L of
// a K = 10 run is bitwise the K = 1 run of label L; K = 1 therefore takes the same matrix-pipe path (a padded 16-column tile) instead of a
// VALU GEMV pair.
//
// MFMA fragment maps (tools/probe/probe64.hip, as kernels_gemm.hip / kernels_grad.hip): lane l = 16 g + i holds A[i][g], B[g][i], and
// C[g + 4 e][i] in accumulator element e.  Both streams PERMUTE the images inside a tile (any fixed permutation of a sum over images is as good
// as another) so that a lane's four images are consecutive: one 4-byte load of pixels (or 32 bytes of fp64 features) feeds four MFMAs.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <string>
#include <vector>

#include "tnml_internal.h"

typedef double f64x4l __attribute__((ext_vector_type(4)));

#define LIN_CA 256          // images per stream-A chunk (one workgroup)
#define LIN_CB 1024         // images per stream-B chunk (one workgroup row)
#define LIN_KC 16           // label columns per tile (K <= 16)

struct LinData {
    const uint8_t* X8; const double* XD;   // [N][NTp] (one of them)
    const double* tab;                     // [256] fl(b/255.)/4
    const int32_t* labels;                 // [NTp], -1 beyond NT
    int N, NT, NTp, Dp;                    // Dp: features incl. the constant one, padded to 16
};
struct LinCols { int K, KO; int lab[LIN_KC]; };   // KO: column of p_0 in the [W | p] operand (8 for K <= 8, else 16)

// four consecutive images n..n+3 of feature row `row` (0 = the constant feature, 1..N = pixels, beyond: padding)
template <typename T>
__device__ __forceinline__ void lin_ld4(const LinData& A, const double* tab, int row, int n, double x[4]) {
    if (row == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = (n + t < A.NT) ? 1. : 0.;
    } else if (row <= A.N) {
        if constexpr (sizeof(T) == 1) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(A.X8 + (size_t)(row - 1) * A.NTp + n);
#pragma unroll
            for (int t = 0; t < 4; ++t) x[t] = tab[(v >> (8 * t)) & 255u];
        } else {
            const double2* p = reinterpret_cast<const double2*>(A.XD + (size_t)(row - 1) * A.NTp + n);
            const double2 u = p[0], w = p[1];
            x[0] = u.x; x[1] = u.y; x[2] = w.x; x[3] = w.y;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = 0.;
    }
}

template <typename T>
__device__ __forceinline__ void lin_tab_load(const LinData& A, double* tab) {
    if constexpr (sizeof(T) == 1) { tab[threadIdx.x] = A.tab[threadIdx.x]; }
    __syncthreads();
}

// ---- stream A: FQ[c][n] = sum_j B[j][c] v_n[j] for c < 16 NCT; part[chunk][k] = sum over the chunk of FQ[KO + k][n]^2 -------------------
// 256 threads = 4 waves, a wave owns 64 images as 4 row tiles: tile r, row i <-> image nb + 4 i + r
template <typename T, int NCT>
__global__ __launch_bounds__(256) void k_lin_fwd(LinData A, const double* __restrict__ B /* [Dp][32] */, double* __restrict__ FQ /* [32][NTp] */,
                                                 double* __restrict__ part /* [NTp/256][16] or null */, int KO) {
    __shared__ double tab[256];
    __shared__ double red[4][4][32];
    lin_tab_load<T>(A, tab);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, i = l & 15, g = l >> 4;
    const int nb = blockIdx.x * LIN_CA + 64 * w;
    f64x4l acc[4][NCT];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[r][ct] = f64x4l{0., 0., 0., 0.};
    for (int k0 = 0; k0 < A.Dp; k0 += 4) {
        const int row = k0 + g;
        double x[4];
        lin_ld4<T>(A, tab, row, nb + 4 * i, x);
        double b[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) b[ct] = B[(size_t)row * 32 + 16 * ct + i];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[r][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[r], b[ct], acc[r][ct], 0, 0, 0);
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        double* o = FQ + (size_t)(16 * ct + i) * A.NTp + nb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double2* d = reinterpret_cast<double2*>(o + 4 * (g + 4 * e));
            d[0] = double2{acc[0][ct][e], acc[1][ct][e]};
            d[1] = double2{acc[2][ct][e], acc[3][ct][e]};
        }
    }
    if (!part) return;                           // (uniform over the grid)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        double s = 0.;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) s += acc[r][ct][e] * acc[r][ct][e];
        red[w][g][16 * ct + i] = s;
    }
    __syncthreads();
    if (threadIdx.x < LIN_KC) {
        const int col = KO + threadIdx.x;
        double tot = 0.;
        if (col < 16 * NCT)
            for (int ww = 0; ww < 4; ++ww)
                for (int gg = 0; gg < 4; ++gg) tot += red[ww][gg][col];
        part[(size_t)blockIdx.x * LIN_KC + threadIdx.x] = tot;
    }
}

// ---- a_k = r.r / pAp, pAp = sum q^2 / NT + lambda W.W (linear.cc:51-61); one workgroup ----------------------------------------------------
__global__ __launch_bounds__(256) void k_lin_alpha(const double* __restrict__ part, int nch, LinCols C, int NT, double lambda,
                                                   const double* __restrict__ rr, const double* __restrict__ ww, double* __restrict__ a, int start) {
    __shared__ double red[16][LIN_KC];
    const int c = threadIdx.x & 15, s = threadIdx.x >> 4;
    double t = 0.;
#pragma unroll 4
    for (int ch = s; ch < nch; ch += 16) t += part[(size_t)ch * LIN_KC + c];
    red[s][c] = t;
    __syncthreads();
    if (threadIdx.x < LIN_KC) {
        double tot = 0.;
        for (int k = 0; k < 16; ++k) tot += red[k][c];
        double pAp = tot / NT;
        pAp += lambda * ww[c];                 // :58 lambda*(W*W), sic
        a[c] = (start || c >= C.K) ? 0. : rr[c] / pAp;
    }
}

// ---- stream B: e = y - (f + a q) per image and column, partials of sum e^2 and of nr = X e per 1024-image chunk ----------------------------
// grid (NTp/1024, ceil(Dp/16 / 16)); wave w of row y owns feature tiles 16 y + 4 w + tt; k-step t of a 16-image block: lane (i, g) <-> image nb + 4 g + t.
// The residuals are formed ONCE per workgroup: per 64-image step every thread computes four of them (column c = tid & 15, images 4 (tid >> 4)
// .. + 3) into LDS, and the four waves read their fragments from there; sum e^2 is taken by row 0 only.
#define LIN_ES 64                      // images per staging step
#define LIN_ER 17                      // doubles between staged images (16 columns + 1: fragment reads of the four lane groups on different banks)
template <typename T>
__global__ __launch_bounds__(256) void k_lin_bwd(LinData A, LinCols C, const double* __restrict__ FQ, const double* __restrict__ a,
                                                 double* __restrict__ nrpart /* [NTp/1024][Dp][16] */, double* __restrict__ cpart /* [NTp/1024][16] */) {
    __shared__ double tab[256];
    __shared__ double es[2][LIN_ES * LIN_ER];
    __shared__ double red[16][LIN_KC];
    lin_tab_load<T>(A, tab);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, i = l & 15, g = l >> 4;
    const int ch = blockIdx.x, n0 = ch * LIN_CB, ntile = A.Dp / 16;
    // the residual share of this thread: column sc, images 4 sq .. 4 sq + 3 of every staging step
    const int sc = threadIdx.x & 15, sq = threadIdx.x >> 4;
    const bool live = sc < C.K, cost_row = blockIdx.y == 0;
    const double as = live ? a[sc] : 0.;
    const int lab = live ? C.lab[sc] : -2;
    const double* fcol = FQ + (size_t)(live ? sc : 0) * A.NTp;
    const double* qcol = FQ + (size_t)(live ? C.KO + sc : 0) * A.NTp;
    int tI[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) tI[tt] = 16 * blockIdx.y + 4 * w + tt;
    f64x4l acc[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) acc[tt] = f64x4l{0., 0., 0., 0.};
    double c2 = 0.;
    for (int ns = n0, buf = 0; ns < n0 + LIN_CB; ns += LIN_ES, buf ^= 1) {
        // (a thread writes buffer buf only after every thread has passed the barrier of the previous step, i.e. has finished reading
        //  the buffer it read two steps ago)
        double* eb = es[buf];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = ns + 4 * sq + t;
            double e = 0.;
            if (live && n < A.NT) {
                const double y = A.labels[n] == lab ? 1. : -1.;
                e = y - (fcol[n] + as * qcol[n]);                             // :66 y - W.v with W = W + a p
            }
            if (cost_row) c2 += e * e;
            eb[(4 * sq + t) * LIN_ER + sc] = e;
        }
        __syncthreads();
#pragma unroll 2
        for (int s = 0; s < LIN_ES / 16; ++s) {
            const int n = ns + 16 * s + 4 * g;
            double e[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) e[t] = eb[(16 * s + 4 * g + t) * LIN_ER + i];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                if (tI[tt] >= ntile) continue;                               // (uniform over the wave)
                double x[4];
                lin_ld4<T>(A, tab, 16 * tI[tt] + i, n, x);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[t], e[t], acc[tt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
        if (tI[tt] >= ntile) continue;
        double* o = nrpart + ((size_t)ch * A.Dp + 16 * tI[tt]) * LIN_KC + i;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[(size_t)(g + 4 * e) * LIN_KC] = acc[tt][e];
    }
    if (!cost_row) return;                                                   // (uniform over the workgroup)
    red[sq][sc] = c2;
    __syncthreads();
    if (threadIdx.x < LIN_KC) {
        double t = 0.;
        for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
        cpart[(size_t)ch * LIN_KC + threadIdx.x] = t;
    }
}

// ---- W += a p, nr = sum_chunks nrpart / NT - lambda W; partials of nr.nr and W.W per 16 features (grid Dp/16) ------------------------------
__global__ __launch_bounds__(256) void k_lin_reduce(double* __restrict__ WP, double* __restrict__ R, const double* __restrict__ nrpart, int nch,
                                                    const double* __restrict__ a, LinCols C, int Dp, int NT, double lambda, double* __restrict__ bpart) {
    __shared__ double red[16][LIN_KC][2];
    const int c = threadIdx.x & 15, jr = threadIdx.x >> 4, j = 16 * blockIdx.x + jr;
    double s = 0.;
#pragma unroll 8
    for (int ch = 0; ch < nch; ++ch) s += nrpart[((size_t)ch * Dp + j) * LIN_KC + c];     // (unrolled: the loads go out together, the sum keeps its order)
    double wn = 0., nr = 0.;
    if (c < C.K) {
        wn = WP[(size_t)j * 32 + c] + a[c] * WP[(size_t)j * 32 + C.KO + c];   // :62 W = W + a*p
        nr = s / NT;                                                          // :70
        if (lambda != 0.) nr = nr - lambda * wn;                              // :72
        WP[(size_t)j * 32 + c] = wn;
        R[(size_t)j * LIN_KC + c] = nr;
    }
    red[jr][c][0] = nr * nr;
    red[jr][c][1] = wn * wn;
    __syncthreads();
    if (threadIdx.x < LIN_KC) {
        double t0 = 0., t1 = 0.;
        for (int k = 0; k < 16; ++k) { t0 += red[k][c][0]; t1 += red[k][c][1]; }
        bpart[((size_t)blockIdx.x * LIN_KC + c) * 2 + 0] = t0;
        bpart[((size_t)blockIdx.x * LIN_KC + c) * 2 + 1] = t1;
    }
}

// ---- beta = nr.nr / r.r, p = r + beta p (start: p = r); block 0 records r.r, W.W and the pass's cost (linear.cc:74-89) ---------------------
__global__ __launch_bounds__(256) void k_lin_p(double* __restrict__ WP, const double* __restrict__ R, const double* __restrict__ bpart, int nblk,
                                               LinCols C, const double* __restrict__ rr_rd, double* __restrict__ rr_wr, double* __restrict__ ww_wr,
                                               const double* __restrict__ cpart, int nchB, int NT, double lambda, double* __restrict__ cost_row, int start) {
    const int c = threadIdx.x & 15, j = 16 * blockIdx.x + (threadIdx.x >> 4);
    double nn = 0.;
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) nn += bpart[((size_t)b * LIN_KC + c) * 2];
    if (c < C.K) {
        const double r = R[(size_t)j * LIN_KC + c];
        if (start) WP[(size_t)j * 32 + C.KO + c] = r;                          // :48 p = r
        else {
            const double beta = nn / rr_rd[c];                                 // :74
            WP[(size_t)j * 32 + C.KO + c] = r + beta * WP[(size_t)j * 32 + C.KO + c];   // :87
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < LIN_KC) {
        double ww = 0.;
#pragma unroll 8
        for (int b = 0; b < nblk; ++b) ww += bpart[((size_t)b * LIN_KC + c) * 2 + 1];
        rr_wr[c] = nn;
        ww_wr[c] = ww;
        if (!start && c < C.K) {
            double cs = 0.;
#pragma unroll 8
            for (int ch = 0; ch < nchB; ++ch) cs += cpart[(size_t)ch * LIN_KC + c];
            double Cc = cs / NT;                                               // :69
            Cc += lambda * ww;                                                 // :76
            cost_row[c] = Cc;
        }
    }
}

// ---- evaluation (linear.cc:169-187): per 256-image chunk, #(f y > 0) and sum (f - y)^2 per column ----------------------------------------
__global__ __launch_bounds__(256) void k_lin_eval(LinData A, LinCols C, const double* __restrict__ FQ, double* __restrict__ cnl, int* __restrict__ cnt) {
    __shared__ double rd[256];
    __shared__ int ri[256];
    const int n = blockIdx.x * LIN_CA + threadIdx.x;
    for (int c = 0; c < C.K; ++c) {
        double d2 = 0.; int ok = 0;
        if (n < A.NT) {
            const double f = FQ[(size_t)c * A.NTp + n], y = A.labels[n] == C.lab[c] ? 1. : -1.;
            ok = f * y > 0. ? 1 : 0;
            d2 = (f - y) * (f - y);
        }
        rd[threadIdx.x] = d2; ri[threadIdx.x] = ok;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) { rd[threadIdx.x] += rd[threadIdx.x + h]; ri[threadIdx.x] += ri[threadIdx.x + h]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) { cnl[(size_t)blockIdx.x * LIN_KC + c] = rd[0]; cnt[(size_t)blockIdx.x * LIN_KC + c] = ri[0]; }
        __syncthreads();
    }
}

// =========================================================================================================================================
// C-ABI (include/tnml.h, tnml_lin_*)
// =========================================================================================================================================
struct tnml_lin {
    int device = 0, N = 0, Dp = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // data
    int NT = 0, NTp = 0; bool u8 = true;
    uint8_t* X8 = nullptr; double* XD = nullptr; int32_t* labels = nullptr; double* tab = nullptr;
    // columns and CG state
    LinCols cols{};
    bool started = false; long pass = 0; double lambda = 0.;
    double *WP = nullptr, *EV = nullptr, *R = nullptr, *scal = nullptr;   // scal: a[16], rr[2][16], ww[2][16]
    double *FQ = nullptr, *apart = nullptr, *nrpart = nullptr, *cpart = nullptr, *bpart = nullptr, *evd = nullptr;
    int* evi = nullptr;
    double* costs = nullptr; int cost_cap = 0;
};

static std::string g_lin_create_err;
static int lin_fail(tnml_lin* c, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) c->err = buf; else g_lin_create_err = buf;
    return 1;
}
#define LCK(c, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return lin_fail((c), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

template <typename P> static void lin_free(P*& p) { if (p) (void)hipFree(p); p = nullptr; }
static void lin_free_data(tnml_lin* c) {
    lin_free(c->X8); lin_free(c->XD); lin_free(c->labels); lin_free(c->FQ); lin_free(c->apart); lin_free(c->nrpart); lin_free(c->cpart);
    lin_free(c->evd); lin_free(c->evi);
    c->NT = c->NTp = 0; c->started = false;
}
static LinData lin_data(const tnml_lin* c) {
    LinData d; d.X8 = c->X8; d.XD = c->XD; d.tab = c->tab; d.labels = c->labels; d.N = c->N; d.NT = c->NT; d.NTp = c->NTp; d.Dp = c->Dp; return d;
}

extern "C" {

const char* tnml_lin_last_error(const tnml_lin* c) { return c ? c->err.c_str() : g_lin_create_err.c_str(); }

int tnml_lin_create(tnml_lin** out, int device, int N) {
    if (!out) return lin_fail(nullptr, "tnml_lin_create: out is NULL");
    *out = nullptr;
    if (N < 1) return lin_fail(nullptr, "tnml_lin_create: N = %d (need >= 1)", N);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return lin_fail(nullptr, "tnml_lin_create: no HIP device available (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return lin_fail(nullptr, "tnml_lin_create: device %d out of range (%d visible)", device, ndev);
    if (hipSetDevice(device) != hipSuccess) return lin_fail(nullptr, "tnml_lin_create: hipSetDevice failed");
    tnml_lin* c = new tnml_lin;
    c->device = device; c->N = N; c->Dp = (N + 1 + 15) / 16 * 16;
    auto bail = [&](const char* what) { g_lin_create_err = std::string("tnml_lin_create: ") + what; tnml_lin_destroy(c); return 1; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail("hipStreamCreate failed");
    const size_t wpb = sizeof(double) * (size_t)c->Dp * 32, rb = sizeof(double) * (size_t)c->Dp * LIN_KC, bb = sizeof(double) * (size_t)c->Dp * 2;
    if (hipMalloc(&c->WP, wpb) != hipSuccess || hipMalloc(&c->EV, wpb) != hipSuccess || hipMalloc(&c->R, rb) != hipSuccess ||
        hipMalloc(&c->scal, sizeof(double) * 5 * LIN_KC) != hipSuccess || hipMalloc(&c->bpart, bb) != hipSuccess ||
        hipMalloc(&c->tab, sizeof(double) * 256) != hipSuccess)
        return bail("hipMalloc failed");
    double tab[256];
    for (int b = 0; b < 256; ++b) tab[b] = ((double)b / 255.) / 4.;            // mllib/mnist.h:495, linear.cc:133-139
    if (hipMemcpy(c->tab, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) return bail("hipMemcpy failed");
    if (hipMemset(c->WP, 0, wpb) != hipSuccess || hipMemset(c->R, 0, rb) != hipSuccess || hipMemset(c->scal, 0, sizeof(double) * 5 * LIN_KC) != hipSuccess)
        return bail("hipMemset failed");
    c->cols.K = 0;
    *out = c;
    return 0;
}

int tnml_lin_destroy(tnml_lin* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    lin_free_data(c);
    lin_free(c->WP); lin_free(c->EV); lin_free(c->R); lin_free(c->scal); lin_free(c->bpart); lin_free(c->tab); lin_free(c->costs);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

static int lin_set_data(tnml_lin* c, int NT, const uint8_t* px, const double* ft, const int32_t* labels) {
    if (!c) return lin_fail(nullptr, "tnml_lin_set_data: ctx is NULL");
    if (NT < 1 || (!px && !ft) || !labels) return lin_fail(c, "tnml_lin_set_data: need NT >= 1, the data and the labels");
    LCK(c, hipSetDevice(c->device));
    LCK(c, hipStreamSynchronize(c->stream));
    lin_free_data(c);
    const int N = c->N, NTp = (NT + LIN_CB - 1) / LIN_CB * LIN_CB;
    c->NT = NT; c->NTp = NTp; c->u8 = px != nullptr;
    // image-fastest layout X[j][n], zero padding
    if (c->u8) {
        std::vector<uint8_t> h((size_t)N * NTp, 0);
        for (int n = 0; n < NT; ++n) for (int j = 0; j < N; ++j) h[(size_t)j * NTp + n] = px[(size_t)n * N + j];
        LCK(c, hipMalloc(&c->X8, h.size()));
        LCK(c, hipMemcpy(c->X8, h.data(), h.size(), hipMemcpyHostToDevice));
    } else {
        std::vector<double> h((size_t)N * NTp, 0.);
        for (int n = 0; n < NT; ++n) for (int j = 0; j < N; ++j) h[(size_t)j * NTp + n] = ft[(size_t)n * N + j];
        LCK(c, hipMalloc(&c->XD, h.size() * sizeof(double)));
        LCK(c, hipMemcpy(c->XD, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    std::vector<int32_t> lab(NTp, -1);
    std::copy(labels, labels + NT, lab.begin());
    LCK(c, hipMalloc(&c->labels, sizeof(int32_t) * NTp));
    LCK(c, hipMemcpy(c->labels, lab.data(), sizeof(int32_t) * NTp, hipMemcpyHostToDevice));
    LCK(c, hipMalloc(&c->FQ, sizeof(double) * 32 * (size_t)NTp));
    LCK(c, hipMemset(c->FQ, 0, sizeof(double) * 32 * (size_t)NTp));
    LCK(c, hipMalloc(&c->apart, sizeof(double) * LIN_KC * (size_t)(NTp / LIN_CA)));
    LCK(c, hipMalloc(&c->nrpart, sizeof(double) * LIN_KC * (size_t)c->Dp * (NTp / LIN_CB)));
    LCK(c, hipMalloc(&c->cpart, sizeof(double) * LIN_KC * (size_t)(NTp / LIN_CB)));
    LCK(c, hipMalloc(&c->evd, sizeof(double) * LIN_KC * (size_t)(NTp / LIN_CA)));
    LCK(c, hipMalloc(&c->evi, sizeof(int) * LIN_KC * (size_t)(NTp / LIN_CA)));
    return 0;
}
int tnml_lin_set_data_u8(tnml_lin* c, int NT, const uint8_t* pixels, const int32_t* labels) {
    if (!pixels) return lin_fail(c, "tnml_lin_set_data_u8: pixels is NULL");
    return lin_set_data(c, NT, pixels, nullptr, labels);
}
int tnml_lin_set_data_f64(tnml_lin* c, int NT, const double* features, const int32_t* labels) {
    if (!features) return lin_fail(c, "tnml_lin_set_data_f64: features is NULL");
    return lin_set_data(c, NT, nullptr, features, labels);
}

int tnml_lin_set_labels(tnml_lin* c, int K, const int32_t* labels) {
    if (!c) return lin_fail(nullptr, "tnml_lin_set_labels: ctx is NULL");
    if (K < 1 || K > TNML_LIN_MAX_COLS || !labels) return lin_fail(c, "tnml_lin_set_labels: K = %d (need 1..%d)", K, TNML_LIN_MAX_COLS);
    c->cols = LinCols{};
    c->cols.K = K; c->cols.KO = K <= 8 ? 8 : 16;
    for (int k = 0; k < LIN_KC; ++k) c->cols.lab[k] = k < K ? labels[k] : -2;
    c->started = false;
    return 0;
}

// one pass of the CG (or, start != 0, the initial residual and p = r): five launches, no host synchronisation
static int lin_pass(tnml_lin* c, long pass, int start, double* cost_row) {
    const LinData d = lin_data(c);
    const LinCols C = c->cols;
    const int nchA = c->NTp / LIN_CA, nchB = c->NTp / LIN_CB, nt = c->Dp / 16;
    const int rd = start ? 0 : (int)(pass & 1), wr = start ? 0 : rd ^ 1;
    double* a = c->scal; double* rr = c->scal + LIN_KC; double* ww = c->scal + 3 * LIN_KC;
    const dim3 gA(nchA), gB(nchB, (nt + 15) / 16), gR(nt), blk(256);
    if (c->u8) {
        if (C.KO == 8) k_lin_fwd<uint8_t, 1><<<gA, blk, 0, c->stream>>>(d, c->WP, c->FQ, c->apart, C.KO);
        else           k_lin_fwd<uint8_t, 2><<<gA, blk, 0, c->stream>>>(d, c->WP, c->FQ, c->apart, C.KO);
    } else {
        if (C.KO == 8) k_lin_fwd<double, 1><<<gA, blk, 0, c->stream>>>(d, c->WP, c->FQ, c->apart, C.KO);
        else           k_lin_fwd<double, 2><<<gA, blk, 0, c->stream>>>(d, c->WP, c->FQ, c->apart, C.KO);
    }
    k_lin_alpha<<<1, blk, 0, c->stream>>>(c->apart, nchA, C, c->NT, c->lambda, rr + LIN_KC * rd, ww + LIN_KC * rd, a, start);
    if (c->u8) k_lin_bwd<uint8_t><<<gB, blk, 0, c->stream>>>(d, C, c->FQ, a, c->nrpart, c->cpart);
    else       k_lin_bwd<double><<<gB, blk, 0, c->stream>>>(d, C, c->FQ, a, c->nrpart, c->cpart);
    k_lin_reduce<<<gR, blk, 0, c->stream>>>(c->WP, c->R, c->nrpart, nchB, a, C, c->Dp, c->NT, c->lambda, c->bpart);
    k_lin_p<<<gR, blk, 0, c->stream>>>(c->WP, c->R, c->bpart, nt, C, rr + LIN_KC * rd, rr + LIN_KC * wr, ww + LIN_KC * wr, c->cpart, nchB, c->NT,
                                       c->lambda, cost_row, start);
    LCK(c, hipGetLastError());
    return 0;
}

static int lin_ready(tnml_lin* c, const char* who) {
    if (!c) return lin_fail(nullptr, "%s: ctx is NULL", who);
    if (c->NT == 0) return lin_fail(c, "%s: no data set (tnml_lin_set_data_u8 / _f64)", who);
    if (c->cols.K == 0) return lin_fail(c, "%s: no label columns (tnml_lin_set_labels)", who);
    return 0;
}

int tnml_lin_cg_start(tnml_lin* c, const double* V, double lambda) {
    if (lin_ready(c, "tnml_lin_cg_start")) return 1;
    if (!V) return lin_fail(c, "tnml_lin_cg_start: V is NULL");
    LCK(c, hipSetDevice(c->device));
    const int D = c->N + 1, K = c->cols.K;
    std::vector<double> h((size_t)c->Dp * 32, 0.);                            // [W | p = 0]
    for (int k = 0; k < K; ++k) for (int j = 0; j < D; ++j) h[(size_t)j * 32 + k] = V[(size_t)k * D + j];
    LCK(c, hipMemcpyAsync(c->WP, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->lambda = lambda;
    if (lin_pass(c, 0, 1, nullptr)) return 1;                                 // linear.cc:37-48
    LCK(c, hipStreamSynchronize(c->stream));                                  // (h goes out of scope)
    c->started = true; c->pass = 0;
    return 0;
}

int tnml_lin_cg_run(tnml_lin* c, int npass, double* costs) {
    if (lin_ready(c, "tnml_lin_cg_run")) return 1;
    if (!c->started) return lin_fail(c, "tnml_lin_cg_run: tnml_lin_cg_start first");
    if (npass < 0) return lin_fail(c, "tnml_lin_cg_run: npass = %d", npass);
    if (npass == 0) return 0;
    LCK(c, hipSetDevice(c->device));
    const int K = c->cols.K;
    if (npass > c->cost_cap) {
        LCK(c, hipStreamSynchronize(c->stream));
        lin_free(c->costs);
        LCK(c, hipMalloc(&c->costs, sizeof(double) * LIN_KC * (size_t)npass));
        c->cost_cap = npass;
    }
    for (int i = 0; i < npass; ++i)
        if (lin_pass(c, c->pass + i, 0, c->costs + (size_t)i * K)) return 1;
    c->pass += npass;
    if (costs) LCK(c, hipMemcpyAsync(costs, c->costs, sizeof(double) * K * (size_t)npass, hipMemcpyDeviceToHost, c->stream));
    LCK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int tnml_lin_get_v(tnml_lin* c, double* V) {
    if (!c) return lin_fail(nullptr, "tnml_lin_get_v: ctx is NULL");
    if (!c->started) return lin_fail(c, "tnml_lin_get_v: tnml_lin_cg_start first");
    LCK(c, hipSetDevice(c->device));
    const int D = c->N + 1, K = c->cols.K;
    std::vector<double> h((size_t)c->Dp * 32);
    LCK(c, hipMemcpyAsync(h.data(), c->WP, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LCK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < K; ++k) for (int j = 0; j < D; ++j) V[(size_t)k * D + j] = h[(size_t)j * 32 + k];
    return 0;
}

int tnml_lin_evaluate(tnml_lin* c, const double* V, int64_t* ncorrect, double* cnl) {
    if (lin_ready(c, "tnml_lin_evaluate")) return 1;
    if (!V || !ncorrect || !cnl) return lin_fail(c, "tnml_lin_evaluate: NULL argument");
    LCK(c, hipSetDevice(c->device));
    const int D = c->N + 1, K = c->cols.K, nchA = c->NTp / LIN_CA;
    std::vector<double> h((size_t)c->Dp * 32, 0.);
    for (int k = 0; k < K; ++k) for (int j = 0; j < D; ++j) h[(size_t)j * 32 + k] = V[(size_t)k * D + j];
    LCK(c, hipMemcpyAsync(c->EV, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const LinData d = lin_data(c);
    if (c->u8) k_lin_fwd<uint8_t, 1><<<nchA, 256, 0, c->stream>>>(d, c->EV, c->FQ, nullptr, 8);
    else       k_lin_fwd<double, 1><<<nchA, 256, 0, c->stream>>>(d, c->EV, c->FQ, nullptr, 8);
    k_lin_eval<<<nchA, 256, 0, c->stream>>>(d, c->cols, c->FQ, c->evd, c->evi);
    LCK(c, hipGetLastError());
    std::vector<double> pd((size_t)nchA * LIN_KC);
    std::vector<int> pi((size_t)nchA * LIN_KC);
    LCK(c, hipMemcpyAsync(pd.data(), c->evd, pd.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LCK(c, hipMemcpyAsync(pi.data(), c->evi, pi.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LCK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < K; ++k) {
        double s = 0.; int64_t n = 0;
        for (int b = 0; b < nchA; ++b) { s += pd[(size_t)b * LIN_KC + k]; n += pi[(size_t)b * LIN_KC + k]; }
        ncorrect[k] = n;
        cnl[k] = s / c->NT;                                                   // :181
    }
    // (the CG state is untouched: FQ is recomputed at the top of every pass)
    return 0;
}

}  // extern "C"
