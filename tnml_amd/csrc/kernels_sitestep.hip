// kernels_sitestep.hip -- gradient steps on the device (tnml_site_step_u8 / tnml_site_step_phi): one optimiser step on W from the
// gradient that k_site_grad (kernels_sitegrad.hip) left in device memory.  The flat gradient g[0 .. E) is the sites concatenated as
// grad of tnml_site_gradient_* lays them out; the state arrays m and v have the same layout; the site tensors are separate
// allocations and are rewritten in place.  Three launches per step, whatever N and n are.
//
// The arithmetic -- the contract; tests/sitestep_model.py restates it in numpy and the GPU tests compare W bit for bit.  Every
// operation below is one IEEE fp64 rounding fl(.): the file is compiled with -ffp-contract=off like its neighbours, quotient and
// root are the correctly rounded forms (__ddiv_rn, __dsqrt_rn), there is no reciprocal or rsqrt approximation and no pow.
// Measured on the MI355X: no quotient and no root differed from numpy's in any test, Adam's results are numpy's bits as SGD's are.
//
// 1. total = sum of g^2 (class step_norm, k_step_norm then k_step_total).  g is cut into consecutive blocks of STEP_NORM_BLOCK = 65 536
//    elements, whatever site they fall in.  One workgroup of 256 threads per block: thread t starts from 0 and adds fl(g g) of the
//    block's elements t, t + 256, ... in ascending order; the 256 partial sums are joined by the fixed tree of k_eval_tally (stride
//    128, ..., 1: element t += element t + stride); the block sum goes to bsum[block].  k_step_total: one thread starts from 0 and adds
//    the block sums in block order.  No atomics: total is the same bits on every repeat.
// 2. The same thread forms grad_norm = fl(|scale| fl(sqrt(total))) and the factor f = scale, unless clip > 0 and grad_norm > clip:
//    then f = fl(scale fl(clip / grad_norm)) and clipped = 1.  applied = [total is finite].  All five go to res[SR_*].
//    gh = fl(f g) below.
// 3. k_site_step (class site_step), SGD:   v <- fl(fl(mu v) + gh);  A <- fl(A - fl(lr v))
// 4.                                Adam:  m <- fl(fl(beta1 m) + fl(o1 gh));  v <- fl(fl(beta2 v) + fl(fl(o2 gh) gh));
//                                          A <- fl(A - fl(lr fl(fl(m / c1) / fl(fl(sqrt(fl(v / c2))) + eps))))
//    with o1 = fl(1 - beta1), o2 = fl(1 - beta2), c1 = fl(1 - p1), c2 = fl(1 - p2) formed on the host, p1 <- fl(p1 beta1) and
//    p2 <- fl(p2 beta2) being the state's running powers (both start at 1).
// 5. k_site_step reads res[SR_APPLIED] first: when total is not finite it returns at once -- W, m and v stay bit for bit as they
//    were.  The host learns of it from res, which it reads after the stream is synchronised, and then leaves t, p1 and p2 alone too.
//
// The update is one pass over A, g and the state (about 7 E doubles of traffic for Adam), bound by memory bandwidth.  A workgroup
// owns STEP_WG_ELEMS = 4 096 consecutive elements of ONE site (a prefix table gives the first workgroup of every site, the site
// follows by binary search as in k_site_grad; 6 243 workgroups at N = 784, m = 120); its 256 threads walk them as 16-byte pairs,
// thread t taking pairs t, t + 256, ..., so that a wave reads and writes 1 KiB of consecutive addresses per access, four independent
// accesses per array in flight.  A site has an even element count (the site index s), the starts in g are even and the site tensors
// are allocations of their own: every pair is 16-byte aligned.
#include <hip/hip_runtime.h>

#include "tnml_internal.h"

#define STEP_THREADS 256
#define STEP_PAIRS (STEP_WG_ELEMS / 2)                    /* pairs per workgroup of the update */
static_assert(STEP_NORM_BLOCK % (STEP_THREADS * 8) == 0 && STEP_PAIRS % (STEP_THREADS * 4) == 0, "the unrolled walks cover a block exactly");

__global__ __launch_bounds__(STEP_THREADS) void k_step_norm(const double* __restrict__ g, size_t elems, double* __restrict__ bsum) {
    __shared__ double red[STEP_THREADS];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * STEP_NORM_BLOCK;
    const size_t end = elems - base < (size_t)STEP_NORM_BLOCK ? elems : base + STEP_NORM_BLOCK;
    double s = 0.;
    for (size_t i = base + t; i < end; i += STEP_THREADS * 8) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const size_t k = i + (size_t)STEP_THREADS * u; x[u] = k < end ? g[k] : 0.; }      // eight loads in flight
#pragma unroll
        for (int u = 0; u < 8; ++u) s += x[u] * x[u];                                                                   // in ascending order (+ 0 beyond the end changes nothing)
    }
    red[t] = s;
    __syncthreads();
    for (int stride = STEP_THREADS / 2; stride > 0; stride >>= 1) {
        if (t < stride) red[t] += red[t + stride];
        __syncthreads();
    }
    if (t == 0) bsum[blockIdx.x] = red[0];
}

// one workgroup: the block sums pass through LDS, thread 0 adds them in block order and leaves res[SR_*]
__global__ __launch_bounds__(STEP_THREADS) void k_step_total(const double* __restrict__ bsum, int nblk, double scale, double clip, double* __restrict__ res) {
    __shared__ double sh[STEP_THREADS];
    const int t = threadIdx.x;
    double total = 0.;
    for (int b0 = 0; b0 < nblk; b0 += STEP_THREADS) {
        if (b0 + t < nblk) sh[t] = bsum[b0 + t];
        __syncthreads();
        if (t == 0) { const int cnt = nblk - b0 < STEP_THREADS ? nblk - b0 : STEP_THREADS; for (int k = 0; k < cnt; ++k) total += sh[k]; }
        __syncthreads();
    }
    if (t != 0) return;
    const double norm = fabs(scale) * __dsqrt_rn(total);
    double f = scale, clipped = 0.;
    if (clip > 0. && norm > clip) { f = scale * __ddiv_rn(clip, norm); clipped = 1.; }
    res[SR_TOTAL] = total; res[SR_NORM] = norm; res[SR_FACTOR] = f; res[SR_CLIPPED] = clipped;
    res[SR_APPLIED] = isfinite(total) ? 1. : 0.;
}

template <int METHOD>
__global__ __launch_bounds__(STEP_THREADS) void k_site_step(const SiteStepArgs a) {
    if (a.res[SR_APPLIED] == 0.) return;                               // the gradient is out of range: nothing is touched
    const double f = a.res[SR_FACTOR];
    const int t = threadIdx.x;
    // the site of this workgroup: the last j with wg0[j] <= blockIdx.x
    int lo = 0, hi = a.N;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.wg0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid; }
    const int j = lo;
    const long long g0 = a.goff[j];
    const size_t npairs = (size_t)(a.goff[j + 1] - g0) / 2;
    const size_t p0 = (size_t)((int)blockIdx.x - a.wg0[j]) * STEP_PAIRS;
    double2* const A = reinterpret_cast<double2*>(const_cast<double*>(a.sites[j].a));
    const double2* const G = reinterpret_cast<const double2*>(a.grad + g0);
    double2* const V = reinterpret_cast<double2*>(a.v + g0);
    double2* const M = METHOD == TNML_STEP_ADAM ? reinterpret_cast<double2*>(a.m + g0) : nullptr;
    const double lr = a.lr, mu = a.mu, b1 = a.beta1, b2 = a.beta2, o1 = a.o1, o2 = a.o2, c1 = a.c1, c2 = a.c2, eps = a.eps;
    auto one = [&](double& A_, double g, double& m, double& v) {
        const double gh = f * g;
        if (METHOD == TNML_STEP_SGD) {
            v = mu * v + gh;
            A_ = A_ - lr * v;
        } else {
            m = b1 * m + o1 * gh;
            v = b2 * v + (o2 * gh) * gh;
            A_ = A_ - lr * __ddiv_rn(__ddiv_rn(m, c1), __dsqrt_rn(__ddiv_rn(v, c2)) + eps);
        }
    };
    for (int round = 0; round < STEP_PAIRS / (STEP_THREADS * 4); ++round) {
        double2 xa[4], xg[4], xv[4], xm[4];
        size_t p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            p[u] = p0 + (size_t)STEP_THREADS * (4 * round + u) + t;
            if (p[u] < npairs) {
                xa[u] = A[p[u]]; xg[u] = G[p[u]]; xv[u] = V[p[u]];
                if (METHOD == TNML_STEP_ADAM) xm[u] = M[p[u]];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p[u] < npairs) {
                one(xa[u].x, xg[u].x, xm[u].x, xv[u].x);
                one(xa[u].y, xg[u].y, xm[u].y, xv[u].y);
                A[p[u]] = xa[u]; V[p[u]] = xv[u];
                if (METHOD == TNML_STEP_ADAM) M[p[u]] = xm[u];
            }
        }
    }
}

int launch_site_step(tnml_ctx* c, const SiteStepArgs& a, int nwg) {
    if (a.nblk < 1 || nwg < 1 || a.elems == 0 || a.nblk != (int)((a.elems + STEP_NORM_BLOCK - 1) / STEP_NORM_BLOCK)) return tnml_fail(c, "site step kernels: %d norm blocks, %d workgroups for %zu elements", a.nblk, nwg, a.elems);
    if (!a.v || (a.method == TNML_STEP_ADAM && !a.m) || (a.method != TNML_STEP_ADAM && a.method != TNML_STEP_SGD)) return tnml_fail(c, "site step kernels: no state for method %d", a.method);
    {
        ProfScope ps(c, KC_STEP_NORM);
        hipLaunchKernelGGL(k_step_norm, dim3(a.nblk), dim3(STEP_THREADS), 0, c->stream, a.grad, a.elems, a.bsum);
        HIPCK(c, hipGetLastError());
    }
    {
        ProfScope ps(c, KC_STEP_NORM);
        hipLaunchKernelGGL(k_step_total, dim3(1), dim3(STEP_THREADS), 0, c->stream, a.bsum, a.nblk, a.scale, a.clip, a.res);
        HIPCK(c, hipGetLastError());
    }
    ProfScope ps(c, KC_SITE_STEP);
    if (a.method == TNML_STEP_ADAM) hipLaunchKernelGGL(k_site_step<TNML_STEP_ADAM>, dim3(nwg), dim3(STEP_THREADS), 0, c->stream, a);
    else                            hipLaunchKernelGGL(k_site_step<TNML_STEP_SGD>, dim3(nwg), dim3(STEP_THREADS), 0, c->stream, a);
    HIPCK(c, hipGetLastError());
    return 0;
}
