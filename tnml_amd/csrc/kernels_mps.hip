// kernels_mps.hip -- MPS algebra outside the sweep: the block placement of a direct sum (tnml_mps_place) and the
// transfer step of overlap(W,W) (tnml_mps_overlap).  sum(ipsis,{"Cutoff",1E-10}) and overlap(W,W) of fixedL.cc:697,729.
//
// Both are O(m^2) / O(m^3) items that run once per start, not roofline items: plain fp64 FMA kernels with a fixed
// summation order (the same bits on every run).
#include "tnml_internal.h"

// ---- direct sum: one block into a zeroed site tensor ------------------------------------------------------------
// dst[(row0 + a) + ML (s + 2 ((col0 + r) + MR slot))] += src[a + ml (s + 2 r)]; the launcher has checked that the block lies inside
__global__ void k_mps_place(const double* __restrict__ src, int ml, int mr, double* __restrict__ dst, int ML, int MR, int row0, int col0, int slot) {
    const size_t total = (size_t)ml * 2 * mr;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        size_t r_ = idx;
        const int a = (int)(r_ % ml); r_ /= ml;
        const int s = (int)(r_ % 2); r_ /= 2;
        const int r = (int)r_;
        dst[(size_t)(row0 + a) + (size_t)ML * (s + 2 * ((size_t)(col0 + r) + (size_t)MR * slot))] += src[idx];
    }
}
int launch_mps_place(tnml_ctx* c, const double* src, int ml, int mr, double* dst, int ML, int MR, int row0, int col0, int slot) {
    ProfScope ps(c, KC_PACK);
    if (row0 < 0 || col0 < 0 || ml < 1 || mr < 1 || row0 + ml > ML || col0 + mr > MR || slot < 0 || slot >= TNML_NL)
        return tnml_fail(c, "mps_place: block [%d,%d) x [%d,%d) leaves the %d x %d site", row0, row0 + ml, col0, col0 + mr, ML, MR);
    const size_t total = (size_t)ml * 2 * mr;
    size_t nb = (total + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(k_mps_place, dim3((unsigned)nb), dim3(256), 0, c->stream, src, ml, mr, dst, ML, MR, row0, col0, slot);
    HIPCK(c, hipGetLastError());
    return 0;
}

// ---- transfer step: Eout[r][r'] = sum_l sum_k A[k][r][l] T[k][r'][l] -------------------------------------------------
// A and T are [K][mr][L] (first index fastest; K = 2 ml runs over the left link and the site index).  64 x 64 output tile per
// workgroup, 4 x 4 outputs per thread, the two operands staged through LDS in slices of TK rows; the sum over the Label slots
// runs inside the kernel, so one launch serves the Label site too.
#define TT 64
#define TK 16
__global__ __launch_bounds__(256) void k_mps_transfer(const double* __restrict__ A, const double* __restrict__ T, int K, int mr, int L, double* __restrict__ Eout) {
    __shared__ double sA[TK][TT + 1];
    __shared__ double sT[TK][TT + 1];
    const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    const int r0 = blockIdx.x * TT, q0 = blockIdx.y * TT;
    const int lk = tid % TK, lc = tid / TK;               // this thread stages rows lk of columns lc, lc + 16, lc + 32, lc + 48
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.;
    for (int l = 0; l < L; ++l) {
        const double* Al = A + (size_t)K * mr * l;
        const double* Tl = T + (size_t)K * mr * l;
        for (int k0 = 0; k0 < K; k0 += TK) {
            const int k = k0 + lk;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = lc + 16 * i;
                const int ra = r0 + col, rt = q0 + col;
                sA[lk][col] = (k < K && ra < mr) ? Al[(size_t)k + (size_t)K * ra] : 0.;
                sT[lk][col] = (k < K && rt < mr) ? Tl[(size_t)k + (size_t)K * rt] : 0.;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < TK; ++kk) {
                double a[4], t[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { a[i] = sA[kk][tx + 16 * i]; t[i] = sT[kk][ty + 16 * i]; }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], t[j], acc[i][j]);
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = r0 + tx + 16 * i, q = q0 + ty + 16 * j;
            if (r < mr && q < mr) Eout[(size_t)r + (size_t)mr * q] = acc[i][j];
        }
}
int launch_mps_transfer(tnml_ctx* c, const double* A, const double* T, int K, int mr, int L, double* Eout) {
    ProfScope ps(c, KC_SMALLGEMM);
    if (K < 1 || mr < 1 || L < 1) return tnml_fail(c, "mps_transfer: bad shape %d x %d x %d", K, mr, L);
    const unsigned g = (unsigned)((mr + TT - 1) / TT);
    hipLaunchKernelGGL(k_mps_transfer, dim3(g, g), dim3(256), 0, c->stream, A, T, K, mr, L, Eout);
    HIPCK(c, hipGetLastError());
    return 0;
}
