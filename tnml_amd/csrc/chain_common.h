// chain_common.h -- what the chain kernels share: k_chain (kernels_chain.hip, streamed inference), k_response (kernels_response.hip,
// streamed site responses) and k_site_backward / k_site_grad (kernels_sitegrad.hip, streamed site gradients).  The element-type traits ChainT<E>, the features of a site (chain_features), the A fragment of a 16-wide k block
// (chain_load_a) and one site of a chain (chain_step); the fragment maps, the k blocks and the arithmetic order are described in the header
// of kernels_chain.hip.
#pragma once
#include "tnml_internal.h"

#define CHAIN_THREADS 512
#define CHAIN_WAVES 8

// what differs between the element types, and nothing else
template <typename E> struct ChainT;
template <> struct ChainT<double> {
    typedef double v4 __attribute__((ext_vector_type(4)));
    typedef double v2 __attribute__((ext_vector_type(2)));
    // two tiles of ru16(maxbond) x T doubles <= 128 KiB: T = 64 up to bond T64, 32 up to T32, 16 up to MAXM
    static constexpr int T64 = 128, T32 = 256, MAXM = TNML_CHAIN_MAXM;
    static constexpr const char* what = "";             // in front of "chain kernel: ..." in every message
    static constexpr const char* elems = "doubles";
    // LDS swizzle: see the header (for T >= 32 the column index of odd rows is XORed with 16)
    template <int NCT>
    static __device__ __forceinline__ int idx(int k, int n) {
        return k * (16 * NCT) + (NCT > 1 ? (n ^ ((k & 1) << 4)) : n);
    }
    // C/D map of the fp64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg
    static __device__ __forceinline__ int row(int rt, int q, int r) { return rt * 16 + q + 4 * r; }
    static __device__ __forceinline__ v4 mfma(double a, double b, v4 acc) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0); }
    static __device__ __forceinline__ double fma(double a, double b, double c) { return ::fma(a, b, c); }
    static __device__ __forceinline__ double abs(double w) { return fabs(w); }
    static __device__ __forceinline__ bool bad(double) { return false; }
};
template <> struct ChainT<float> {
    typedef float v4 __attribute__((ext_vector_type(4)));
    typedef float v2 __attribute__((ext_vector_type(2)));
    // two tiles of ru16(maxbond) x T floats <= 128 KiB: T = 64 up to bond 256, 32 up to 512, 16 up to 1 024
    static constexpr int T64 = 256, T32 = 512, MAXM = TNML_CHAIN32_MAXM;
    static constexpr const char* what = "fp32 ";
    static constexpr const char* elems = "floats";
    // LDS swizzle.  ds_read_b32 / ds_write_b32 serve a wave in two groups of 32 lanes over 32 banks, so the two k rows (q = 0, 1 and
    // q = 2, 3) of a group, 16 floats each, must fall on different halves of the banks.  Those rows are 2 apart in the right chain
    // (row = base / 2 + 2 q + (i >> 1): the lower one has row mod 4 in {0, 1}) and 4 apart in the left chain, the centre and the C/D store
    // (row = 16 rt + 4 q + reg).  g(k) = bit 1 of k xor bit 2 of k differs across both kinds of pair; it is put into address bit 4 (in floats):
    //   T >= 32: column ^ (g(k) << 4), the row pitch being a multiple of 32 floats;
    //   T = 16:  the rows of every aligned group of 8 are permuted, row bits (b2 b1 b0) -> (b2, b0, b1 ^ b2), so that bit 0 of the stored
    //            row -- address bit 4 -- is g(k).
    // (a left-chain block that straddles kk = ml pairs rows 4 - ml apart: at most one block per site keeps a 2-way conflict.)
    template <int NCT>
    static __device__ __forceinline__ int idx(int k, int n) {
        const int g = ((k >> 1) ^ (k >> 2)) & 1;
        if (NCT > 1) return k * (16 * NCT) + (n ^ (g << 4));
        return ((k & ~3) | ((k & 1) << 1) | g) * 16 + n;
    }
    // C/D map of the f32 MFMA: column = lane & 15, row = 4 (lane >> 4) + reg -- not the fp64 form's (lane >> 4) + 4 reg
    static __device__ __forceinline__ int row(int rt, int q, int r) { return rt * 16 + 4 * q + r; }
    static __device__ __forceinline__ v4 mfma(float a, float b, v4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }
    static __device__ __forceinline__ float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
    static __device__ __forceinline__ float abs(float w) { return __builtin_fabsf(w); }
    static __device__ __forceinline__ bool bad(float wa) { return !(wa <= 3.402823466e+38f); }      // Inf or NaN
};

// features of site j (1-indexed) for the NCT columns of this lane: image tile0 + 16 ct + (lane & 15); images beyond cnt get (0, 0)
// SRC 0: bytes through the built-in expression (g.xT) or staged features (g.phiT), chosen at run time as before the input map existed;
// SRC 1: the input map -- one 2-byte block sum and one dependent table row per site and column (g.codeT, g.table; the table
// is at most 261 KB and stays in L2).  The source is a template parameter so that the SRC 0 instantiations carry nothing of it.
template <typename E, int NCT, int SRC>
static __device__ __forceinline__ void chain_features(const ChainArgs<E>& g, int j, int img0, E (&p0)[NCT], E (&p1)[NCT]) {
    typedef typename ChainT<E>::v2 v2;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int n = img0 + 16 * ct;
        E f0 = 0, f1 = 0;
        if (n < g.cnt) {
            if (SRC == 1) {
                const unsigned code = g.codeT[(size_t)(j - 1) * g.ld + n];
                const v2 f = *(const v2*)(g.table + (size_t)2 * code);
                f0 = f.x; f1 = f.y;
            } else if (g.xT) {                         // the expression of k_features_u8<double> (kernels_stream.hip), formed in fp64, rounded once
                const double gq = (double)g.xT[(size_t)(j - 1) * g.ld + n] / 255.;
                f0 = 1;
                f1 = (E)((gq / 255.) / 4.);
            } else {
                f0 = g.phiT[((size_t)(j - 1) * 2 + 0) * g.ld + n];
                f1 = g.phiT[((size_t)(j - 1) * 2 + 1) * g.ld + n];
            }
        }
        p0[ct] = f0; p1[ct] = f1;
    }
}

// the four values kk = base + 4 q + i of output row `orow` (see the header); masked outside the tensor
template <typename E, bool LEFT>
static __device__ __forceinline__ void chain_load_a(const E* __restrict__ A, int ml, int M, int K, int orow, int kk0, E (&a)[4]) {
    typedef typename ChainT<E>::v2 v2;
    a[0] = a[1] = a[2] = a[3] = 0;
    if (orow >= M) return;
    if (LEFT) {                                 // K = 2 ml is even and kk0 a multiple of 4: pairs are inside or outside together, aligned to the pair
        const E* p = A + (size_t)2 * ml * orow + kk0;
        if (kk0 < K)     { const v2 v = *(const v2*)p;       a[0] = v.x; a[1] = v.y; }
        if (kk0 + 2 < K) { const v2 v = *(const v2*)(p + 2); a[2] = v.x; a[3] = v.y; }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (kk0 + i < K) a[i] = A[(size_t)ml * (kk0 + i) + orow];
    }
}

// one site: vout[M][T] = (site matrix) x (phi . vin); vin is an LDS tile, vout an LDS tile or the parked vector
template <typename E, int NCT, bool LEFT>
static __device__ __forceinline__ void chain_step(const E* __restrict__ A, int ml, int mr, const E* vin, E* vout,
                                                  const E (&p0)[NCT], const E (&p1)[NCT], int wave, int lane) {
    typedef ChainT<E> Tr;
    const int c16 = lane & 15, q = lane >> 4;
    const int K = LEFT ? 2 * ml : 2 * mr, M = LEFT ? mr : ml;
    const int nrt = (M + 15) >> 4;
    for (int rt = wave; rt < nrt; rt += CHAIN_WAVES) {
        const int orow = rt * 16 + c16;         // the A fragment's row of this lane
        typename Tr::v4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = typename Tr::v4{0, 0, 0, 0};
        E a[4], an[4] = {0, 0, 0, 0};
        chain_load_a<E, LEFT>(A, ml, M, K, orow, 4 * q, a);
        for (int base = 0; base < K; base += 16) {
            if (base + 16 < K) chain_load_a<E, LEFT>(A, ml, M, K, orow, base + 16 + 4 * q, an);  // the next block's values, in flight during this block's MFMAs
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = base + 4 * q + i;
                const bool kok = kk < K;
                int s, vr;
                if (LEFT) { s = kk >= ml ? 1 : 0; vr = kk - (s ? ml : 0); }
                else      { s = kk & 1; vr = kk >> 1; }
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    E b = 0;
                    if (kok) b = (s ? p1[ct] : p0[ct]) * vin[Tr::template idx<NCT>(vr, 16 * ct + c16)];
                    acc[ct] = Tr::mfma(a[i], b, acc[ct]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = an[i];
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = Tr::row(rt, q, r);
                if (row < M) vout[Tr::template idx<NCT>(row, 16 * ct + c16)] = acc[ct][r];
            }
    }
}
