// chain_common.h -- what the chain kernels share: k_chain (kernels_chain.hip, streamed inference), k_response (kernels_response.hip,
// streamed site responses) and k_site_backward / k_site_grad (kernels_sitegrad.hip, streamed site gradients).  Everything here is written
// once over the element type E: double, and float for k_chain<float> (option predict_dtype = 1) and the gradient kernels under option
// gradient_dtype = 1.
//   * All of them: the element-type traits ChainT<E>, the features of a site (chain_features), the A fragment of a 16-wide k block
//     (chain_load_a) and one site of a chain (chain_step); the fragment maps, the k blocks and the arithmetic order are described in the
//     header of kernels_chain.hip.
//     k_input_grad (kernels_inputgrad.hip, streamed input gradients) takes the traits, the fragment maps and the tape's layout from here.
//   * k_response and k_site_backward, which walk the chain inward and then outward: the tape (ChainTape), the taped inward walk
//     (chain_walk_taped), the centre site with weights and pred (chain_centre_taped) and the host side of their launches (taped_launch).
//     The inward walk and the centre are k_chain's, call for call and in its order; that order is stated once, above chain_walk_taped.
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
    static __device__ __forceinline__ int rowq(int q, int r) { return q + 4 * r; }                 // the same inside a 16-row tile
    // the swizzle taken apart, for code that walks a stored row: idx(k, n) = prow(k) * 16 NCT + pc with n = lcol(k, pc); rows 0 .. rows-1
    // lie in the first span(rows) stored rows
    template <int NCT> static __device__ __forceinline__ int prow(int k) { return k; }
    template <int NCT> static __device__ __forceinline__ int lcol(int k, int pc) { return NCT > 1 ? (pc ^ ((k & 1) << 4)) : pc; }
    template <int NCT> static __device__ __forceinline__ int span(int rows) { return rows; }
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
    static __device__ __forceinline__ int rowq(int q, int r) { return 4 * q + r; }
    // the swizzle taken apart (see ChainT<double>): T = 16 permutes rows inside aligned groups of 8, so rows 0 .. rows-1 span ru8(rows) stored rows
    template <int NCT> static __device__ __forceinline__ int prow(int k) { return NCT > 1 ? k : ((k & ~3) | ((k & 1) << 1) | (((k >> 1) ^ (k >> 2)) & 1)); }
    template <int NCT> static __device__ __forceinline__ int lcol(int k, int pc) { return NCT > 1 ? (pc ^ ((((k >> 1) ^ (k >> 2)) & 1) << 4)) : pc; }
    template <int NCT> static __device__ __forceinline__ int span(int rows) { return NCT > 1 ? rows : ((rows + 7) & ~7); }
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

// ---- the taped walk: what k_response and k_site_backward share ----
// A workgroup's slice of a tape: one region of ru16(bond) x T elements per bond b = 0..N (between sites b and b + 1; b = 0 and b = N: the 1
// that starts a chain), in the LDS tile's own element order ChainT<E>::idx<NCT>, region b at row rowoff[b].  The inward tape holds L_b
// for b < cs and R_{b+1} for b >= cs.  A slice is written and read by its own workgroup (and by the launch behind it).
// E = double: k_response and the fp64 gradient kernels; E = float: the gradient kernels under option gradient_dtype = 1, whose tapes
// hold floats in ChainT<float>'s order (T >= 32: the bank function g in address bit 4; T = 16: rows permuted inside groups of 8).
template <typename E, int T> struct ChainTape {
    E* tp; const int* rowoff;
    __device__ __forceinline__ E* bond(int b) const { return tp + (size_t)rowoff[b] * T; }
};
// rows 0 .. rows-1 of a tile or region, as stored: the first ChainT<E>::span(rows) physical rows (what lies beyond row rows-1 in them is never read)
template <typename E, int T>
static __device__ __forceinline__ void chain_copy_rows(const E* src, E* dst, int rows, int tid) {
    const int n = ChainT<E>::template span<T / 16>(rows) * T;
    for (int i = tid; i < n; i += CHAIN_THREADS) dst[i] = src[i];
}

// The inward walk of k_chain<E>, call for call and in its order -- right chain N -> cs+1, whose last vector R_{cs+1} is parked on bond
// cs of the tape, then left chain 1 -> cs-1 -- with every chain vector also copied to the tape (R_j on bond j-1, L_j on bond j).  On return
// buf[cur] holds L_{cs-1}, p0 / p1 the features of the centre site, and every thread has passed the last barrier.
template <typename E, int NCT, int SRC>
static __device__ __forceinline__ int chain_walk_taped(const ChainArgs<E>& ch, E* const (&buf)[2], const ChainTape<E, 16 * NCT>& tape,
                                                       E (&p0)[NCT], E (&p1)[NCT], int tile0, int tid) {
    typedef ChainT<E> Tr;
    constexpr int T = 16 * NCT;
    const int lane = tid & 63, wave = tid >> 6;
    const int N = ch.N, cs = ch.cs, nright = N - cs;
    auto site_at = [&](int t) { return t < nright ? N - t : (t < N - 1 ? t - nright + 1 : cs); };
    E q0[NCT], q1[NCT];
    const int img0 = tile0 + (lane & 15);
    chain_features<E, NCT, SRC>(ch, site_at(0), img0, p0, p1);
    E* const park = tape.bond(cs);                                     // R_{cs+1}
    if (tid < T) {
        const int at = Tr::template idx<NCT>(0, tid);
        buf[0][at] = 1; tape.bond(N)[at] = 1; tape.bond(0)[at] = 1;
    }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < N - 1; ++t) {
        const int j = site_at(t);
        chain_features<E, NCT, SRC>(ch, site_at(t + 1), img0, q0, q1);
        const ChainSite<E> st = ch.sites[j - 1];
        const bool right = t < nright, last = t == nright - 1;
        if (right) {
            chain_step<E, NCT, false>(st.a, st.ml, st.mr, buf[cur], last ? park : buf[cur ^ 1], p0, p1, wave, lane);
            if (last) { if (tid < T) buf[cur ^ 1][Tr::template idx<NCT>(0, tid)] = 1; }        // the left chain starts from 1
        } else {
            chain_step<E, NCT, true>(st.a, st.ml, st.mr, buf[cur], buf[cur ^ 1], p0, p1, wave, lane);
        }
        cur ^= 1;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) { p0[ct] = q0[ct]; p1[ct] = q1[ct]; }
        __syncthreads();
        if (!last) chain_copy_rows<E, T>(buf[cur], right ? tape.bond(j - 1) : tape.bond(j), right ? st.ml : st.mr, tid);
    }
    return cur;
}

// The centre site as k_chain<E> has it: per label l ascending one left-chain step into buf[cur ^ 1] and, by thread tid < T for image
// tile0 + tid, the dot with R (park) over r ascending, w = fma(T[r], R[r], w) from 0 -> wout (fp32: widened); pred = the first maximum of
// |W_l| (util.h:42-57; per-label variant [W_0 > 1/2]), decided on the values of type E -> pred.  weights and pred are therefore bit for
// bit those of k_chain<E>.
// hook(l, w, tid, img) runs in the threads tid < T between the two barriers of label l (w = 0 for an image beyond the chunk).
// Returns pred of the thread's image (threads tid < T inside the chunk).
template <typename E, int NCT, typename Hook>
static __device__ __forceinline__ int chain_centre_taped(const ChainArgs<E>& ch, E* const (&buf)[2], int cur, const E* park,
                                                         const E (&p0)[NCT], const E (&p1)[NCT], int tile0, int tid, Hook hook) {
    typedef ChainT<E> Tr;
    constexpr int T = 16 * NCT;
    const ChainSite<E> sc = ch.sites[ch.cs - 1];
    const size_t lstride = (size_t)sc.ml * 2 * sc.mr;
    const int img = tile0 + tid;
    E best = 0, w0 = 0; int arg = 0;
    for (int l = 0; l < ch.nl; ++l) {
        chain_step<E, NCT, true>(sc.a + l * lstride, sc.ml, sc.mr, buf[cur], buf[cur ^ 1], p0, p1, tid >> 6, tid & 63);
        __syncthreads();
        if (tid < T) {
            E w = 0;
            if (img < ch.cnt) {
                for (int r = 0; r < sc.mr; ++r) w = Tr::fma(buf[cur ^ 1][Tr::template idx<NCT>(r, tid)], park[Tr::template idx<NCT>(r, tid)], w);
                ch.wout[(size_t)img * ch.nl + l] = w;
                const E wa = Tr::abs(w);
                if (l == 0) { best = wa; w0 = w; } else if (wa > best) { best = wa; arg = l; }
            }
            hook(l, w, tid, img);
        }
        __syncthreads();
    }
    const int pr = ch.single ? (w0 > (E)0.5 ? 1 : 0) : arg;
    if (tid < T && img < ch.cnt) ch.pred[img] = pr;
    return pr;
}

// The host side of a launch of k_response / k_site_backward (name and tape_word in the messages): the argument checks, ch.mcap, the grid and
// the dynamic LDS (two tiles + lds_extra bytes), and once per context the LDS attribute of the three tile widths kern[input map][T / 32]
struct TapedLaunch { int grid; size_t lds; bool codes; };
template <typename E, typename K>
static inline int taped_launch(tnml_ctx* c, const char* name, const char* tape_word, ChainArgs<E>& ch, int maxbond, int T, int rows, size_t tape_elems,
                               size_t lds_extra, const K (&kern)[2][3], bool (&attr)[2], TapedLaunch* o) {
    typedef ChainT<E> Tr;
    if (maxbond < 1 || maxbond > Tr::MAXM) return tnml_fail(c, "%s: bond dimension %d outside 1..%d", name, maxbond, Tr::MAXM);
    if (ch.cnt < 1 || ch.cnt > ch.ld) return tnml_fail(c, "%s: %d images in a chunk of %d", name, ch.cnt, ch.ld);
    if (T != 64 && T != 32 && T != 16) return tnml_fail(c, "%s: tile width %d", name, T);
    ch.mcap = (maxbond + 15) / 16 * 16;
    ch.park = nullptr;
    o->grid = (ch.cnt + T - 1) / T;
    o->lds = (size_t)2 * ch.mcap * T * sizeof(E) + lds_extra;
    if (o->lds > TNML_CHAIN_LDS) return tnml_fail(c, "%s: two tiles of %d x %d do not fit the LDS", name, ch.mcap, T);
    if ((size_t)o->grid * T * rows > tape_elems) return tnml_fail(c, "%s: %s of %zu %s too small for %d tiles of %d x %d", name, tape_word, tape_elems, Tr::elems, o->grid, rows, T);
    o->codes = ch.codeT != nullptr;
    if (o->codes && !ch.table) return tnml_fail(c, "%s: block sums without a table", name);
    if (!attr[o->codes]) {
        for (K fn : kern[o->codes])
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, TNML_CHAIN_LDS) != hipSuccess)
                return tnml_fail(c, "%s: hipFuncSetAttribute failed", name);
        attr[o->codes] = true;
    }
    return 0;
}
