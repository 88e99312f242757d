// kernels_chain32.hip -- streamed inference in fp32 (option predict_dtype = 1): the chain kernel of kernels_chain.hip on
// v_mfma_f32_16x16x4_f32.  Same walk: one workgroup (8 waves) carries a tile of T images through all N sites (right chain N -> c+1, left
// chain 1 -> c-1, centre site c), the chain vectors resident in LDS, the site tensors straight from L2, the next site's features and the
// next k block's A values fetched one step ahead.  kernels_chain.hip is not touched: the fp64 path keeps its code.
//
// Operands.  The site tensors are the fp32 copy k_chain_pack32 makes of W once per call (fl32 of every element, in the layout SiteT::a
// has, all sites packed into one workspace).  The features are formed in fp64 by the expressions of the fp64 path and rounded once to
// fp32: the byte expression here in the kernel, the given phi by the staging kernel, the input map's table by the host.
//
// Arithmetic (IEEE fp32, fixed order; per image independent of n, chunk, tile width and tile position):
//   * the B operand of every product is fl32(phi32_s * v): one v_mul_f32, never fused (the file is compiled with -ffp-contract=off);
//   * the contraction index kk runs over the memory order of the site tensor as in kernels_chain.hip (right chain kk = s + 2 r, left
//     chain and centre kk = a + ml s) in blocks of 16; lane (row = lane & 15, q = lane >> 4) holds kk = base + 4 q + i, i = 0..3, and
//     MFMA step i multiplies element i.  The MFMA is a k-ordered fmaf chain, so every output element is ONE chain from 0:
//         for base = 0, 16, ..: for i = 0..3: for q = 0..3:  acc = fmaf(a[kk], b[kk], acc),  kk = base + 4 q + i
//     kk >= K inside the last block contribute fmaf(0, 0, acc);
//   * centre, per label: one such step, then w = fmaf(T[r], R[r], w) for r = 0 .. mr-1 ascending, one image per thread; the output is
//     (double)w; pred = first maximum of |w| over the labels (per-label variant: [w > 0.5f]), decided on the fp32 values.
//   tests/chain32_model.py restates this order; tests/test_predict_f32_gpu.py holds the kernel to it bit for bit.
// A weight that is not finite (the chain has left the fp32 range) raises g.flag with a vector atomic; the host fails the call.
//
// C/D map.  The f32 MFMA stores row = 4 (lane >> 4) + reg, column = lane & 15 -- not the fp64 form's (lane >> 4) + 4 reg.
//
// LDS.  Chain tiles [mcap][T] floats, two ping-pong with one __syncthreads() per site; R waits for the centre in a third tile when three
// fit the 160 KiB, otherwise in the workgroup's slice of the global scratch.  Two tiles <= 128 KiB: T = 64 up to bond 256, 32 up to 512,
// 16 up to 1 024.  ds_read_b32 / ds_write_b32 serve a wave in two groups of 32 lanes over 32 banks, so the two k rows (q = 0, 1 and
// q = 2, 3) of a group, 16 floats each, must fall on different halves of the banks.  Those rows are 2 apart in the right chain
// (row = base / 2 + 2 q + (i >> 1): the lower one has row mod 4 in {0, 1}) and 4 apart in the left chain, the centre and the C/D store
// (row = 16 rt + 4 q + reg).  g(k) = bit 1 of k xor bit 2 of k differs across both kinds of pair; it is put into address bit 4 (in floats):
//   T >= 32: column ^ (g(k) << 4), the row pitch being a multiple of 32 floats;
//   T = 16:  the rows of every aligned group of 8 are permuted, row bits (b2 b1 b0) -> (b2, b0, b1 ^ b2), so that bit 0 of the stored
//            row -- address bit 4 -- is g(k).
// (a left-chain block that straddles kk = ml pairs rows 4 - ml apart: at most one block per site keeps a 2-way conflict.)
//
// Latency.  The MFMA issues every 32 cycles per SIMD and has 40 cycles of dependent latency.  At T = 16 a wave has one accumulator, so
// alone it would issue every 40 cycles; the workgroup's 8 waves sit two to a SIMD and two dependent chains ask for 64 issue cycles
// per 40, so the pipe, not the latency, is the limit whenever a site has 8 or more row tiles.  No second row tile is interleaved.
#include "tnml_internal.h"

typedef float chain_f4 __attribute__((ext_vector_type(4)));
typedef float chain_f2 __attribute__((ext_vector_type(2)));

#define CHAIN32_THREADS 512
#define CHAIN32_WAVES 8

template <int NCT>
static __device__ __forceinline__ int chain32_idx(int k, int n) {
    const int g = ((k >> 1) ^ (k >> 2)) & 1;
    if (NCT > 1) return k * (16 * NCT) + (n ^ (g << 4));
    return ((k & ~3) | ((k & 1) << 1) | g) * 16 + n;
}

// features of site j (1-indexed) for the NCT columns of this lane, rounded once to fp32; images beyond cnt get (0, 0)
// SRC 0: bytes through the built-in expression (g.xT) or the staged fp32 features (g.phiT); SRC 1: the input map (g.codeT, g.table)
template <int NCT, int SRC>
static __device__ __forceinline__ void chain32_features(const ChainArgs32& g, int j, int img0, float (&p0)[NCT], float (&p1)[NCT]) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int n = img0 + 16 * ct;
        float f0 = 0.f, f1 = 0.f;
        if (n < g.cnt) {
            if (SRC == 1) {
                const unsigned code = g.codeT[(size_t)(j - 1) * g.ld + n];
                const chain_f2 f = *(const chain_f2*)(g.table + (size_t)2 * code);
                f0 = f.x; f1 = f.y;
            } else if (g.xT) {                         // the fp64 expression of k_chain, then one rounding
                const double gq = (double)g.xT[(size_t)(j - 1) * g.ld + n] / 255.;
                f0 = 1.f;
                f1 = (float)((gq / 255.) / 4.);
            } else {
                f0 = g.phiT[((size_t)(j - 1) * 2 + 0) * g.ld + n];
                f1 = g.phiT[((size_t)(j - 1) * 2 + 1) * g.ld + n];
            }
        }
        p0[ct] = f0; p1[ct] = f1;
    }
}

// the four values kk = kk0 + i of output row `orow`; masked outside the tensor
template <bool LEFT>
static __device__ __forceinline__ void chain32_load_a(const float* __restrict__ A, int ml, int M, int K, int orow, int kk0, float (&a)[4]) {
    a[0] = a[1] = a[2] = a[3] = 0.f;
    if (orow >= M) return;
    if (LEFT) {                                 // K = 2 ml is even and kk0 a multiple of 4: pairs are inside or outside together, 8-byte aligned
        const float* p = A + (size_t)2 * ml * orow + kk0;
        if (kk0 < K)     { const chain_f2 v = *(const chain_f2*)p;       a[0] = v.x; a[1] = v.y; }
        if (kk0 + 2 < K) { const chain_f2 v = *(const chain_f2*)(p + 2); a[2] = v.x; a[3] = v.y; }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (kk0 + i < K) a[i] = A[(size_t)ml * (kk0 + i) + orow];
    }
}

// one site: vout[M][T] = (site matrix) x (phi . vin); vin is an LDS tile, vout an LDS tile or the parked vector
template <int NCT, bool LEFT>
static __device__ __forceinline__ void chain32_step(const float* __restrict__ A, int ml, int mr, const float* vin, float* vout,
                                                    const float (&p0)[NCT], const float (&p1)[NCT], int wave, int lane) {
    const int c16 = lane & 15, q = lane >> 4;
    const int K = LEFT ? 2 * ml : 2 * mr, M = LEFT ? mr : ml;
    const int nrt = (M + 15) >> 4;
    for (int rt = wave; rt < nrt; rt += CHAIN32_WAVES) {
        const int orow = rt * 16 + c16;         // the A fragment's row of this lane
        chain_f4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = chain_f4{0.f, 0.f, 0.f, 0.f};
        float a[4], an[4] = {0.f, 0.f, 0.f, 0.f};
        chain32_load_a<LEFT>(A, ml, M, K, orow, 4 * q, a);
        for (int base = 0; base < K; base += 16) {
            if (base + 16 < K) chain32_load_a<LEFT>(A, ml, M, K, orow, base + 16 + 4 * q, an);   // the next block's values, in flight during this block's MFMAs
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = base + 4 * q + i;
                const bool kok = kk < K;
                int s, vr;
                if (LEFT) { s = kk >= ml ? 1 : 0; vr = kk - (s ? ml : 0); }
                else      { s = kk & 1; vr = kk >> 1; }
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    float b = 0.f;
                    if (kok) b = (s ? p1[ct] : p0[ct]) * vin[chain32_idx<NCT>(vr, 16 * ct + c16)];
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b, acc[ct], 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = an[i];
        }
        // C/D map of the f32 MFMA: column = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rt * 16 + 4 * q + r;
                if (row < M) vout[chain32_idx<NCT>(row, 16 * ct + c16)] = acc[ct][r];
            }
    }
}

template <int NCT, int SRC>
__global__ __launch_bounds__(CHAIN32_THREADS) void k_chain32(const ChainArgs32 g) {
    constexpr int T = 16 * NCT;
    extern __shared__ __attribute__((aligned(16))) float ch32_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile0 = blockIdx.x * T;
    const size_t tile_elems = (size_t)g.mcap * T;
    float* buf[2] = {ch32_lds, ch32_lds + tile_elems};
    float* park = g.park ? g.park + (size_t)blockIdx.x * tile_elems : ch32_lds + 2 * tile_elems;
    const int N = g.N, cs = g.cs, nright = N - cs;
    // walk order: N .. cs+1 (right chain), 1 .. cs-1 (left chain), cs (centre)
    auto site_at = [&](int t) { return t < nright ? N - t : (t < N - 1 ? t - nright + 1 : cs); };

    float p0[NCT], p1[NCT], q0[NCT], q1[NCT];
    const int img0 = tile0 + (lane & 15);
    chain32_features<NCT, SRC>(g, site_at(0), img0, p0, p1);
    if (tid < T) { buf[0][chain32_idx<NCT>(0, tid)] = 1.f; if (nright == 0) park[chain32_idx<NCT>(0, tid)] = 1.f; }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < N - 1; ++t) {
        const int j = site_at(t);
        chain32_features<NCT, SRC>(g, site_at(t + 1), img0, q0, q1);         // the next site's features, loaded ahead of the barrier
        const ChainSite32 st = g.sites[j - 1];
        if (t < nright) {
            const bool last = t == nright - 1;
            chain32_step<NCT, false>(st.a, st.ml, st.mr, buf[cur], last ? park : buf[cur ^ 1], p0, p1, wave, lane);
            if (last) { if (tid < T) buf[cur ^ 1][chain32_idx<NCT>(0, tid)] = 1.f; }     // the left chain starts from 1
            cur ^= 1;
        } else {
            chain32_step<NCT, true>(st.a, st.ml, st.mr, buf[cur], buf[cur ^ 1], p0, p1, wave, lane);
            cur ^= 1;
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) { p0[ct] = q0[ct]; p1[ct] = q1[ct]; }
        __syncthreads();
    }
    // centre site: per label one left-chain step into the free tile, then the dot with R over r = 0 .. mr-1 in order, one image per thread
    const ChainSite32 sc = g.sites[cs - 1];
    const int img = tile0 + tid;
    float best = 0.f, w0 = 0.f; int arg = 0; bool bad = false;
    for (int l = 0; l < g.nl; ++l) {
        chain32_step<NCT, true>(sc.a + (size_t)l * sc.ml * 2 * sc.mr, sc.ml, sc.mr, buf[cur], buf[cur ^ 1], p0, p1, wave, lane);
        __syncthreads();
        if (tid < T && img < g.cnt) {
            float w = 0.f;
            for (int r = 0; r < sc.mr; ++r) w = __builtin_fmaf(buf[cur ^ 1][chain32_idx<NCT>(r, tid)], park[chain32_idx<NCT>(r, tid)], w);
            g.wout[(size_t)img * g.nl + l] = (double)w;
            const float wa = __builtin_fabsf(w);
            if (!(wa <= 3.402823466e+38f)) bad = true;                                  // Inf or NaN
            if (l == 0) { best = wa; w0 = w; } else if (wa > best) { best = wa; arg = l; }      // first maximum of |W_l| (util.h:42-57)
        }
        __syncthreads();
    }
    if (tid < T && img < g.cnt) {
        g.pred[img] = g.single ? (w0 > 0.5f ? 1 : 0) : arg;
        if (bad) atomicOr(g.flag, 1);
    }
}

// features as given [cnt][N][2] doubles -> site-first [N][2][ld] floats, rounded once
__global__ void k_chain32_stage_phi(const double* __restrict__ phi, int N, int cnt, int ld, float* __restrict__ phiT) {
    const size_t total = (size_t)N * 2 * cnt;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int js = (int)(idx / cnt), n = (int)(idx % cnt);          // js = 2 (j - 1) + s
        phiT[(size_t)js * ld + n] = (float)phi[(size_t)n * 2 * N + js];
    }
}
int launch_chain32_stage_phi(tnml_ctx* c, const double* phi, int N, int cnt, int ld, float* phiT) {
    ProfScope ps(c, KC_PACK);
    const size_t total = (size_t)N * cnt * 2;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_chain32_stage_phi, dim3(grid), dim3(256), 0, c->stream, phi, N, cnt, ld, phiT);
    HIPCK(c, hipGetLastError());
    return 0;
}

// W -> its fp32 copy: blockIdx.y is the site, src[site] the fp64 tensor where it lives, dst[site] its place in the packed workspace;
// the Label site `lsite` (1-indexed; none: <= 0) carries nl times the elements
__global__ void k_chain_pack32(const ChainSite* __restrict__ src, const ChainSite32* __restrict__ dst, int lsite, int nl) {
    const ChainSite s = src[blockIdx.y];
    float* d = const_cast<float*>(dst[blockIdx.y].a);
    const size_t total = (size_t)2 * s.ml * s.mr * ((int)blockIdx.y + 1 == lsite ? nl : 1);
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) d[idx] = (float)s.a[idx];
}
int launch_chain_pack32(tnml_ctx* c, const ChainSite* src, const ChainSite32* dst, int N, int lsite, int nl, size_t largest) {
    if (N < 1 || N > 65535) return tnml_fail(c, "fp32 copy of W: %d sites", N);
    ProfScope ps(c, KC_PACK);
    const int gx = (int)std::max<size_t>(1, std::min<size_t>((largest + 255) / 256, 64));
    hipLaunchKernelGGL(k_chain_pack32, dim3(gx, N), dim3(256), 0, c->stream, src, dst, lsite, nl);
    HIPCK(c, hipGetLastError());
    return 0;
}

// tile width for a chunk of cnt images at largest bond dimension maxbond (<= TNML_CHAIN32_MAXM): the widest the LDS budget allows
// (two tiles of ru16(maxbond) x T floats <= 128 KiB), halved while that leaves compute units without a workgroup
int chain32_tile(tnml_ctx* c, int maxbond, int cnt) {
    int T = maxbond <= 256 ? 64 : (maxbond <= 512 ? 32 : 16);
    if (c->predict_tile) return std::min(T, c->predict_tile);
    if (!c->cu_count) { hipDeviceProp_t pr; c->cu_count = hipGetDeviceProperties(&pr, c->cfg.device) == hipSuccess ? pr.multiProcessorCount : 256; }
    while (T > 16 && (cnt + T - 1) / T < c->cu_count) T /= 2;
    return T;
}

// a.mcap, a.park (null: R parked in LDS) and the grid follow from T; park_ws is the context's scratch of park_elems floats
int launch_chain32(tnml_ctx* c, ChainArgs32 a, int maxbond, int T, float* park_ws, size_t park_elems) {
    if (maxbond < 1 || maxbond > TNML_CHAIN32_MAXM) return tnml_fail(c, "fp32 chain kernel: bond dimension %d outside 1..%d", maxbond, TNML_CHAIN32_MAXM);
    if (a.cnt < 1 || a.cnt > a.ld) return tnml_fail(c, "fp32 chain kernel: %d images in a chunk of %d", a.cnt, a.ld);
    if (T != 64 && T != 32 && T != 16) return tnml_fail(c, "fp32 chain kernel: tile width %d", T);
    if (!a.flag) return tnml_fail(c, "fp32 chain kernel: no range flag");
    a.mcap = (maxbond + 15) / 16 * 16;
    const size_t tile = (size_t)a.mcap * T * sizeof(float);
    const int grid = (a.cnt + T - 1) / T;
    const bool park_lds = 3 * tile <= TNML_CHAIN_LDS;
    if (2 * tile > TNML_CHAIN_LDS) return tnml_fail(c, "fp32 chain kernel: two tiles of %d x %d do not fit the LDS", a.mcap, T);
    if (!park_lds && (size_t)grid * a.mcap * T > park_elems) return tnml_fail(c, "fp32 chain kernel: scratch of %zu floats too small for %d tiles of %d x %d", park_elems, grid, a.mcap, T);
    a.park = park_lds ? nullptr : park_ws;
    const size_t lds = (park_lds ? 3 : 2) * tile;
    const bool codes = a.codeT != nullptr;
    if (codes && !a.table) return tnml_fail(c, "fp32 chain kernel: block sums without a table");
    if (codes ? !c->attr_chain32_codes : !c->attr_chain32) {
        const void* f[3];
        if (codes) { f[0] = reinterpret_cast<const void*>(k_chain32<1, 1>); f[1] = reinterpret_cast<const void*>(k_chain32<2, 1>); f[2] = reinterpret_cast<const void*>(k_chain32<4, 1>); }
        else       { f[0] = reinterpret_cast<const void*>(k_chain32<1, 0>); f[1] = reinterpret_cast<const void*>(k_chain32<2, 0>); f[2] = reinterpret_cast<const void*>(k_chain32<4, 0>); }
        for (const void* fn : f)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, TNML_CHAIN_LDS) != hipSuccess) return tnml_fail(c, "fp32 chain kernel: hipFuncSetAttribute failed");
        (codes ? c->attr_chain32_codes : c->attr_chain32) = true;
    }
    ProfScope ps(c, KC_CHAIN);
    if (codes) {
        if (T == 64)      hipLaunchKernelGGL((k_chain32<4, 1>), dim3(grid), dim3(CHAIN32_THREADS), lds, c->stream, a);
        else if (T == 32) hipLaunchKernelGGL((k_chain32<2, 1>), dim3(grid), dim3(CHAIN32_THREADS), lds, c->stream, a);
        else              hipLaunchKernelGGL((k_chain32<1, 1>), dim3(grid), dim3(CHAIN32_THREADS), lds, c->stream, a);
    } else {
        if (T == 64)      hipLaunchKernelGGL((k_chain32<4, 0>), dim3(grid), dim3(CHAIN32_THREADS), lds, c->stream, a);
        else if (T == 32) hipLaunchKernelGGL((k_chain32<2, 0>), dim3(grid), dim3(CHAIN32_THREADS), lds, c->stream, a);
        else              hipLaunchKernelGGL((k_chain32<1, 0>), dim3(grid), dim3(CHAIN32_THREADS), lds, c->stream, a);
    }
    HIPCK(c, hipGetLastError());
    return 0;
}
