// kernels_chain.hip -- streamed inference (tnml_predict_u8 / tnml_predict_phi): the whole Label-free contraction of toverlap
// (util.h:19-40) for a tile of T images in ONE launch, the chain vectors resident in LDS.
//
//   right chain N -> c+1   V_out[a][n] = sum_{s,r} A_j[a,s,r] phi_s(x_nj) V_in[r][n]
//   left chain  1 -> c-1   V_out[r][n] = sum_{a,s} A_j[a,s,r] phi_s(x_nj) V_in[a][n]
//   centre site c          W_l(n) = sum_r (sum_{a,s} A_c[a,s,r,l] phi_s L[a][n]) R[r][n],  l = 0..nl-1
//
// One workgroup (8 waves) owns one tile and walks all N sites; nothing is exchanged between workgroups.  Every site is a product
// (site matrix) x (chain tile) on v_mfma_f64_16x16x4_f64 with the images on the MFMA column index (kernels_gemm.hip:13-16): a wave owns
// 16-row output tiles (row tile rt = wave, wave + 8, ...) over all T / 16 column tiles and runs the full contraction index for them, so
// the order of every sum is that of the 16-wide k blocks below -- the same for every T, every tile and every chunk.
//
// k blocks.  The contraction index kk runs over the memory order of the site tensor ([ml][2][mr], first index fastest):
//   right chain  kk = s + 2 r   (stride ml doubles; the output index a is the fastest in memory)
//   left chain   kk = a + ml s  (contiguous; the output index r has stride 2 ml)
// A block is 16 consecutive kk.  Lane (row = lane & 15, q = lane >> 4) holds the four values kk = base + 4 q + i, i = 0..3, of its output
// row and MFMA step i of the block multiplies element i of every lane: the MFMA's own k index q stands for kk = base + 4 q + i, and the
// B fragment of lane (q, column) is phi_s V_in of that same kk.  For the left chain the four values are 32 contiguous bytes per lane,
// so a wave reads 16 rows x 128 bytes in whole lines (the naive fragment would touch 16 lines for 32 bytes each); for the right chain
// each of the four is a coalesced 128-byte read over the 16 rows.  The site tensors are read where tnml_set_site / the split left them
// (SiteT::a), straight from L2: no packed copy, no LDS staging.  Rows and kk beyond the bond dimensions are masked, never read.
//
// LDS: chain tiles [mcap][T] doubles (mcap = the largest bond dimension rounded up to 16), two of them ping-pong with one
// __syncthreads() per site.  The finished right-chain vector R waits for the centre site in a third tile when three fit the 160 KiB,
// otherwise in the workgroup's own slice of a global scratch (written once, read once by the same workgroup).  For T >= 32 the column
// index of odd rows is XORed with 16: the two k rows a half-wave reads with one ds_read_b64 then fall on different banks.
#include "tnml_internal.h"

typedef double chain_d4 __attribute__((ext_vector_type(4)));
typedef double chain_d2 __attribute__((ext_vector_type(2)));

#define CHAIN_THREADS 512
#define CHAIN_WAVES 8

template <int NCT>
static __device__ __forceinline__ int chain_idx(int k, int n) {
    return k * (16 * NCT) + (NCT > 1 ? (n ^ ((k & 1) << 4)) : n);
}

// features of site j (1-indexed) for the NCT columns of this lane: image tile0 + 16 ct + (lane & 15); images beyond cnt get (0, 0)
template <int NCT>
static __device__ __forceinline__ void chain_features(const ChainArgs& g, int j, int img0, double (&p0)[NCT], double (&p1)[NCT]) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int n = img0 + 16 * ct;
        double f0 = 0., f1 = 0.;
        if (n < g.cnt) {
            if (g.xT) {                         // the expression of k_features_u8<double> (kernels_stream.hip)
                const double gq = (double)g.xT[(size_t)(j - 1) * g.ld + n] / 255.;
                f0 = 1.;
                f1 = (gq / 255.) / 4.;
            } else {
                f0 = g.phiT[((size_t)(j - 1) * 2 + 0) * g.ld + n];
                f1 = g.phiT[((size_t)(j - 1) * 2 + 1) * g.ld + n];
            }
        }
        p0[ct] = f0; p1[ct] = f1;
    }
}

// the four values kk = base + 4 q + i of output row `orow` (see the header); masked outside the tensor
template <bool LEFT>
static __device__ __forceinline__ void chain_load_a(const double* __restrict__ A, int ml, int M, int K, int orow, int kk0, double (&a)[4]) {
    a[0] = a[1] = a[2] = a[3] = 0.;
    if (orow >= M) return;
    if (LEFT) {                                 // K = 2 ml is even and kk0 a multiple of 4: pairs are inside or outside together, 16-byte aligned
        const double* p = A + (size_t)2 * ml * orow + kk0;
        if (kk0 < K)     { const chain_d2 v = *(const chain_d2*)p;       a[0] = v.x; a[1] = v.y; }
        if (kk0 + 2 < K) { const chain_d2 v = *(const chain_d2*)(p + 2); a[2] = v.x; a[3] = v.y; }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (kk0 + i < K) a[i] = A[(size_t)ml * (kk0 + i) + orow];
    }
}

// one site: vout[M][T] = (site matrix) x (phi . vin); vin is an LDS tile, vout an LDS tile or the parked vector
template <int NCT, bool LEFT>
static __device__ __forceinline__ void chain_step(const double* __restrict__ A, int ml, int mr, const double* vin, double* vout,
                                                  const double (&p0)[NCT], const double (&p1)[NCT], int wave, int lane) {
    const int c16 = lane & 15, q = lane >> 4;
    const int K = LEFT ? 2 * ml : 2 * mr, M = LEFT ? mr : ml;
    const int nrt = (M + 15) >> 4;
    for (int rt = wave; rt < nrt; rt += CHAIN_WAVES) {
        const int orow = rt * 16 + c16;         // the A fragment's row of this lane
        chain_d4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = chain_d4{0., 0., 0., 0.};
        double a[4], an[4] = {0., 0., 0., 0.};
        chain_load_a<LEFT>(A, ml, M, K, orow, 4 * q, a);
        for (int base = 0; base < K; base += 16) {
            if (base + 16 < K) chain_load_a<LEFT>(A, ml, M, K, orow, base + 16 + 4 * q, an);     // the next block's values, in flight during this block's MFMAs
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = base + 4 * q + i;
                const bool kok = kk < K;
                int s, vr;
                if (LEFT) { s = kk >= ml ? 1 : 0; vr = kk - (s ? ml : 0); }
                else      { s = kk & 1; vr = kk >> 1; }
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    double b = 0.;
                    if (kok) b = (s ? p1[ct] : p0[ct]) * vin[chain_idx<NCT>(vr, 16 * ct + c16)];
                    acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b, acc[ct], 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = an[i];
        }
        // C/D map of the fp64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rt * 16 + q + 4 * r;
                if (row < M) vout[chain_idx<NCT>(row, 16 * ct + c16)] = acc[ct][r];
            }
    }
}

template <int NCT>
__global__ __launch_bounds__(CHAIN_THREADS) void k_chain(const ChainArgs g) {
    constexpr int T = 16 * NCT;
    extern __shared__ __attribute__((aligned(16))) double ch_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile0 = blockIdx.x * T;
    const size_t tile_elems = (size_t)g.mcap * T;
    double* buf[2] = {ch_lds, ch_lds + tile_elems};
    double* park = g.park ? g.park + (size_t)blockIdx.x * tile_elems : ch_lds + 2 * tile_elems;
    const int N = g.N, cs = g.cs, nright = N - cs;
    // walk order: N .. cs+1 (right chain), 1 .. cs-1 (left chain), cs (centre)
    auto site_at = [&](int t) { return t < nright ? N - t : (t < N - 1 ? t - nright + 1 : cs); };

    double p0[NCT], p1[NCT], q0[NCT], q1[NCT];
    const int img0 = tile0 + (lane & 15);
    chain_features<NCT>(g, site_at(0), img0, p0, p1);
    if (tid < T) { buf[0][chain_idx<NCT>(0, tid)] = 1.; if (nright == 0) park[chain_idx<NCT>(0, tid)] = 1.; }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < N - 1; ++t) {
        const int j = site_at(t);
        chain_features<NCT>(g, site_at(t + 1), img0, q0, q1);           // the next site's features, loaded ahead of the barrier
        const ChainSite st = g.sites[j - 1];
        if (t < nright) {
            const bool last = t == nright - 1;
            chain_step<NCT, false>(st.a, st.ml, st.mr, buf[cur], last ? park : buf[cur ^ 1], p0, p1, wave, lane);
            if (last) { if (tid < T) buf[cur ^ 1][chain_idx<NCT>(0, tid)] = 1.; }       // the left chain starts from 1
            cur ^= 1;
        } else {
            chain_step<NCT, true>(st.a, st.ml, st.mr, buf[cur], buf[cur ^ 1], p0, p1, wave, lane);
            cur ^= 1;
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) { p0[ct] = q0[ct]; p1[ct] = q1[ct]; }
        __syncthreads();
    }
    // centre site: per label one left-chain step into the free tile, then the dot with R over r = 0 .. mr-1 in order, one image per thread
    const ChainSite sc = g.sites[cs - 1];
    const int img = tile0 + tid;
    double best = 0., w0 = 0.; int arg = 0;
    for (int l = 0; l < g.nl; ++l) {
        chain_step<NCT, true>(sc.a + (size_t)l * sc.ml * 2 * sc.mr, sc.ml, sc.mr, buf[cur], buf[cur ^ 1], p0, p1, wave, lane);
        __syncthreads();
        if (tid < T && img < g.cnt) {
            double w = 0.;
            for (int r = 0; r < sc.mr; ++r) w = fma(buf[cur ^ 1][chain_idx<NCT>(r, tid)], park[chain_idx<NCT>(r, tid)], w);
            g.wout[(size_t)img * g.nl + l] = w;
            const double wa = fabs(w);
            if (l == 0) { best = wa; w0 = w; } else if (wa > best) { best = wa; arg = l; }      // first maximum of |W_l| (util.h:42-57)
        }
        __syncthreads();
    }
    if (tid < T && img < g.cnt) g.pred[img] = g.single ? (w0 > 0.5 ? 1 : 0) : arg;
}

// images-first input -> the chunk-local site-first images the chain kernel reads: bytes [cnt][N] -> [N][ld], features [cnt][N][2] -> [N][2][ld]
__global__ void k_chain_stage_u8(const uint8_t* __restrict__ pix, int N, int cnt, int ld, uint8_t* __restrict__ xT) {
    const size_t total = (size_t)N * cnt;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(idx / cnt), n = (int)(idx % cnt);
        xT[(size_t)j * ld + n] = pix[(size_t)n * N + j];
    }
}
__global__ void k_chain_stage_phi(const double* __restrict__ phi, int N, int cnt, int ld, double* __restrict__ phiT) {
    const size_t total = (size_t)N * 2 * cnt;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int js = (int)(idx / cnt), n = (int)(idx % cnt);          // js = 2 (j - 1) + s
        phiT[(size_t)js * ld + n] = phi[(size_t)n * 2 * N + js];
    }
}

int launch_chain_stage(tnml_ctx* c, const uint8_t* pix, const double* phi, int N, int cnt, int ld, uint8_t* xT, double* phiT) {
    ProfScope ps(c, KC_PACK);
    const size_t total = (size_t)N * cnt * (pix ? 1 : 2);
    const int grid = (int)std::min<size_t>((total + 255) / 256, 4096);
    if (pix) hipLaunchKernelGGL(k_chain_stage_u8, dim3(grid), dim3(256), 0, c->stream, pix, N, cnt, ld, xT);
    else     hipLaunchKernelGGL(k_chain_stage_phi, dim3(grid), dim3(256), 0, c->stream, phi, N, cnt, ld, phiT);
    HIPCK(c, hipGetLastError());
    return 0;
}

// tile width for a chunk of cnt images at largest bond dimension maxbond (<= TNML_CHAIN_MAXM): the widest the LDS budget allows
// (two tiles of ru16(maxbond) x T doubles <= 128 KiB), halved while that leaves compute units without a workgroup
int chain_tile(tnml_ctx* c, int maxbond, int cnt) {
    int T = maxbond <= 128 ? 64 : (maxbond <= 256 ? 32 : 16);
    if (c->predict_tile) return std::min(T, c->predict_tile);
    if (!c->cu_count) { hipDeviceProp_t pr; c->cu_count = hipGetDeviceProperties(&pr, c->cfg.device) == hipSuccess ? pr.multiProcessorCount : 256; }
    while (T > 16 && (cnt + T - 1) / T < c->cu_count) T /= 2;
    return T;
}

// a.mcap, a.park (null: R parked in LDS) and the grid follow from T; park_ws is the context's scratch of park_elems doubles
int launch_chain(tnml_ctx* c, ChainArgs a, int maxbond, int T, double* park_ws, size_t park_elems) {
    if (maxbond < 1 || maxbond > TNML_CHAIN_MAXM) return tnml_fail(c, "chain kernel: bond dimension %d outside 1..%d", maxbond, TNML_CHAIN_MAXM);
    if (a.cnt < 1 || a.cnt > a.ld) return tnml_fail(c, "chain kernel: %d images in a chunk of %d", a.cnt, a.ld);
    a.mcap = (maxbond + 15) / 16 * 16;
    const size_t tile = (size_t)a.mcap * T * sizeof(double);
    const int grid = (a.cnt + T - 1) / T;
    const bool park_lds = 3 * tile <= TNML_CHAIN_LDS;
    if (2 * tile > TNML_CHAIN_LDS) return tnml_fail(c, "chain kernel: two tiles of %d x %d do not fit the LDS", a.mcap, T);
    if (!park_lds && (size_t)grid * a.mcap * T > park_elems) return tnml_fail(c, "chain kernel: scratch of %zu doubles too small for %d tiles of %d x %d", park_elems, grid, a.mcap, T);
    a.park = park_lds ? nullptr : park_ws;
    const size_t lds = (park_lds ? 3 : 2) * tile;
    if (!c->attr_chain) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_chain<1>), hipFuncAttributeMaxDynamicSharedMemorySize, TNML_CHAIN_LDS) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_chain<2>), hipFuncAttributeMaxDynamicSharedMemorySize, TNML_CHAIN_LDS) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_chain<4>), hipFuncAttributeMaxDynamicSharedMemorySize, TNML_CHAIN_LDS) != hipSuccess)
            return tnml_fail(c, "chain kernel: hipFuncSetAttribute failed");
        c->attr_chain = true;
    }
    ProfScope ps(c, KC_CHAIN);
    if (T == 64)      hipLaunchKernelGGL(k_chain<4>, dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
    else if (T == 32) hipLaunchKernelGGL(k_chain<2>, dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
    else if (T == 16) hipLaunchKernelGGL(k_chain<1>, dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
    else return tnml_fail(c, "chain kernel: tile width %d", T);
    HIPCK(c, hipGetLastError());
    return 0;
}
