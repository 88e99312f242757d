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
// SRC 0: bytes through the built-in expression (g.xT) or fp64 features (g.phiT), chosen at run time as before the input map existed;
// SRC 1: the input map -- one 2-byte block sum and one dependent 16-byte table row per site and column (g.codeT, g.table; the table
// is at most 261 KB and stays in L2).  The source is a template parameter so that the SRC 0 instantiations carry nothing of it.
template <int NCT, int SRC>
static __device__ __forceinline__ void chain_features(const ChainArgs& g, int j, int img0, double (&p0)[NCT], double (&p1)[NCT]) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int n = img0 + 16 * ct;
        double f0 = 0., f1 = 0.;
        if (n < g.cnt) {
            if (SRC == 1) {
                const unsigned code = g.codeT[(size_t)(j - 1) * g.ld + n];
                const chain_d2 f = *(const chain_d2*)(g.table + (size_t)2 * code);
                f0 = f.x; f1 = f.y;
            } else if (g.xT) {                         // the expression of k_features_u8<double> (kernels_stream.hip)
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

template <int NCT, int SRC>
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
    chain_features<NCT, SRC>(g, site_at(0), img0, p0, p1);
    if (tid < T) { buf[0][chain_idx<NCT>(0, tid)] = 1.; if (nright == 0) park[chain_idx<NCT>(0, tid)] = 1.; }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < N - 1; ++t) {
        const int j = site_at(t);
        chain_features<NCT, SRC>(g, site_at(t + 1), img0, q0, q1);           // the next site's features, loaded ahead of the barrier
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

// Input map: raw bytes [cnt][S] -> block sums, site-first codes[N][ld] with the image index fastest -- the LDS-tiled transpose of the byte
// path with the block sum folded in.  A workgroup takes 64 images x a group of output rows x a chunk of output columns: it copies the
// source-row pieces under them into LDS with consecutive threads on consecutive bytes of an image's rows (byte loads: with S odd no
// image after the first is dword-aligned; full-width rows of one image follow each other in memory, so a group of rows is one run),
// sums the block x block squares in integers, and writes codes with consecutive lanes on consecutive images (128-byte rows of 16-bit
// values).  The LDS pitch of an image is an odd number of dwords, so the 64 lanes of the summing phase fall on 64 different banks.
// Source pixels outside every block are never read.
#define STAGE_IMGS 64
#define STAGE_THREADS 256
#define STAGE_IMG_BYTES 512        /* LDS bytes per image a workgroup aims at: 64 block^2 at block = 8, one output site */
struct StageLaunch { int ncc, nry, pitch; };
// output columns and rows per workgroup and the LDS pitch (bytes) of an image
static StageLaunch stage_shape(const StageGeom& g) {
    StageLaunch s;
    const int b2 = g.block * g.block;
    s.ncc = std::max(1, std::min(g.out_cols, STAGE_IMG_BYTES / b2));
    s.nry = std::max(1, std::min(g.out_rows, STAGE_IMG_BYTES / (b2 * s.ncc)));
    int dw = (b2 * s.ncc * s.nry + 3) / 4;
    if (!(dw & 1)) dw += 1;
    s.pitch = 4 * dw;
    return s;
}
__global__ __launch_bounds__(STAGE_THREADS) void k_stage_codes(const uint8_t* __restrict__ raw, const StageGeom g, int ncc, int nry, int pitch, int cnt, int ld, uint16_t* __restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t st_lds[];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * STAGE_IMGS, oy0 = blockIdx.y * nry, oc0 = blockIdx.z * ncc;
    const int ncol = min(ncc, g.out_cols - oc0), nrow = min(nry, g.out_rows - oy0), nimg = min(STAGE_IMGS, cnt - n0);
    const int wc = g.block * ncol, per_img = g.block * nrow * wc;       // bytes of one source-row piece, of all block * nrow pieces of an image (<= pitch)
    const size_t src0 = (size_t)(g.row0 + g.block * oy0) * g.src_cols + g.col0 + g.block * oc0;
    for (int i = tid; i < nimg * per_img; i += STAGE_THREADS) {
        const int img = i / per_img, rem = i - img * per_img, r = rem / wc, x = rem - r * wc;
        st_lds[img * pitch + rem] = raw[(size_t)(n0 + img) * g.S + src0 + (size_t)r * g.src_cols + x];
    }
    __syncthreads();
    for (int i = tid; i < nrow * ncol * STAGE_IMGS; i += STAGE_THREADS) {
        const int img = i & (STAGE_IMGS - 1), q = i / STAGE_IMGS, oyl = q / ncol, oc = q - oyl * ncol;
        if (img >= nimg) continue;
        const uint8_t* p = st_lds + img * pitch + oyl * g.block * wc + oc * g.block;
        unsigned sum = 0;
        for (int r = 0; r < g.block; ++r) for (int dx = 0; dx < g.block; ++dx) sum += p[r * wc + dx];
        codes[(size_t)((oy0 + oyl) * g.out_cols + oc0 + oc) * ld + n0 + img] = (uint16_t)sum;     // <= 255 * 64
    }
}
int launch_stage_codes(tnml_ctx* c, const uint8_t* raw, const StageGeom& g, int cnt, int ld, uint16_t* codes) {
    if (cnt < 1 || cnt > ld) return tnml_fail(c, "input map staging: %d images in rows of %d", cnt, ld);
    if (g.block < 1 || g.block > 8 || g.row0 < 0 || g.col0 < 0 || g.out_rows < 1 || g.out_cols < 1 || g.src_cols < g.col0 + (int64_t)g.block * g.out_cols ||
        (int64_t)g.S < (g.row0 + (int64_t)g.block * g.out_rows) * g.src_cols)
        return tnml_fail(c, "input map staging: a block leaves the source image");
    const StageLaunch s = stage_shape(g);
    const dim3 grid((cnt + STAGE_IMGS - 1) / STAGE_IMGS, (g.out_rows + s.nry - 1) / s.nry, (g.out_cols + s.ncc - 1) / s.ncc);
    if (grid.y > 65535 || grid.z > 65535) return tnml_fail(c, "input map staging: %d x %d sites are too many", g.out_rows, g.out_cols);
    hipLaunchKernelGGL(k_stage_codes, grid, dim3(STAGE_THREADS), (size_t)STAGE_IMGS * s.pitch, c->stream, raw, g, s.ncc, s.nry, s.pitch, cnt, ld, codes);
    HIPCK(c, hipGetLastError());
    return 0;
}
// block sums -> stored features (tnml_set_data_u8 under a map): one thread per (site, image), reads and writes along the image index
template <typename TE>
__global__ void k_codes_phi(const uint16_t* __restrict__ codes, const TE* __restrict__ tab, int N, int NT, int NTp, TE* __restrict__ phi) {
    const size_t total = (size_t)N * NTp;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t j = idx / NTp; const int n = (int)(idx - j * NTp);
        TE f0 = 0, f1 = 0;
        if (n < NT) { const unsigned code = codes[idx]; f0 = tab[2 * code]; f1 = tab[2 * code + 1]; }
        phi[(j * 2 + 0) * NTp + n] = f0;
        phi[(j * 2 + 1) * NTp + n] = f1;
    }
}
int launch_codes_phi(tnml_ctx* c, const uint16_t* codes, const void* tab, int N, int NT, int NTp, void* phi) {
    const size_t total = (size_t)N * NTp;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 4096);
    if (c->env64()) hipLaunchKernelGGL(k_codes_phi<double>, dim3(grid), dim3(256), 0, c->stream, codes, (const double*)tab, N, NT, NTp, (double*)phi);
    else            hipLaunchKernelGGL(k_codes_phi<float>, dim3(grid), dim3(256), 0, c->stream, codes, (const float*)tab, N, NT, NTp, (float*)phi);
    HIPCK(c, hipGetLastError());
    return 0;
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
    const bool codes = a.codeT != nullptr;
    if (codes ? !c->attr_chain_codes : !c->attr_chain) {
        const void* f[3];
        if (codes) { f[0] = reinterpret_cast<const void*>(k_chain<1, 1>); f[1] = reinterpret_cast<const void*>(k_chain<2, 1>); f[2] = reinterpret_cast<const void*>(k_chain<4, 1>); }
        else       { f[0] = reinterpret_cast<const void*>(k_chain<1, 0>); f[1] = reinterpret_cast<const void*>(k_chain<2, 0>); f[2] = reinterpret_cast<const void*>(k_chain<4, 0>); }
        for (const void* fn : f)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, TNML_CHAIN_LDS) != hipSuccess) return tnml_fail(c, "chain kernel: hipFuncSetAttribute failed");
        (codes ? c->attr_chain_codes : c->attr_chain) = true;
    }
    if (codes && !a.table) return tnml_fail(c, "chain kernel: block sums without a table");
    ProfScope ps(c, KC_CHAIN);
    if (T != 64 && T != 32 && T != 16) return tnml_fail(c, "chain kernel: tile width %d", T);
    if (codes) {
        if (T == 64)      hipLaunchKernelGGL((k_chain<4, 1>), dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
        else if (T == 32) hipLaunchKernelGGL((k_chain<2, 1>), dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
        else              hipLaunchKernelGGL((k_chain<1, 1>), dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
    } else {
        if (T == 64)      hipLaunchKernelGGL((k_chain<4, 0>), dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
        else if (T == 32) hipLaunchKernelGGL((k_chain<2, 0>), dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
        else              hipLaunchKernelGGL((k_chain<1, 0>), dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
    }
    HIPCK(c, hipGetLastError());
    return 0;
}
