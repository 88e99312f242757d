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
//
// Element type.  Everything below is written once over the element type E: double (option predict_dtype = 0, v_mfma_f64_16x16x4_f64 on
// W where it lives) and float (predict_dtype = 1, v_mfma_f32_16x16x4_f32 on the fp32 copy k_chain_pack32 makes of W once per call: fl32
// of every element, in the layout SiteT::a has, all sites packed into one workspace).  What differs between the two -- the MFMA and its
// C/D map, the LDS swizzle, the non-finite flag, the tile thresholds -- is in ChainT<E>, each with its reasoning.  In fp32 the features
// are formed in fp64 by the expressions of the fp64 path and rounded once: the byte expression here in the kernel, the given phi by the
// staging kernel, the input map's table by the host.
//
// Arithmetic of the fp32 kernel (IEEE fp32, fixed order; per image independent of n, chunk, tile width and tile position):
//   * the B operand of every product is fl32(phi32_s * v): one v_mul_f32, never fused (the file is compiled with -ffp-contract=off);
//   * the contraction index kk runs over the memory order of the site tensor as above (right chain kk = s + 2 r, left chain and centre
//     kk = a + ml s) in blocks of 16; lane (row = lane & 15, q = lane >> 4) holds kk = base + 4 q + i, i = 0..3, and MFMA step i
//     multiplies element i.  The MFMA is a k-ordered fmaf chain, so every output element is ONE chain from 0:
//         for base = 0, 16, ..: for i = 0..3: for q = 0..3:  acc = fmaf(a[kk], b[kk], acc),  kk = base + 4 q + i
//     kk >= K inside the last block contribute fmaf(0, 0, acc);
//   * centre, per label: one such step, then w = fmaf(T[r], R[r], w) for r = 0 .. mr-1 ascending, one image per thread; the output is
//     (double)w; pred = first maximum of |w| over the labels (per-label variant: [w > 0.5f]), decided on the fp32 values.
//   tests/chain32_model.py restates this order; tests/test_predict_f32_gpu.py holds the kernel to it bit for bit.
// A weight that is not finite (the chain has left the fp32 range) raises g.flag with a vector atomic; the host fails the call.
//
// Latency (fp32).  The MFMA issues every 32 cycles per SIMD and has 40 cycles of dependent latency.  At T = 16 a wave has one
// accumulator, so alone it would issue every 40 cycles; the workgroup's 8 waves sit two to a SIMD and two dependent chains ask for 64
// issue cycles per 40, so the pipe, not the latency, is the limit whenever a site has 8 or more row tiles.  No second row tile is
// interleaved.
#include "tnml_internal.h"
#include "chain_common.h"       // ChainT<E>, chain_features, chain_load_a, chain_step: shared with k_response (kernels_response.hip)

template <typename E, int NCT, int SRC>
__global__ __launch_bounds__(CHAIN_THREADS) void k_chain(const ChainArgs<E> g) {
    typedef ChainT<E> Tr;
    constexpr int T = 16 * NCT;
    extern __shared__ __attribute__((aligned(16))) unsigned char ch_lds_raw[];
    E* const ch_lds = reinterpret_cast<E*>(ch_lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile0 = blockIdx.x * T;
    const size_t tile_elems = (size_t)g.mcap * T;
    E* buf[2] = {ch_lds, ch_lds + tile_elems};
    E* park = g.park ? g.park + (size_t)blockIdx.x * tile_elems : ch_lds + 2 * tile_elems;
    const int N = g.N, cs = g.cs, nright = N - cs;
    // walk order: N .. cs+1 (right chain), 1 .. cs-1 (left chain), cs (centre)
    auto site_at = [&](int t) { return t < nright ? N - t : (t < N - 1 ? t - nright + 1 : cs); };

    E p0[NCT], p1[NCT], q0[NCT], q1[NCT];
    const int img0 = tile0 + (lane & 15);
    chain_features<E, NCT, SRC>(g, site_at(0), img0, p0, p1);
    if (tid < T) { buf[0][Tr::template idx<NCT>(0, tid)] = 1; if (nright == 0) park[Tr::template idx<NCT>(0, tid)] = 1; }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < N - 1; ++t) {
        const int j = site_at(t);
        chain_features<E, NCT, SRC>(g, site_at(t + 1), img0, q0, q1);        // the next site's features, loaded ahead of the barrier
        const ChainSite<E> st = g.sites[j - 1];
        if (t < nright) {
            const bool last = t == nright - 1;
            chain_step<E, NCT, false>(st.a, st.ml, st.mr, buf[cur], last ? park : buf[cur ^ 1], p0, p1, wave, lane);
            if (last) { if (tid < T) buf[cur ^ 1][Tr::template idx<NCT>(0, tid)] = 1; }        // the left chain starts from 1
            cur ^= 1;
        } else {
            chain_step<E, NCT, true>(st.a, st.ml, st.mr, buf[cur], buf[cur ^ 1], p0, p1, wave, lane);
            cur ^= 1;
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) { p0[ct] = q0[ct]; p1[ct] = q1[ct]; }
        __syncthreads();
    }
    // centre site: per label one left-chain step into the free tile, then the dot with R over r = 0 .. mr-1 in order, one image per thread
    const ChainSite<E> sc = g.sites[cs - 1];
    const int img = tile0 + tid;
    E best = 0, w0 = 0; int arg = 0; bool bad = false;
    for (int l = 0; l < g.nl; ++l) {
        chain_step<E, NCT, true>(sc.a + (size_t)l * sc.ml * 2 * sc.mr, sc.ml, sc.mr, buf[cur], buf[cur ^ 1], p0, p1, wave, lane);
        __syncthreads();
        if (tid < T && img < g.cnt) {
            E w = 0;
            for (int r = 0; r < sc.mr; ++r) w = Tr::fma(buf[cur ^ 1][Tr::template idx<NCT>(r, tid)], park[Tr::template idx<NCT>(r, tid)], w);
            g.wout[(size_t)img * g.nl + l] = (double)w;
            const E wa = Tr::abs(w);
            if (Tr::bad(wa)) bad = true;
            if (l == 0) { best = wa; w0 = w; } else if (wa > best) { best = wa; arg = l; }      // first maximum of |W_l| (util.h:42-57)
        }
        __syncthreads();
    }
    if (tid < T && img < g.cnt) {
        g.pred[img] = g.single ? (w0 > (E)0.5 ? 1 : 0) : arg;
        if (bad) atomicOr(g.flag, 1);
    }
}
// images-first input -> the chunk-local site-first images the chain kernel reads: bytes [cnt][N] -> [N][ld], features [cnt][N][2] doubles -> [N][2][ld] of E, rounded once
__global__ void k_chain_stage_u8(const uint8_t* __restrict__ pix, int N, int cnt, int ld, uint8_t* __restrict__ xT) {
    const size_t total = (size_t)N * cnt;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(idx / cnt), n = (int)(idx % cnt);
        xT[(size_t)j * ld + n] = pix[(size_t)n * N + j];
    }
}
// S: the element type of the caller's features (double; float for the phi32 of a device-resident batch, which widens exactly)
template <typename E, typename S>
__global__ void k_chain_stage_phi(const S* __restrict__ phi, int N, int cnt, int ld, E* __restrict__ phiT) {
    const size_t total = (size_t)N * 2 * cnt;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int js = (int)(idx / cnt), n = (int)(idx % cnt);          // js = 2 (j - 1) + s
        phiT[(size_t)js * ld + n] = (E)phi[(size_t)n * 2 * N + js];
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

template <typename E>
int launch_chain_stage(tnml_ctx* c, const uint8_t* pix, const double* phi, int N, int cnt, int ld, uint8_t* xT, E* phiT, const float* phi32) {
    ProfScope ps(c, KC_PACK);
    const size_t total = (size_t)N * cnt * (pix ? 1 : 2);
    const int grid = (int)std::min<size_t>((total + 255) / 256, 4096);
    if (pix)      hipLaunchKernelGGL(k_chain_stage_u8, dim3(grid), dim3(256), 0, c->stream, pix, N, cnt, ld, xT);
    else if (phi) hipLaunchKernelGGL((k_chain_stage_phi<E, double>), dim3(grid), dim3(256), 0, c->stream, phi, N, cnt, ld, phiT);
    else          hipLaunchKernelGGL((k_chain_stage_phi<E, float>), dim3(grid), dim3(256), 0, c->stream, phi32, N, cnt, ld, phiT);
    HIPCK(c, hipGetLastError());
    return 0;
}
template int launch_chain_stage<double>(tnml_ctx*, const uint8_t*, const double*, int, int, int, uint8_t*, double*, const float*);
template int launch_chain_stage<float>(tnml_ctx*, const uint8_t*, const double*, int, int, int, uint8_t*, float*, const float*);

// W -> its fp32 copy: blockIdx.y is the site, src[site] the fp64 tensor where it lives, dst[site] its place in the packed workspace;
// the Label site `lsite` (1-indexed; none: <= 0) carries nl times the elements
__global__ void k_chain_pack32(const ChainSite<double>* __restrict__ src, const ChainSite<float>* __restrict__ dst, int lsite, int nl) {
    const ChainSite<double> s = src[blockIdx.y];
    float* d = const_cast<float*>(dst[blockIdx.y].a);
    const size_t total = (size_t)2 * s.ml * s.mr * ((int)blockIdx.y + 1 == lsite ? nl : 1);
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) d[idx] = (float)s.a[idx];
}
int launch_chain_pack32(tnml_ctx* c, const ChainSite<double>* src, const ChainSite<float>* dst, int N, int lsite, int nl, size_t largest) {
    if (N < 1 || N > 65535) return tnml_fail(c, "fp32 copy of W: %d sites", N);
    ProfScope ps(c, KC_PACK);
    const int gx = (int)std::max<size_t>(1, std::min<size_t>((largest + 255) / 256, 64));
    hipLaunchKernelGGL(k_chain_pack32, dim3(gx, N), dim3(256), 0, c->stream, src, dst, lsite, nl);
    HIPCK(c, hipGetLastError());
    return 0;
}

// tile width for a chunk of cnt images at largest bond dimension maxbond (<= ChainT<E>::MAXM): the widest the LDS budget allows
// (two tiles of ru16(maxbond) x T elements <= 128 KiB), halved while that leaves compute units without a workgroup
template <typename E>
int chain_tile(tnml_ctx* c, int maxbond, int cnt) {
    int T = maxbond <= ChainT<E>::T64 ? 64 : (maxbond <= ChainT<E>::T32 ? 32 : 16);
    if (c->predict_tile) return std::min(T, c->predict_tile);
    if (!c->cu_count) { hipDeviceProp_t pr; c->cu_count = hipGetDeviceProperties(&pr, c->cfg.device) == hipSuccess ? pr.multiProcessorCount : 256; }
    while (T > 16 && (cnt + T - 1) / T < c->cu_count) T /= 2;
    return T;
}
template int chain_tile<double>(tnml_ctx*, int, int);
template int chain_tile<float>(tnml_ctx*, int, int);

// a.mcap, a.park (null: R parked in LDS) and the grid follow from T; park_ws is the context's scratch of park_elems elements
template <typename E>
int launch_chain(tnml_ctx* c, ChainArgs<E> a, int maxbond, int T, E* park_ws, size_t park_elems) {
    typedef ChainT<E> Tr;
    constexpr bool f32 = sizeof(E) == sizeof(float);
    if (maxbond < 1 || maxbond > Tr::MAXM) return tnml_fail(c, "%schain kernel: bond dimension %d outside 1..%d", Tr::what, maxbond, Tr::MAXM);
    if (a.cnt < 1 || a.cnt > a.ld) return tnml_fail(c, "%schain kernel: %d images in a chunk of %d", Tr::what, a.cnt, a.ld);
    if (T != 64 && T != 32 && T != 16) return tnml_fail(c, "%schain kernel: tile width %d", Tr::what, T);
    if (f32 && !a.flag) return tnml_fail(c, "%schain kernel: no range flag", Tr::what);
    a.mcap = (maxbond + 15) / 16 * 16;
    const size_t tile = (size_t)a.mcap * T * sizeof(E);
    const int grid = (a.cnt + T - 1) / T;
    const bool park_lds = 3 * tile <= TNML_CHAIN_LDS;
    if (2 * tile > TNML_CHAIN_LDS) return tnml_fail(c, "%schain kernel: two tiles of %d x %d do not fit the LDS", Tr::what, a.mcap, T);
    if (!park_lds && (size_t)grid * a.mcap * T > park_elems)
        return tnml_fail(c, "%schain kernel: scratch of %zu %s too small for %d tiles of %d x %d", Tr::what, park_elems, Tr::elems, grid, a.mcap, T);
    a.park = park_lds ? nullptr : park_ws;
    const size_t lds = (park_lds ? 3 : 2) * tile;
    const bool codes = a.codeT != nullptr;
    if (codes && !a.table) return tnml_fail(c, "%schain kernel: block sums without a table", Tr::what);
    typedef void (*kern_t)(const ChainArgs<E>);
    static const kern_t kern[2][3] = {{k_chain<E, 1, 0>, k_chain<E, 2, 0>, k_chain<E, 4, 0>}, {k_chain<E, 1, 1>, k_chain<E, 2, 1>, k_chain<E, 4, 1>}};   // [SRC][T / 32]
    bool& attr = c->attr_chain[f32][codes];
    if (!attr) {
        for (kern_t fn : kern[codes])
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, TNML_CHAIN_LDS) != hipSuccess)
                return tnml_fail(c, "%schain kernel: hipFuncSetAttribute failed", Tr::what);
        attr = true;
    }
    ProfScope ps(c, KC_CHAIN);
    hipLaunchKernelGGL(kern[codes][T / 32], dim3(grid), dim3(CHAIN_THREADS), lds, c->stream, a);
    HIPCK(c, hipGetLastError());
    return 0;
}
template int launch_chain<double>(tnml_ctx*, ChainArgs<double>, int, int, double*, size_t);
template int launch_chain<float>(tnml_ctx*, ChainArgs<float>, int, int, float*, size_t);
