// kernels_sitegrad.hip -- streamed site gradients (tnml_site_gradient_u8 / tnml_site_gradient_phi): for a chunk of images and
// coefficients c[n][l] = dC/dW_l(x_n), the gradient of C with respect to every site tensor,
//
//   j < c:   G_j[a,s,r]   += sum_n L_{j-1,n}[a] phi_{n,j}[s] X_{j,n}[r]
//   j > c:   G_j[a,s,r]   += sum_n Y_{j-1,n}[a] phi_{n,j}[s] R_{j+1,n}[r]
//   j = c:   G_c[a,s,r,l] += sum_n c_nl L_{c-1,n}[a] phi_{n,c}[s] R_{c+1,n}[r]
//
// L and R are the inward chain vectors of k_chain / k_response, X and Y the outward vectors on the left and on the right of the Label
// site c (site 1 in the per-label variant), seeded at c with
//   X_{c-1}[a] = sum_l c_nl sum_s phi_{n,c}[s] sum_r A_c[a,s,r,l] R_{c+1}[r],     Y_c[r] = sum_l c_nl sum_s phi_{n,c}[s] sum_a A_c[a,s,r,l] L_{c-1}[a]
// and carried outward by X_{j-1} = (phi_j A_j) X_j, Y_j = Y_{j-1} (phi_j A_j).  Two launches per chunk.
//
// 1. k_site_backward (class site_bwd): one workgroup (8 waves) per tile of T = 64 / 32 / 16 images (chain_tile<double>), two walks.
//    Phase A is k_response's, the same code: the taped inward walk and the centre of chain_common.h (chain_walk_taped,
//    chain_centre_taped; their order and the tape's layout, ChainTape, are stated there), so that weights and pred are bit for bit
//    those of k_chain<double>.
//    Centre: the coefficients of the tile go to LDS [nl][T] (the per-label hook of chain_centre_taped) -- given (coef), or formed from the weight just computed as
//    c_nl = 2 (W_l(x_n) - y_nl) (labels; y as tnml_evaluate_*: [l == label_n], per-label variant [label_n == target]) and written to the
//    [C][nl] buffer the GEMM reads; columns beyond the chunk get 0.  The seeds are chain steps over the compound index (l, s, r):
//    operand fl(fl(c_nl phi_s) R[r]) (resp. L[a]), accumulated by v_mfma_f64_16x16x4_f64 with l ascending and, inside a label, the k
//    blocks of chain_step.  Phase B carries X and Y outward with chain_step itself (the products of k_response without its dots) and
//    writes every outward vector to a second tape with the same region table: X_b on bond b < c, Y_b on bond b >= c.
//    LDS: two chain tiles [mcap][T] and the coefficients [nl][T]: k_chain's tile thresholds carry over.
//
// 2. k_site_grad (class site_grad), the hot path: per site an fp64 GEMM whose reduction index is the image.  The grid runs over
//    (virtual site, 32 x 32 output block), a virtual site being a site or one label of the Label site; a prefix table gives the first
//    block of each.  A workgroup of 4 waves stages, per tile of the chunk, 32 rows of the a-side vector and 32 rows of the r-side
//    vector into LDS, the r side multiplied by the feature while staging (fl(phi_s X[r]); Label site: fl(fl(c_nl phi_s) R[r])); each wave
//    owns a 16 (a) x 16 (r) output tile for both s and issues v_mfma_f64_16x16x4_f64 with the r side as the row operand, so that a
//    lane's outputs are contiguous in a.
//    Summation order, fixed: the accumulators are loaded from G at the chunk's start (the host zeroes G before the first chunk) and
//    stored at its end, chunks in chunk order; inside a chunk the tiles this launch's k_site_backward wrote, in tile order, images
//    ascending, four per MFMA step (step t of a tile multiplies images 4 t .. 4 t + 3, lane group q holding image 4 t + q).  Images
//    beyond the chunk contribute exact zeros: both operands are masked, the r side through its feature / coefficient operand (the
//    tape holds 1 on bonds 0 and N for every column).  Rows beyond a bond are neither read nor stored.
//    G is therefore bit-identical on repeats and independent of the tile width (predict_tile: a narrower tile only moves the same
//    MFMA steps to other tiles, and trailing steps of zeros change nothing).  Its last bits may depend on gradient_chunk: a chunk
//    that is no multiple of 4 images shifts the grouping of the images into MFMA steps.
//
//    k_site_backward<.., .., 1> (labels under option "loss" = TNML_LOSS_SOFTMAX; never the per-label variant): the hook parks the weight
//    itself in the thread's column of the LDS coefficients; after the centre the thread that owns the image turns its column into the
//    coefficients of the softmax cross-entropy (loss_dev.h) and writes them to LDS and to the [C][nl] buffer.  Everything after is shared.
//
// Element type.  Both kernels are written once over E: double (option gradient_dtype = 0, everything above) and float (gradient_dtype = 1),
// which takes ChainT<float> for the MFMA (v_mfma_f32_16x16x4_f32), its C/D map (row = 16 rt + 4 q + reg), the element order of the LDS
// tiles and of both tapes (ChainT<float>::idx) and the tile thresholds (64 up to bond 256, 32 up to 512, 16 up to 1 024).  In fp32:
//   * operands: the fp32 copy of W (k_chain_pack32, once per call), features formed in fp64 and rounded once, as k_chain<float> has them;
//     phase A is k_chain<float>'s walk and centre, so weights and pred are those of tnml_predict_* under predict_dtype = 1 bit for bit;
//   * coefficients: the thread that owns the image widens its weights, forms c in fp64 by the expressions above (2 (W - y), or loss_dev.h),
//     rounds once to fp32 and writes the rounded value, widened, to the [C][nl] buffer; given coefficients are rounded to fp32 once;
//   * seeds and outward walk in fp32, the operand fl32(fl32(c phi_s) v); both tapes hold floats;
//   * k_site_grad<float>: accumulators from 0 in every chunk, the fp32 MFMA over the tiles in the order above (per output element one
//     fmaf chain over the images, four per MFMA step, q ascending), then G[e] = G[e] + (double)acc: one fp64 addition per element and
//     chunk.  G, and so the sum over chunks, stays fp64;
//   * a weight that is not finite raises ch.flag (a plain vector store of 1); the host fails the call.
// tests/grad32_model.py restates this order.
//
// Registers (gfx950 cross-compile; VGPRs at T = 16 / 32 / 64, bytes / input map source alike to within 3; no scratch in any instantiation):
//   k_site_backward<double>: 104 / 127 / 162      k_site_backward<float>: 94 / 99 / 121     (the softmax forms: the same counts, float T = 16: 96)
//   k_site_grad<double>:     60 / 56 / 58 + 16 accumulator registers      k_site_grad<float>: 36 / 33 / 33 + 8
//   k_forward_taped<double>: 96 / 129 / 164       k_forward_taped<float>: 92 / 94 / 121     (input map source: within 2)
//   k_site_outward<double>:  96 / 119 / 161       k_site_outward<float>:  86 / 90 / 115     (input map source at T = 16: 114 and 100)
// No atomics; compiled with -ffp-contract=off like its neighbours.
//
// 3. The same work in two calls (tnml_forward_taped_* / tnml_backward_taped*; the kernels are at the end of this file).  k_forward_taped
//    (class fwd_taped) is phase A alone and leaves weights, pred and the inward tape.  k_site_outward (class site_out) is the centre's seeds
//    and phase B in the coef mode, started from that tape: a grid of (tiles, 2), one workgroup for X and one for Y, each with seed_step and
//    carry_outward as k_site_backward calls them.  The second tape is k_site_backward's bit for bit, so k_site_grad and k_input_grad run
//    behind it unchanged.  No existing kernel's instructions moved (tools/compare_isa.py against the commit before: 71 of 71 identical).
#include "chain_common.h"
#include "loss_dev.h"

#define SG_THREADS 256
#define SG_BLK 32                   /* output block: SG_BLK (a) x SG_BLK (r), both s */

// the seed of an outward walk (see the header): vout[M][T] = sum_l (site matrix of label l) x (c_l phi . vin); vin an LDS tile, vout a tape region
template <typename E, int NCT, bool LEFT>
static __device__ __forceinline__ void seed_step(const E* __restrict__ A, size_t lstride, int nl, int ml, int mr, const E* vin, E* vout,
                                                 const E (&p0)[NCT], const E (&p1)[NCT], const E* cl, int wave, int lane) {
    typedef ChainT<E> Tr;
    constexpr int T = 16 * NCT;
    const int c16 = lane & 15, q = lane >> 4;
    const int K = LEFT ? 2 * ml : 2 * mr, M = LEFT ? mr : ml;
    const int nrt = (M + 15) >> 4;
    for (int rt = wave; rt < nrt; rt += CHAIN_WAVES) {
        const int orow = rt * 16 + c16;
        typename Tr::v4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = typename Tr::v4{0, 0, 0, 0};
        for (int l = 0; l < nl; ++l) {
            E c0[NCT], c1[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const E cv = cl[l * T + 16 * ct + c16];
                c0[ct] = cv * p0[ct]; c1[ct] = cv * p1[ct];
            }
            const E* const Al = A + (size_t)l * lstride;
            for (int base = 0; base < K; base += 16) {
                E a[4];
                chain_load_a<E, LEFT>(Al, ml, M, K, orow, base + 4 * q, a);
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
                        if (kok) b = (s ? c1[ct] : c0[ct]) * vin[Tr::template idx<NCT>(vr, 16 * ct + c16)];
                        acc[ct] = Tr::mfma(a[i], b, acc[ct]);
                    }
                }
            }
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

// One outward walk from the seed on the second tape with chain_step itself, every vector to the second tape.  LEFT is chain_step's:
// false carries X left of the centre (seed of seed_rows on bond cs-1; site j = cs-1 .. 2 writes bond j-1), true carries Y right of it
// (seed on bond cs; site j = cs+1 .. N-1 writes bond j).  Opens with a barrier: the seeds are written, the tiles free.
template <typename E, int NCT, int SRC, bool LEFT>
static __device__ __forceinline__ void carry_outward(const ChainArgs<E>& ch, E* const (&buf)[2], const ChainTape<E, 16 * NCT>& tape2, int seed_rows,
                                                     E (&p0)[NCT], E (&p1)[NCT], int tile0, int tid) {
    constexpr int T = 16 * NCT, D = LEFT ? 1 : -1;
    const int lane = tid & 63, wave = tid >> 6, img0 = tile0 + (lane & 15);
    const int N = ch.N, cs = ch.cs;
    if (LEFT ? cs >= N - 1 : cs <= 2) return;
    E q0[NCT], q1[NCT];
    __syncthreads();
    chain_copy_rows<E, T>(tape2.bond(LEFT ? cs : cs - 1), buf[0], seed_rows, tid);
    chain_features<E, NCT, SRC>(ch, cs + D, img0, p0, p1);
    __syncthreads();
    int cur = 0;
    for (int j = cs + D; LEFT ? j <= N - 1 : j >= 2; j += D) {
        chain_features<E, NCT, SRC>(ch, j + D, img0, q0, q1);
        const ChainSite<E> st = ch.sites[j - 1];
        chain_step<E, NCT, LEFT>(st.a, st.ml, st.mr, buf[cur], buf[cur ^ 1], p0, p1, wave, lane);
        cur ^= 1;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) { p0[ct] = q0[ct]; p1[ct] = q1[ct]; }
        __syncthreads();
        chain_copy_rows<E, T>(buf[cur], tape2.bond(LEFT ? j : j - 1), LEFT ? st.mr : st.ml, tid);
    }
}

template <typename E, int NCT, int SRC, int LOSS = 0>
__global__ __launch_bounds__(CHAIN_THREADS) void k_site_backward(const SiteGradArgsT<E> g) {
    typedef ChainT<E> Tr;
    constexpr bool f32 = sizeof(E) == sizeof(float);
    constexpr int T = 16 * NCT;
    extern __shared__ __attribute__((aligned(16))) unsigned char sg_lds_raw[];
    E* const lds = reinterpret_cast<E*>(sg_lds_raw);
    const ChainArgs<E>& ch = g.ch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile0 = blockIdx.x * T;
    const size_t tile_elems = (size_t)ch.mcap * T;
    E* buf[2] = {lds, lds + tile_elems};
    E* const cl = lds + 2 * tile_elems;                                // [nl][T] coefficients of the tile
    const int N = ch.N, cs = ch.cs;
    const size_t slice = (size_t)blockIdx.x * g.rowoff[N + 1] * T;
    const ChainTape<E, T> tape{g.tape + slice, g.rowoff};              // inward vectors (chain_common.h)
    const ChainTape<E, T> tape2{g.tape2 + slice, g.rowoff};              // outward vectors: X_b (b < cs), Y_b (b >= cs) on bond b

    // ---- phase A: k_chain's walk and centre, every chain vector also to the tape (chain_common.h).  The coefficients of the tile go to cl. ----
    E p0[NCT], p1[NCT];
    int cur = chain_walk_taped<E, NCT, SRC>(ch, buf, tape, p0, p1, tile0, tid);
    E* const park = tape.bond(cs);                                     // R_{cs+1}
    bool bad = false;                                                  // fp32: a weight of the thread's image is Inf or NaN
    chain_centre_taped<E, NCT>(ch, buf, cur, park, p0, p1, tile0, tid, [&](int l, E w, int col, int img) {
        E cv = 0;
        if (img < ch.cnt) {
            if (Tr::bad(Tr::abs(w))) bad = true;
            if constexpr (LOSS == 1) {
                cv = w;                                                // parked: the softmax block below needs all ten
            } else if (g.lab) {                                        // formed in fp64 from the (widened) weight, rounded once to E
                const int lb = g.lab[img];
                const double y = (ch.single ? lb == g.target : lb == l) ? 1. : 0.;
                cv = (E)(2. * ((double)w - y));
                g.coef[(size_t)img * ch.nl + l] = cv;
            } else {
                cv = (E)g.coef[(size_t)img * ch.nl + l];
            }
        }
        cl[l * T + col] = cv;
    });
    if constexpr (f32) { if (bad) *ch.flag = 1; }
    if constexpr (LOSS == 1) {                                         // (the centre ends on a barrier; the one below orders this before seed_step)
        const int img = tile0 + tid;
        if (tid < T && img < ch.cnt) {
            double wv[TNML_NL];
#pragma unroll
            for (int l = 0; l < TNML_NL; ++l) wv[l] = cl[l * T + tid];
            int d;
            (void)loss_softmax(wv, g.lab[img], g.beta, &d);
#pragma unroll
            for (int l = 0; l < TNML_NL; ++l) { const E cv = (E)wv[l]; cl[l * T + tid] = cv; g.coef[(size_t)img * TNML_NL + l] = cv; }
        }
    }
    const ChainSite<E> sc = ch.sites[cs - 1];
    const size_t lstride = (size_t)sc.ml * 2 * sc.mr;
    chain_copy_rows<E, T>(park, buf[cur ^ 1], sc.mr, tid);                // R into the free tile: the operand of the right-type seed
    __syncthreads();

    // ---- centre: the seeds X_{cs-1} (second tape, bond cs-1) and Y_cs (bond cs) ----
    if (cs > 1) seed_step<E, NCT, false>(sc.a, lstride, ch.nl, sc.ml, sc.mr, buf[cur ^ 1], tape2.bond(cs - 1), p0, p1, cl, wave, lane);
    if (cs < N) seed_step<E, NCT, true>(sc.a, lstride, ch.nl, sc.ml, sc.mr, buf[cur], tape2.bond(cs), p0, p1, cl, wave, lane);

    // ---- phase B: X_{j-1} = (phi_j A_j) X_j, j = cs-1 .. 2, then Y_j = Y_{j-1} (phi_j A_j), j = cs+1 .. N-1 ----
    carry_outward<E, NCT, SRC, false>(ch, buf, tape2, sc.ml, p0, p1, tile0, tid);
    carry_outward<E, NCT, SRC, true>(ch, buf, tape2, sc.mr, p0, p1, tile0, tid);
}

// ---- the GEMM over the image index ----
template <typename E, int NCT, int SRC>
__global__ __launch_bounds__(SG_THREADS) void k_site_grad(const SiteGradArgsT<E> g) {
    typedef ChainT<E> Tr;
    constexpr bool f32 = sizeof(E) == sizeof(float);
    // row pitch of the staged operands (elements).  The MFMA loop reads element (16 w + c16) P + q + 4 t per lane: in fp32 a ds_read_b32
    // serves 32 lanes (c16 = 0..15, two q) over 32 banks, and P = 2 mod 32 puts them on 32 different banks
    constexpr int T = 16 * NCT, P = T + (f32 ? 2 : 4);
    __shared__ E sa[SG_BLK * P];                                       // a side [32][P]
    __shared__ E sr[2 * SG_BLK * P];                                   // r side [s][32][P], the feature multiplied in
    __shared__ E fs[2][2][T];                                          // [parity][s][image of the tile]: the feature / coefficient operand
    const ChainArgs<E>& ch = g.ch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, q = lane >> 4;
    const int N = ch.N, cs = ch.cs, nl = ch.nl, NV = N - 1 + nl;
    // the virtual site of this block: the last v with blk0[v] <= blockIdx.x
    int lo = 0, hi = NV;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (g.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid; }
    const int v = lo;
    int j, l = 0;
    if (v < cs - 1) j = v + 1; else if (v < cs - 1 + nl) { j = cs; l = v - (cs - 1); } else j = v - nl + 2;
    const ChainSite<E> st = ch.sites[j - 1];
    const int ml = st.ml, mr = st.mr;
    const int nrb = (mr + SG_BLK - 1) / SG_BLK;
    const int bi = (int)blockIdx.x - g.blk0[v];
    const int a0 = (bi / nrb) * SG_BLK, r0 = (bi % nrb) * SG_BLK;
    // a side on bond j-1: L_{j-1} (first tape) up to the centre, Y_{j-1} (second tape) right of it;
    // r side on bond j: X_j (second tape) left of the centre, R_{j+1} (first tape) from the centre on
    const size_t rows = g.rowoff[N + 1];
    const E* const abase = (j <= cs ? g.tape : g.tape2) + (size_t)g.rowoff[j - 1] * T;
    const E* const rbase = (j < cs ? g.tape2 : g.tape) + (size_t)g.rowoff[j] * T;
    const bool centre = j == cs;
    double* const G = g.grad + g.goff[j - 1] + (centre ? (size_t)l * ml * 2 * mr : 0);

    // this wave's output tile: rows of the MFMA = r (r0 + 16 wr + ..), columns = a (a0 + 16 wa + ..); accumulators from G (fp32: from 0)
    const int wa = wave & 1, wr = wave >> 1;
    const int oa = a0 + 16 * wa + c16;
    typename Tr::v4 acc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int orr = r0 + 16 * wr + Tr::rowq(q, reg);
            if constexpr (f32) acc[s][reg] = 0;
            else acc[s][reg] = (oa < ml && orr < mr) ? G[oa + (size_t)ml * (s + 2 * orr)] : 0.;
        }

    // the feature operand of a tile: phi_s of site j (x c_nl at the Label site), (0, 0) beyond the chunk
    auto features = [&](int tile, int par) {
        if (tid < T) {
            const int img = tile * T + tid;
            E f0[1], f1[1];
            chain_features<E, 1, SRC>(ch, j, img, f0, f1);
            if (centre) {                                              // (fp32: the buffer holds fp32 values widened, or given coefficients, rounded here)
                const E cv = img < ch.cnt ? (E)g.coef[(size_t)img * nl + l] : (E)0;
                f0[0] = cv * f0[0]; f1[0] = cv * f1[0];
            }
            fs[par][0][tid] = f0[0]; fs[par][1][tid] = f1[0];
        }
    };
    const int ntiles = (ch.cnt + T - 1) / T;                          // the tiles this launch's k_site_backward wrote, and no more
    features(0, 0);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int par = tile & 1;
        const E* const at = abase + (size_t)tile * rows * T;
        const E* const rt = rbase + (size_t)tile * rows * T;
        __syncthreads();                                               // the MFMAs of the tile before have read sa / sr; fs[par] is there
        // stage: thread -> (row, a pair of physical columns); where the tape keeps them: ChainT<E>::prow / lcol (fp64: odd rows have their
        // 16-column halves swapped for T >= 32)
        for (int e = tid; e < SG_BLK * (T / 2); e += SG_THREADS) {
            const int row = e / (T / 2), pc = (e - row * (T / 2)) * 2;
            const bool live = tile * T + T <= ch.cnt;                  // every image of the tile is inside the chunk
            {
                const int ar = a0 + row;
                const int col = Tr::template lcol<NCT>(ar, pc);
                typename Tr::v2 x = {0, 0};
                if (ar < ml) x = *(const typename Tr::v2*)(at + (size_t)Tr::template prow<NCT>(ar) * T + pc);
                if (!live) { if (tile * T + col >= ch.cnt) x.x = 0; if (tile * T + col + 1 >= ch.cnt) x.y = 0; }
                sa[row * P + col] = x.x; sa[row * P + col + 1] = x.y;
            }
            {
                const int rr = r0 + row;
                const int col = Tr::template lcol<NCT>(rr, pc);
                typename Tr::v2 x = {0, 0};
                if (rr < mr) x = *(const typename Tr::v2*)(rt + (size_t)Tr::template prow<NCT>(rr) * T + pc);
                E y00 = fs[par][0][col] * x.x, y01 = fs[par][0][col + 1] * x.y;
                E y10 = fs[par][1][col] * x.x, y11 = fs[par][1][col + 1] * x.y;
                if (!live) {                                           // the zero comes from the feature operand, as a select
                    if (tile * T + col >= ch.cnt) { y00 = 0; y10 = 0; }
                    if (tile * T + col + 1 >= ch.cnt) { y01 = 0; y11 = 0; }
                }
                sr[row * P + col] = y00; sr[row * P + col + 1] = y01;
                sr[(SG_BLK + row) * P + col] = y10; sr[(SG_BLK + row) * P + col + 1] = y11;
            }
        }
        if (tile + 1 < ntiles) features(tile + 1, par ^ 1);
        __syncthreads();
        const E* const pa = sa + (16 * wa + c16) * P + q;
        const E* const pr0 = sr + (16 * wr + c16) * P + q;
        const E* const pr1 = pr0 + SG_BLK * P;
#pragma unroll 4
        for (int t = 0; t < T / 4; ++t) {
            const E a = pa[4 * t];
            acc[0] = Tr::mfma(pr0[4 * t], a, acc[0]);
            acc[1] = Tr::mfma(pr1[4 * t], a, acc[1]);
        }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int orr = r0 + 16 * wr + Tr::rowq(q, reg);
            if constexpr (f32) {                                       // the chunk's fp32 sum joins the fp64 gradient: one addition
                if (oa < ml && orr < mr) G[oa + (size_t)ml * (s + 2 * orr)] = G[oa + (size_t)ml * (s + 2 * orr)] + (double)acc[s][reg];
            } else {
                if (oa < ml && orr < mr) G[oa + (size_t)ml * (s + 2 * orr)] = acc[s][reg];
            }
        }
}

// a.ch.mcap and the grids follow from T; rows: a.rowoff[N + 1] as the host knows it; tape_elems: elements behind each of the two tapes;
// nblocks: a.blk0[N - 1 + nl] as the host knows it
// run_gemm false: k_site_backward alone (tnml_backward_* without grad)
template <typename E>
int launch_site_gradient(tnml_ctx* c, SiteGradArgsT<E> a, int maxbond, int T, int rows, size_t tape_elems, int nblocks, bool run_gemm) {
    constexpr bool f32 = sizeof(E) == sizeof(float);
    if (nblocks < 1) return tnml_fail(c, "site gradient kernel: %d output blocks", nblocks);
    if (f32 && !a.ch.flag) return tnml_fail(c, "site gradient kernel: no range flag");
    typedef void (*kern_t)(const SiteGradArgsT<E>);
    static const kern_t bwd[2][3] = {{k_site_backward<E, 1, 0>, k_site_backward<E, 2, 0>, k_site_backward<E, 4, 0>}, {k_site_backward<E, 1, 1>, k_site_backward<E, 2, 1>, k_site_backward<E, 4, 1>}};   // [SRC][T / 32]
    static const kern_t gemm[2][3] = {{k_site_grad<E, 1, 0>, k_site_grad<E, 2, 0>, k_site_grad<E, 4, 0>}, {k_site_grad<E, 1, 1>, k_site_grad<E, 2, 1>, k_site_grad<E, 4, 1>}};
    static const kern_t bwd_sm[2][3] = {{k_site_backward<E, 1, 0, 1>, k_site_backward<E, 2, 0, 1>, k_site_backward<E, 4, 0, 1>}, {k_site_backward<E, 1, 1, 1>, k_site_backward<E, 2, 1, 1>, k_site_backward<E, 4, 1, 1>}};
    const bool softmax = a.loss == TNML_LOSS_SOFTMAX;                  // (the host sets it in the labels mode only)
    if (softmax && (!a.lab || a.ch.single || a.ch.nl != TNML_NL)) return tnml_fail(c, "site gradient kernel: the softmax loss needs labels and %d outputs", TNML_NL);
    TapedLaunch L;                                                     // beside the two tiles: the coefficients [nl][T]
    TCK(taped_launch(c, "site gradient kernel", "tapes", a.ch, maxbond, T, rows, tape_elems, (size_t)a.ch.nl * T * sizeof(E), softmax ? bwd_sm : bwd,
                     softmax ? c->attr_sitegrad_sm[f32] : c->attr_sitegrad[f32], &L));
    {
        ProfScope ps(c, KC_SITE_BWD);
        hipLaunchKernelGGL((softmax ? bwd_sm : bwd)[L.codes][T / 32], dim3(L.grid), dim3(CHAIN_THREADS), L.lds, c->stream, a);
        HIPCK(c, hipGetLastError());
    }
    if (!run_gemm) return 0;
    ProfScope ps(c, KC_SITE_GRAD);
    hipLaunchKernelGGL(gemm[L.codes][T / 32], dim3(nblocks), dim3(SG_THREADS), 0, c->stream, a);
    HIPCK(c, hipGetLastError());
    return 0;
}
template int launch_site_gradient<double>(tnml_ctx*, SiteGradArgsT<double>, int, int, int, size_t, int, bool);
template int launch_site_gradient<float>(tnml_ctx*, SiteGradArgsT<float>, int, int, int, size_t, int, bool);

// ---- the forward that keeps its tape, and the backward that starts from it (tnml_forward_taped_* / tnml_backward_taped*) ----
// k_forward_taped is phase A of k_site_backward and nothing else: the taped inward walk and the centre, so weights, pred and the inward tape
// are those k_site_backward leaves, bit for bit; the hook keeps the fp32 range check alone.  Two tiles of LDS, no coefficients.
template <typename E, int NCT, int SRC>
__global__ __launch_bounds__(CHAIN_THREADS) void k_forward_taped(const SiteGradArgsT<E> g) {
    typedef ChainT<E> Tr;
    constexpr bool f32 = sizeof(E) == sizeof(float);
    constexpr int T = 16 * NCT;
    extern __shared__ __attribute__((aligned(16))) unsigned char sg_lds_raw[];
    E* const lds = reinterpret_cast<E*>(sg_lds_raw);
    const ChainArgs<E>& ch = g.ch;
    const int tid = threadIdx.x;
    const int tile0 = blockIdx.x * T;
    const size_t tile_elems = (size_t)ch.mcap * T;
    E* buf[2] = {lds, lds + tile_elems};
    const size_t slice = (size_t)blockIdx.x * g.rowoff[ch.N + 1] * T;
    const ChainTape<E, T> tape{g.tape + slice, g.rowoff};
    E p0[NCT], p1[NCT];
    const int cur = chain_walk_taped<E, NCT, SRC>(ch, buf, tape, p0, p1, tile0, tid);
    bool bad = false;
    chain_centre_taped<E, NCT>(ch, buf, cur, tape.bond(ch.cs), p0, p1, tile0, tid, [&](int, E w, int, int img) {
        if (img < ch.cnt && Tr::bad(Tr::abs(w))) bad = true;
    });
    if constexpr (f32) { if (bad) *ch.flag = 1; }
}

// k_site_outward: the centre's seeds and phase B of k_site_backward in its coef mode, from the inward tape of a k_forward_taped launch with
// the same tile width.  Grid (tiles, 2): the two outward walks share nothing but the tile's coefficients and the centre's features, so
// workgroup y = 0 seeds and carries X (left of the Label site), y = 1 seeds and carries Y (right of it), with seed_step and
// carry_outward as they are -- the operands of a seed are the tape's copies of R_{cs+1} (bond cs) and L_{cs-1} (bond cs-1; the 1 of a
// chain's start when cs = 1), the very values k_site_backward has in its tiles, so the second tape comes out bit for bit.  A side with
// nothing to do returns at once.  LDS as k_site_backward: two tiles and the coefficients [nl][T].
template <typename E, int NCT, int SRC>
__global__ __launch_bounds__(CHAIN_THREADS) void k_site_outward(const SiteGradArgsT<E> g) {
    constexpr int T = 16 * NCT;
    extern __shared__ __attribute__((aligned(16))) unsigned char sg_lds_raw[];
    E* const lds = reinterpret_cast<E*>(sg_lds_raw);
    const ChainArgs<E>& ch = g.ch;
    const int N = ch.N, cs = ch.cs;
    const bool right = blockIdx.y == 1;
    if (right ? cs >= N : cs <= 1) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile0 = blockIdx.x * T;
    const size_t tile_elems = (size_t)ch.mcap * T;
    E* buf[2] = {lds, lds + tile_elems};
    E* const cl = lds + 2 * tile_elems;                                // [nl][T] coefficients of the tile
    const size_t slice = (size_t)blockIdx.x * g.rowoff[N + 1] * T;
    const ChainTape<E, T> tape{g.tape + slice, g.rowoff};
    const ChainTape<E, T> tape2{g.tape2 + slice, g.rowoff};
    if (tid < T) {                                                     // the coef branch of k_site_backward's hook: rounded once to E, 0 beyond the chunk
        const int img = tile0 + tid;
        for (int l = 0; l < ch.nl; ++l) cl[l * T + tid] = img < ch.cnt ? (E)g.coef[(size_t)img * ch.nl + l] : (E)0;
    }
    E p0[NCT], p1[NCT];
    chain_features<E, NCT, SRC>(ch, cs, tile0 + (lane & 15), p0, p1);
    const ChainSite<E> sc = ch.sites[cs - 1];
    const size_t lstride = (size_t)sc.ml * 2 * sc.mr;
    if (right) {
        chain_copy_rows<E, T>(tape.bond(cs - 1), buf[0], sc.ml, tid);  // L_{cs-1}
        __syncthreads();
        seed_step<E, NCT, true>(sc.a, lstride, ch.nl, sc.ml, sc.mr, buf[0], tape2.bond(cs), p0, p1, cl, wave, lane);
        carry_outward<E, NCT, SRC, true>(ch, buf, tape2, sc.mr, p0, p1, tile0, tid);
    } else {
        chain_copy_rows<E, T>(tape.bond(cs), buf[0], sc.mr, tid);      // R_{cs+1}
        __syncthreads();
        seed_step<E, NCT, false>(sc.a, lstride, ch.nl, sc.ml, sc.mr, buf[0], tape2.bond(cs - 1), p0, p1, cl, wave, lane);
        carry_outward<E, NCT, SRC, false>(ch, buf, tape2, sc.ml, p0, p1, tile0, tid);
    }
}

template <typename E>
int launch_forward_taped(tnml_ctx* c, SiteGradArgsT<E> a, int maxbond, int T, int rows, size_t tape_elems) {
    constexpr bool f32 = sizeof(E) == sizeof(float);
    if (f32 && !a.ch.flag) return tnml_fail(c, "taped forward kernel: no range flag");
    typedef void (*kern_t)(const SiteGradArgsT<E>);
    static const kern_t fwd[2][3] = {{k_forward_taped<E, 1, 0>, k_forward_taped<E, 2, 0>, k_forward_taped<E, 4, 0>}, {k_forward_taped<E, 1, 1>, k_forward_taped<E, 2, 1>, k_forward_taped<E, 4, 1>}};   // [SRC][T / 32]
    TapedLaunch L;
    TCK(taped_launch(c, "taped forward kernel", "tape", a.ch, maxbond, T, rows, tape_elems, 0, fwd, c->attr_fwdtaped[f32], &L));
    ProfScope ps(c, KC_FWD_TAPED);
    hipLaunchKernelGGL(fwd[L.codes][T / 32], dim3(L.grid), dim3(CHAIN_THREADS), L.lds, c->stream, a);
    HIPCK(c, hipGetLastError());
    return 0;
}
template int launch_forward_taped<double>(tnml_ctx*, SiteGradArgsT<double>, int, int, int, size_t);
template int launch_forward_taped<float>(tnml_ctx*, SiteGradArgsT<float>, int, int, int, size_t);

template <typename E>
int launch_site_outward(tnml_ctx* c, SiteGradArgsT<E> a, int maxbond, int T, int rows, size_t tape_elems, int nblocks, bool run_gemm) {
    constexpr bool f32 = sizeof(E) == sizeof(float);
    if (nblocks < 1) return tnml_fail(c, "outward kernel: %d output blocks", nblocks);
    if (!a.coef || !a.tape || !a.tape2) return tnml_fail(c, "outward kernel: null argument");
    typedef void (*kern_t)(const SiteGradArgsT<E>);
    static const kern_t out[2][3] = {{k_site_outward<E, 1, 0>, k_site_outward<E, 2, 0>, k_site_outward<E, 4, 0>}, {k_site_outward<E, 1, 1>, k_site_outward<E, 2, 1>, k_site_outward<E, 4, 1>}};   // [SRC][T / 32]
    static const kern_t gemm[2][3] = {{k_site_grad<E, 1, 0>, k_site_grad<E, 2, 0>, k_site_grad<E, 4, 0>}, {k_site_grad<E, 1, 1>, k_site_grad<E, 2, 1>, k_site_grad<E, 4, 1>}};
    TapedLaunch L;
    TCK(taped_launch(c, "outward kernel", "tapes", a.ch, maxbond, T, rows, tape_elems, (size_t)a.ch.nl * T * sizeof(E), out, c->attr_siteout[f32], &L));
    {
        ProfScope ps(c, KC_SITE_OUT);
        hipLaunchKernelGGL(out[L.codes][T / 32], dim3(L.grid, 2), dim3(CHAIN_THREADS), L.lds, c->stream, a);
        HIPCK(c, hipGetLastError());
    }
    if (!run_gemm) return 0;
    ProfScope ps(c, KC_SITE_GRAD);
    hipLaunchKernelGGL(gemm[L.codes][T / 32], dim3(nblocks), dim3(SG_THREADS), 0, c->stream, a);
    HIPCK(c, hipGetLastError());
    return 0;
}
template int launch_site_outward<double>(tnml_ctx*, SiteGradArgsT<double>, int, int, int, size_t, int, bool);
template int launch_site_outward<float>(tnml_ctx*, SiteGradArgsT<float>, int, int, int, size_t, int, bool);
