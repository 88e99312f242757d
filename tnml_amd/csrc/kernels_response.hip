// kernels_response.hip -- streamed site responses (tnml_response_u8 / tnml_response_phi): for a tile of T images and the label l_n of
// every image, in ONE launch,
//
//   resp[j][s][n] = the contraction of W with label index l_n and the features of image n on every site except j, site j getting e_s
//
// so that W_{l_n}(image n with site j's feature replaced by psi) = psi_0 resp[j][0][n] + psi_1 resp[j][1][n] for every psi.
//
// One workgroup (8 waves) owns one tile, as in k_chain (kernels_chain.hip; the fragment maps, the k blocks, the masking and the tile
// thresholds are those of that kernel, the shared code is chain_common.h), and walks the chain twice.
//
// Phase A is the taped inward walk and the centre of chain_common.h (chain_walk_taped, chain_centre_taped; their order is stated
// there): k_chain's walk, so that weights and pred are bit for bit those of k_chain<double>, with every chain vector also written to
// the workgroup's slice of a global tape (ChainTape); the slice is written once and read once, by this workgroup only.
//
// Centre.  l_n = which[n], or pred[n] when which is null.  For every label l that some image of the tile has chosen, the columns of
// those images take
//   U_s[r] = sum_a A_c[a,s,r,l] L[a]        (left-type product, s = 0, 1 apart)   resp[c][s] = sum_r R[r] U_s[r],  Y = phi_0 U_0 + phi_1 U_1
//   U'_s[a] = sum_r A_c[a,s,r,l] R[r]       (right-type product)                  X = phi_0 U'_0 + phi_1 U'_1
// X and Y start the outward walks; they wait in two further regions of the tape.
//
// Phase B, outward from the centre, X resp. Y resident in LDS:
//   j = c-1 .. 1:   U_s[a] = sum_r A_j[a,s,r] X[r];   resp[j][s] = sum_a L_{j-1}[a] U_s[a];   X <- phi_0 U_0 + phi_1 U_1
//   j = c+1 .. N:   U_s[r] = sum_a A_j[a,s,r] Y[a];   resp[j][s] = sum_r R_{j+1}[r] U_s[r];   Y <- phi_0 U_0 + phi_1 U_1
// with L_{j-1}, R_{j+1} from the tape.  The two products of a site are the MFMA count of one chain step.
//
// Arithmetic (fp64, the file is compiled with -ffp-contract=off; per image independent of n, chunk, tile width and tile position):
//   * U_s: v_mfma_f64_16x16x4_f64 over the 16-wide k blocks of the contraction index in ascending order, lane (row, q) holding
//     k = base + 4 q + i and MFMA step i multiplying element i -- the k order of chain_step restricted to one s;
//   * X, Y: fl(fl(phi_0 U_0) + fl(phi_1 U_1));
//   * resp[j][s][n], the dot over the output index of U_s, in this fixed order:
//       1. inside a wave's 16-row tile, a lane's four rows (MFMA C/D registers 0..3, rows q + 4 reg): v = fma(E[row], U[row], v) from 0;
//       2. the four q groups of the tile: ((v_0 + v_1) + v_2) + v_3;
//       3. the row tiles of a wave (rt = wave, wave + 8, ..) ascending, added to the wave's sum from 0;
//       4. the eight wave sums through an LDS block, added in wave order from 0.
//     No atomics.  Rows beyond the bond dimension contribute nothing (never read).
//
// LDS: two chain tiles [mcap][T] doubles, the block of wave sums [2][8][2][T] doubles (two parities, so that one __syncthreads() per site
// suffices) and T + 1 ints for l_n and the set of chosen labels: k_chain's tile thresholds carry over (128 KiB + 16.3 KiB <= 160 KiB).
#include "chain_common.h"

// U_0, U_1 of one site (see the header) for the row tiles of this wave; vin is an LDS tile, ev (the environment of the dot) a region of
// the tape, vout an LDS tile or a region of the tape.  Columns whose lsel differs from l are neither stored nor (by the caller) summed;
// lsel null: every column.  red: this step's block of wave sums [8][2][T].
template <int NCT, bool LEFT>
static __device__ __forceinline__ void resp_step(const double* __restrict__ A, int ml, int mr, const double* vin, const double* __restrict__ ev, double* vout,
                                                 const double (&p0)[NCT], const double (&p1)[NCT], const int* lsel, int l, double* red, int wave, int lane) {
    typedef ChainT<double> Tr;
    constexpr int T = 16 * NCT;
    const int c16 = lane & 15, q = lane >> 4;
    const int K = LEFT ? ml : mr, M = LEFT ? mr : ml;
    const int nrt = (M + 15) >> 4;
    bool sel[NCT];
    double dsum[2][NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) { sel[ct] = !lsel || lsel[16 * ct + c16] == l; dsum[0][ct] = dsum[1][ct] = 0; }
    for (int rt = wave; rt < nrt; rt += CHAIN_WAVES) {
        const int orow = rt * 16 + c16;         // the A fragment's row of this lane
        const bool rok = orow < M;
        Tr::v4 acc0[NCT], acc1[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) { acc0[ct] = Tr::v4{0, 0, 0, 0}; acc1[ct] = Tr::v4{0, 0, 0, 0}; }
        // element (k, s) of output row orow: left-type A[a = k][s][r = orow], right-type A[a = orow][s][r = k] ([ml][2][mr], first index fastest)
        const double* const Ar = LEFT ? A + (size_t)2 * ml * orow : A + orow;
        // (the next block's values and the dot's environment loaded ahead, as chain_step does, cost 56 to 64 VGPRs and gained nothing:
        // 22.37 against 22.33 ms for 256 images at N = 784, m = 120)
        for (int base = 0; base < K; base += 16) {
            double a0[4], a1[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = base + 4 * q + i;
                a0[i] = a1[i] = 0;
                if (rok && k < K) {
                    if (LEFT) { a0[i] = Ar[k]; a1[i] = Ar[ml + k]; }
                    else      { a0[i] = Ar[(size_t)ml * (2 * k)]; a1[i] = Ar[(size_t)ml * (2 * k + 1)]; }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = base + 4 * q + i;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    double b = 0;
                    if (k < K) b = vin[Tr::template idx<NCT>(k, 16 * ct + c16)];
                    acc0[ct] = Tr::mfma(a0[i], b, acc0[ct]);
                    acc1[ct] = Tr::mfma(a1[i], b, acc1[ct]);
                }
            }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            double v0 = 0, v1 = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = Tr::row(rt, q, r);
                if (row < M) {
                    const int at = Tr::template idx<NCT>(row, 16 * ct + c16);
                    const double e = ev[at], u0 = acc0[ct][r], u1 = acc1[ct][r];
                    v0 = Tr::fma(e, u0, v0); v1 = Tr::fma(e, u1, v1);
                    if (sel[ct]) vout[at] = p0[ct] * u0 + p1[ct] * u1;
                }
            }
            // the four q groups in order: every lane forms the same sum
            const double t0 = ((__shfl(v0, c16) + __shfl(v0, c16 + 16)) + __shfl(v0, c16 + 32)) + __shfl(v0, c16 + 48);
            const double t1 = ((__shfl(v1, c16) + __shfl(v1, c16 + 16)) + __shfl(v1, c16 + 32)) + __shfl(v1, c16 + 48);
            dsum[0][ct] += t0; dsum[1][ct] += t1;
        }
    }
    if (q == 0) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            red[(wave * 2 + 0) * T + 16 * ct + c16] = dsum[0][ct];
            red[(wave * 2 + 1) * T + 16 * ct + c16] = dsum[1][ct];
        }
    }
}

template <int NCT, int SRC>
__global__ __launch_bounds__(CHAIN_THREADS) void k_response(const RespArgs g) {
    constexpr int T = 16 * NCT;
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds_raw[];
    double* const lds = reinterpret_cast<double*>(rs_lds_raw);
    const ChainArgs<double>& ch = g.ch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile0 = blockIdx.x * T;
    const size_t tile_elems = (size_t)ch.mcap * T;
    double* buf[2] = {lds, lds + tile_elems};
    double* const redb = lds + 2 * tile_elems;                         // [2][CHAIN_WAVES][2][T]
    int* const lsel = reinterpret_cast<int*>(redb + 2 * CHAIN_WAVES * 2 * T);     // [T], then the set of chosen labels
    int* const lmask = lsel + T;
    const int N = ch.N, cs = ch.cs;
    // the inward tape of this workgroup (chain_common.h), then X and Y of the centre at rowoff[N + 1], rowoff[N + 2]
    const ChainTape<double, T> tape{g.tape + (size_t)blockIdx.x * g.rowoff[N + 3] * T, g.rowoff};
    // the block of wave sums of the step before -> resp[j][s] of the columns that chose l (lsel null: all)
    auto finish = [&](const double* red, int j, bool all, int l) {
        if (tid < 2 * T) {
            const int s = tid / T, col = tid - s * T, img = tile0 + col;
            if (img < ch.cnt && (all || lsel[col] == l)) {
                double sum = 0;
                for (int w = 0; w < CHAIN_WAVES; ++w) sum += red[(w * 2 + s) * T + col];
                g.resp[((size_t)(j - 1) * 2 + s) * ch.ld + img] = sum;
            }
        }
    };

    // ---- phase A: k_chain's walk and centre, every chain vector also to the tape (chain_common.h) ----
    double p0[NCT], p1[NCT], q0[NCT], q1[NCT];
    const int img0 = tile0 + (lane & 15), img = tile0 + tid;
    if (tid == 0) *lmask = 0;                                          // (ahead of the walk: behind it the kernel measured 0.6 % slower)
    int cur = chain_walk_taped<double, NCT, SRC>(ch, buf, tape, p0, p1, tile0, tid);
    double* const park = tape.bond(cs);                                // R_{cs+1}
    const int pr = chain_centre_taped<double, NCT>(ch, buf, cur, park, p0, p1, tile0, tid, [](int, double, int, int) {});
    const ChainSite<double> sc = ch.sites[cs - 1];
    const size_t lstride = (size_t)sc.ml * 2 * sc.mr;
    if (tid < T) {
        int ln = -1;
        if (img < ch.cnt) {
            ln = ch.single ? 0 : (g.which ? g.which[img] : pr);
            atomicOr(lmask, 1 << ln);                                  // an LDS integer
        }
        lsel[tid] = ln;
    }
    chain_copy_rows<double, T>(park, buf[cur ^ 1], sc.mr, tid);                // R into the free tile: the operand of the right-type product
    __syncthreads();
    const int mask = *lmask;
    if (tid < T && lsel[tid] < 0) lsel[tid] = __ffs(mask) - 1;         // columns beyond the chunk (all zero) ride with the first chosen label
    __syncthreads();

    // ---- centre: per chosen label, resp[cs] and the starting vectors X (tape region N + 1) and Y (N + 2) ----
    int par = 0;
    for (int l = 0; l < ch.nl; ++l) {
        if (!((mask >> l) & 1)) continue;
        double* const red = redb + (size_t)par * CHAIN_WAVES * 2 * T;
        resp_step<NCT, true>(sc.a + l * lstride, sc.ml, sc.mr, buf[cur], park, tape.bond(N + 2), p0, p1, lsel, l, red, wave, lane);
        __syncthreads();
        finish(red, cs, false, l);
        par ^= 1;
        if (cs > 1) {                                                  // (its dot with L would give resp[cs] once more: not stored)
            resp_step<NCT, false>(sc.a + l * lstride, sc.ml, sc.mr, buf[cur ^ 1], tape.bond(cs - 1), tape.bond(N + 1), p0, p1, lsel, l, redb + (size_t)par * CHAIN_WAVES * 2 * T, wave, lane);
            __syncthreads();
            par ^= 1;
        }
    }

    // ---- phase B, left of the centre: j = cs-1 .. 1 ----
    if (cs > 1) {
        chain_copy_rows<double, T>(tape.bond(N + 1), buf[0], sc.ml, tid);
        chain_features<double, NCT, SRC>(ch, cs - 1, img0, p0, p1);
        __syncthreads();
        cur = 0;
        for (int j = cs - 1; j >= 1; --j) {
            if (j > 1) chain_features<double, NCT, SRC>(ch, j - 1, img0, q0, q1);
            const ChainSite<double> st = ch.sites[j - 1];
            double* const red = redb + (size_t)par * CHAIN_WAVES * 2 * T;
            resp_step<NCT, false>(st.a, st.ml, st.mr, buf[cur], tape.bond(j - 1), buf[cur ^ 1], p0, p1, nullptr, 0, red, wave, lane);
            __syncthreads();
            finish(red, j, true, 0);
            par ^= 1; cur ^= 1;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) { p0[ct] = q0[ct]; p1[ct] = q1[ct]; }
        }
    }
    // ---- phase B, right of the centre: j = cs+1 .. N ----
    if (cs < N) {
        __syncthreads();                                               // the tiles are free: every wave has left the loop above
        chain_copy_rows<double, T>(tape.bond(N + 2), buf[0], sc.mr, tid);
        chain_features<double, NCT, SRC>(ch, cs + 1, img0, p0, p1);
        __syncthreads();
        cur = 0;
        for (int j = cs + 1; j <= N; ++j) {
            if (j < N) chain_features<double, NCT, SRC>(ch, j + 1, img0, q0, q1);
            const ChainSite<double> st = ch.sites[j - 1];
            double* const red = redb + (size_t)par * CHAIN_WAVES * 2 * T;
            resp_step<NCT, true>(st.a, st.ml, st.mr, buf[cur], tape.bond(j), buf[cur ^ 1], p0, p1, nullptr, 0, red, wave, lane);
            __syncthreads();
            finish(red, j, true, 0);
            par ^= 1; cur ^= 1;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) { p0[ct] = q0[ct]; p1[ct] = q1[ct]; }
        }
    }
}

// the staged result [2 N][ld] (images fastest) -> [cnt][2 N]: 32 x 32 tiles through LDS, both sides in whole lines
template <typename D>                                                  // D: double, or float (the result rounded once: dphi32 of a device-resident call)
__global__ __launch_bounds__(256) void k_response_transpose(const double* __restrict__ in, int rows, int cnt, int ld, D* __restrict__ out) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int n0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < rows && n0 + tx < cnt) tile[i][tx] = in[(size_t)(r0 + i) * ld + n0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (n0 + i < cnt && r0 + tx < rows) out[(size_t)(n0 + i) * rows + r0 + tx] = (D)tile[tx][i];
}

int launch_response_transpose(tnml_ctx* c, const double* in, int rows, int cnt, int ld, double* out, float* out32) {
    const dim3 grid((cnt + 31) / 32, (rows + 31) / 32);
    if (out) hipLaunchKernelGGL(k_response_transpose<double>, grid, dim3(256), 0, c->stream, in, rows, cnt, ld, out);
    else     hipLaunchKernelGGL(k_response_transpose<float>, grid, dim3(256), 0, c->stream, in, rows, cnt, ld, out32);
    HIPCK(c, hipGetLastError());
    return 0;
}

// a.ch.mcap and the grid follow from T; rows: the rows of a workgroup's slice (a.rowoff[N + 3] on the device) as the host knows them
int launch_response(tnml_ctx* c, RespArgs a, int maxbond, int T, int rows, size_t tape_elems, double* outT) {
    typedef void (*kern_t)(const RespArgs);
    static const kern_t kern[2][3] = {{k_response<1, 0>, k_response<2, 0>, k_response<4, 0>}, {k_response<1, 1>, k_response<2, 1>, k_response<4, 1>}};   // [SRC][T / 32]
    TapedLaunch L;                                                     // beside the two tiles: the wave sums [2][8][2][T], l_n [T] and the set of chosen labels
    TCK(taped_launch(c, "response kernel", "tape", a.ch, maxbond, T, rows, tape_elems, (size_t)2 * CHAIN_WAVES * 2 * T * sizeof(double) + (size_t)(T + 1) * sizeof(int), kern, c->attr_response, &L));
    ProfScope ps(c, KC_SITE_RESP);
    hipLaunchKernelGGL(kern[L.codes][T / 32], dim3(L.grid), dim3(CHAIN_THREADS), L.lds, c->stream, a);
    HIPCK(c, hipGetLastError());
    return launch_response_transpose(c, a.resp, 2 * a.ch.N, a.ch.cnt, a.ch.ld, outT);
}
