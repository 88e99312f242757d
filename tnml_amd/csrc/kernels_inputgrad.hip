// kernels_inputgrad.hip -- streamed input gradients (tnml_backward_u8 / tnml_backward_phi): for a chunk of images and coefficients
// c[n][l] = dC/dW_l(x_n), the gradient of C with respect to the features of every site,
//
//   j < c:   dphi[n][j][s] = sum_a L_{j-1,n}[a] sum_r A_j[a,s,r]   X_{j,n}[r]
//   j > c:   dphi[n][j][s] = sum_a Y_{j-1,n}[a] sum_r A_j[a,s,r]   R_{j+1,n}[r]
//   j = c:   dphi[n][c][s] = sum_l c_nl sum_a L_{c-1,n}[a] sum_r A_c[a,s,r,l] R_{c+1,n}[r]
//
// L, R, X, Y are the inward and outward chain vectors that k_site_backward (kernels_sitegrad.hip) leaves on its two tapes; c is the Label
// site (site 1 in the per-label variant).  W is linear in the feature of each site, so this is the whole vector-Jacobian product.
//
// k_input_grad (class input_grad): ONE launch per chunk behind k_site_backward on the same stream.  The grid runs over (tile of T images,
// site j), the tile being the fast index so that the workgroups that read the same A_j run together; T is the tile width k_site_backward
// ran the chunk with, since a tape slice is [tile][rows][T].  It reads the two tapes, the site table and, at the Label site, coef[C][nl];
// it reads no features.  A workgroup of 8 waves stages the r-side vector Z (X_j, or R_{j+1} from the Label site on) into LDS in the tape's
// own element order (ChainT<double>::idx: for T >= 32 the 16-column halves of odd rows are swapped) and then works as one step of
// k_response's outward walk does:
//   * P_s = A_j[:,s,:] Z for s = 0, 1: v_mfma_f64_16x16x4_f64, output ml x T in 16-row tiles (tile rt of wave rt mod 8), the fragment
//     maps of ChainT<double>: lane (c16, q) holds A of row 16 rt + c16 and, of Z, column 16 ct + c16; MFMA step i of a 16-wide k block
//     multiplies r = base + 4 q + i.  At the Label site the Z operand of label l is fl(c_nl R[r]), formed on the fly, and the labels
//     are accumulated into the same tile with l ascending, as seed_step does.
//   * the dot with the a-side vector E (L_{j-1} up to the Label site, Y_{j-1} right of it), read from the tape.
// Bonds 0 and N hold 1 in every column of the inward tape (chain_walk_taped writes it).
//
// Summation order, fixed (fp64, the file is compiled with -ffp-contract=off; no atomics):
//   1. inside a 16-row tile the k blocks ascending, at the Label site label after label, l ascending, into the same accumulators;
//   2. the dot over a: a lane's accumulator rows ascending (C/D registers 0..3, rows 16 rt + q + 4 reg), v = fma(E[row], P[row], v) from
//      0, carried on over the wave's row tiles rt = wave, wave + 8, .. ascending;
//   3. the four lane groups q of the wave: ((v_0 + v_1) + v_2) + v_3;
//   4. the eight wave sums through an LDS block, added in wave order from 0.
// Every step is per column: an image's values do not depend on n, the chunk, the tile width or the tile it lands in, and repeats are
// bit-identical.  Columns beyond the chunk are not stored; rows beyond a bond are neither read nor multiplied with anything but the
// zeros that pad a k block.
//
// LDS: Z [ru16(largest bond)][T] doubles and the wave sums [8][2][T] doubles.  k_chain's tile thresholds (T = 64 up to bond 128, 32 up to
// 256, 16 up to 512) keep Z at 64 KiB, the sums at most 8 KiB: 72 KiB, so that two workgroups are resident per CU (160 KiB) at every
// bond dimension, bond 120 included (there: 128 x 64 x 8 = 64 KiB + 8 KiB).
// Registers: 74 / 98 / 148 VGPRs at T = 16 / 32 / 64, no scratch.  At T = 64 it is therefore the registers, not the LDS, that hold a CU to
// one workgroup (3 waves per SIMD where two workgroups need 4); a cap of 128 registers spills 28 of them and was not taken.
// The kernel leaves [N][2][C] (images fastest); k_response_transpose turns it into [C][N][2] as the caller gets it.
//
// Element type.  The kernel is written once over E: double (option gradient_dtype = 0, everything above) and float (gradient_dtype = 1).
// k_input_grad<float> reads the fp32 copy of W and the float tapes of k_site_backward<float> and takes ChainT<float> for the MFMA
// (v_mfma_f32_16x16x4_f32), the C/D map (rows 16 rt + 4 q + reg), the element order of Z and the tapes (ChainT<float>::idx) and the tile
// thresholds (64 up to bond 256, 32 up to 512, 16 up to 1 024: Z stays at 64 KiB).  At the Label site the Z operand is
// fl32(fl32(c_nl) R[r]).  The four steps above run in fp32 in the same order (step 1 is one fmaf chain per element, see kernels_chain.hip;
// steps 2 to 4 are fmaf and fp32 additions); dphi receives the fp32 result widened exactly, so dphi32 is rounded no second time.
// Registers of k_input_grad<float>: 58 / 70 / 116 VGPRs at T = 16 / 32 / 64, no scratch (8 / 7 / 4 waves per SIMD).
#include "chain_common.h"

template <typename E, int NCT>
__global__ __launch_bounds__(CHAIN_THREADS) void k_input_grad(const InputGradArgsT<E> g) {
    typedef ChainT<E> Tr;
    constexpr int T = 16 * NCT;
    extern __shared__ __attribute__((aligned(16))) unsigned char ig_lds_raw[];
    E* const z = reinterpret_cast<E*>(ig_lds_raw);                     // [mcap][T] the r-side vector, tape order
    E* const red = z + (size_t)g.mcap * T;                             // [CHAIN_WAVES][2][T] wave sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, q = lane >> 4;
    const int N = g.N, cs = g.cs, nl = g.nl;
    const int tile0 = blockIdx.x * T, j = (int)blockIdx.y + 1;
    const ChainSite<E> st = g.sites[j - 1];
    const int ml = st.ml, mr = st.mr;
    const bool centre = j == cs;
    const int nlab = centre ? nl : 1;
    const size_t lstride = (size_t)ml * 2 * mr;
    // a side on bond j-1: L_{j-1} (first tape) up to the centre, Y_{j-1} (second tape) right of it;
    // r side on bond j: X_j (second tape) left of the centre, R_{j+1} (first tape) from the centre on
    const size_t slice = (size_t)blockIdx.x * g.rowoff[N + 1] * T;
    const E* const ev = (j <= cs ? g.tape : g.tape2) + slice + (size_t)g.rowoff[j - 1] * T;
    const E* const zr = (j < cs ? g.tape2 : g.tape) + slice + (size_t)g.rowoff[j] * T;
    for (int i = tid; i < Tr::template span<NCT>(mr) * T; i += CHAIN_THREADS) z[i] = zr[i];     // (rows < mr are the first span(mr) stored rows: chain_common.h)
    __syncthreads();

    const int nrt = (ml + 15) >> 4;
    E v0[NCT], v1[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) v0[ct] = v1[ct] = 0;
    for (int rt = wave; rt < nrt; rt += CHAIN_WAVES) {
        const int orow = rt * 16 + c16;                                 // the A fragment's row of this lane
        const bool rok = orow < ml;
        typename Tr::v4 acc0[NCT], acc1[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) { acc0[ct] = typename Tr::v4{0, 0, 0, 0}; acc1[ct] = typename Tr::v4{0, 0, 0, 0}; }
        for (int l = 0; l < nlab; ++l) {
            E cv[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int img = tile0 + 16 * ct + c16;
                cv[ct] = (centre && img < g.cnt) ? (E)g.coef[(size_t)img * nl + l] : (E)0;
            }
            // element (k, s) of output row orow: A[a = orow][s][r = k] ([ml][2][mr], first index fastest)
            const E* const Ar = st.a + (size_t)l * lstride + orow;
            for (int base = 0; base < mr; base += 16) {
                E a0[4], a1[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = base + 4 * q + i;
                    a0[i] = a1[i] = 0;
                    if (rok && k < mr) { a0[i] = Ar[(size_t)ml * (2 * k)]; a1[i] = Ar[(size_t)ml * (2 * k + 1)]; }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = base + 4 * q + i;
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        E b = 0;
                        if (k < mr) {
                            b = z[Tr::template idx<NCT>(k, 16 * ct + c16)];
                            if (centre) b = cv[ct] * b;
                        }
                        acc0[ct] = Tr::mfma(a0[i], b, acc0[ct]);
                        acc1[ct] = Tr::mfma(a1[i], b, acc1[ct]);
                    }
                }
            }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = Tr::row(rt, q, r);
                if (row < ml) {
                    const E e = ev[Tr::template idx<NCT>(row, 16 * ct + c16)];
                    v0[ct] = Tr::fma(e, acc0[ct][r], v0[ct]);
                    v1[ct] = Tr::fma(e, acc1[ct][r], v1[ct]);
                }
            }
    }
    // the four q groups in order: every lane forms the same sum
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const E t0 = ((__shfl(v0[ct], c16) + __shfl(v0[ct], c16 + 16)) + __shfl(v0[ct], c16 + 32)) + __shfl(v0[ct], c16 + 48);
        const E t1 = ((__shfl(v1[ct], c16) + __shfl(v1[ct], c16 + 16)) + __shfl(v1[ct], c16 + 32)) + __shfl(v1[ct], c16 + 48);
        if (q == 0) {
            red[(wave * 2 + 0) * T + 16 * ct + c16] = t0;
            red[(wave * 2 + 1) * T + 16 * ct + c16] = t1;
        }
    }
    __syncthreads();
    if (tid < 2 * T) {
        const int s = tid / T, col = tid - s * T, img = tile0 + col;
        if (img < g.cnt) {
            E sum = 0;
            for (int w = 0; w < CHAIN_WAVES; ++w) sum += red[(w * 2 + s) * T + col];
            g.dphi[((size_t)(j - 1) * 2 + s) * g.ld + img] = sum;
        }
    }
}

// a.mcap and the grid follow from T and maxbond; rows: a.rowoff[N + 1] as the host knows it; tape_elems: elements behind each of the two tapes
template <typename E>
int launch_input_grad(tnml_ctx* c, InputGradArgsT<E> a, int maxbond, int T, int rows, size_t tape_elems, double* outT, float* outT32) {
    typedef ChainT<E> Tr;
    constexpr bool f32 = sizeof(E) == sizeof(float);
    const char* const name = "input gradient kernel";
    if (maxbond < 1 || maxbond > Tr::MAXM) return tnml_fail(c, "%s: bond dimension %d outside 1..%d", name, maxbond, Tr::MAXM);
    if (a.cnt < 1 || a.cnt > a.ld) return tnml_fail(c, "%s: %d images in a chunk of %d", name, a.cnt, a.ld);
    if (T != 64 && T != 32 && T != 16) return tnml_fail(c, "%s: tile width %d", name, T);
    if (!a.tape || !a.tape2 || !a.coef || !a.dphi || (!outT && !outT32)) return tnml_fail(c, "%s: null argument", name);
    a.mcap = (maxbond + 15) / 16 * 16;
    const int grid = (a.cnt + T - 1) / T;
    const size_t lds = ((size_t)a.mcap * T + (size_t)CHAIN_WAVES * 2 * T) * sizeof(E);
    if (lds > TNML_CHAIN_LDS / 2) return tnml_fail(c, "%s: a tile of %d x %d does not leave room for a second workgroup in the LDS", name, a.mcap, T);
    if ((size_t)grid * T * rows > tape_elems) return tnml_fail(c, "%s: tapes of %zu %s too small for %d tiles of %d x %d", name, tape_elems, Tr::elems, grid, rows, T);
    typedef void (*kern_t)(const InputGradArgsT<E>);
    static const kern_t kern[3] = {k_input_grad<E, 1>, k_input_grad<E, 2>, k_input_grad<E, 4>};     // [T / 32]
    if (!c->attr_inputgrad[f32]) {
        for (kern_t fn : kern)
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, TNML_CHAIN_LDS / 2) != hipSuccess)
                return tnml_fail(c, "%s: hipFuncSetAttribute failed", name);
        c->attr_inputgrad[f32] = true;
    }
    {
        ProfScope ps(c, KC_INPUT_GRAD);
        hipLaunchKernelGGL(kern[T / 32], dim3(grid, a.N), dim3(CHAIN_THREADS), lds, c->stream, a);
        HIPCK(c, hipGetLastError());
    }
    ProfScope ps(c, KC_PACK);
    return launch_response_transpose(c, a.dphi, 2 * a.N, a.cnt, a.ld, outT, outT32);
}
template int launch_input_grad<double>(tnml_ctx*, InputGradArgsT<double>, int, int, int, size_t, double*, float*);
template int launch_input_grad<float>(tnml_ctx*, InputGradArgsT<float>, int, int, int, size_t, double*, float*);
