// kernels_gemm32.hip -- the reduced-precision study modes of the two image-proportional GEMMs (TNML_F32, TNML_BF16, TNML_BF16X3;
// BASELINE config 5's "bf16 MFMA bond contraction vs fp32"): k_fgemm<.., TO, ARITH> (feature GEMM / environment shift) and
// k_bgemm<.., ARITH> (gradient GEMM).  ARITH selects the matrix pipe: AR_F32 is v_mfma_f32_16x16x4_f32 on fp32 operands, AR_BF16 and
// AR_BF16X3 are v_mfma_f32_16x16x32_bf16 on operands rounded to bf16 while they are staged (plain, and hi + lo split).  Storage and
// accumulation are fp32 in all three, and so are the prologue, the C-fragment map and the epilogue of each kernel.
// The default arithmetic (fp64 MFMA) lives in kernels_gemm.hip; the algebra and the tile maps are the same.
#include "tnml_internal.h"
#include "bf16_dev.h"

enum { AR_F32 = 0, AR_BF16 = 1, AR_BF16X3 = 2 };        // the values of tnml_ctx::bf16() and BgemmArgs::bf16

// float4 loads are spelled out as casts at their sites: behind a one-line helper the compiler formed the addresses of the prologues
// differently in every kernel here (profiles/gemm32_shared_isa.txt; the shift at m = 300 measured 0.2 to 1.1 % slower with it)
static __device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }

template <int RT, int CT>
static __device__ __forceinline__ void clear_acc(f32x4 (&acc)[RT][CT]) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// images n .. n + 3 of row r of src[rows][NTp]; zero beyond the last row
static __device__ __forceinline__ float4 row4(const float* src, int r, int rows, int NTp, int n) {
    return r < rows ? *reinterpret_cast<const float4*>(src + (size_t)r * NTp + n) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// the staged operands, four images of the two site-index rows of one environment row, formed in fp32:
// X_n = EI_n (x) phiI_n, rows 2a and 2a + 1 ...
static __device__ __forceinline__ void load_x(const float* EI, int a, int mI, const float* phiI, int NTp, int n, float4& x0, float4& x1) {
    const float4 e = row4(EI, a, mI, NTp, n);
    x0 = mul4(e, *reinterpret_cast<const float4*>(phiI + n));
    x1 = mul4(e, *reinterpret_cast<const float4*>(phiI + NTp + n));
}
// ... and Z_n phiO_n w_n, rows 2q and 2q + 1 (w: per-image weight of this label, or null)
static __device__ __forceinline__ void load_zw(const float* Zq, int q, int mO, const float* w, const float* phiO, int NTp, int n, float4& y0, float4& y1) {
    float4 z = row4(Zq, q, mO, NTp, n);
    if (w) z = mul4(z, *reinterpret_cast<const float4*>(w + n));
    y0 = mul4(z, *reinterpret_cast<const float4*>(phiO + n));
    y1 = mul4(z, *reinterpret_cast<const float4*>(phiO + NTp + n));
}

// One 32-deep step of the bf16 matrix pipe for the RT x CT tiles of a wave whose first row / column in the workgroup's tile is arow / brow.
// An A / B fragment is 8 consecutive reduction indices of one row / column (k = 8 (lane >> 4) + 0..7), so the LDS tiles are [row][k] with
// k contiguous and a row stride of KS = 32 + 8 bf16 elements (80-byte rows: the four lane groups of a 16-byte fragment read land on
// distinct banks); the hi plane [AROWS][KS] / [BROWS][KS] is followed by the lo plane when SPLIT.  SPLIT: every operand x = hi + lo and
// three MFMAs per product, lo*hi + hi*lo + hi*hi (the lo*lo term is below fp32 round-off): ~16 mantissa bits.
template <int RT, int CT, int AROWS, int BROWS, int KS, bool SPLIT>
static __device__ __forceinline__ void bf16_step(const unsigned short* At, const unsigned short* Bt, int arow, int brow, int lane, f32x4 (&acc)[RT][CT]) {
    const int ko = 8 * (lane >> 4);
    bf16x8 ah[RT], bh[CT], al[SPLIT ? RT : 1], bl[SPLIT ? CT : 1];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        ah[r] = *reinterpret_cast<const bf16x8*>(&At[(arow + r * 16 + (lane & 15)) * KS + ko]);
        if (SPLIT) al[r] = *reinterpret_cast<const bf16x8*>(&At[AROWS * KS + (arow + r * 16 + (lane & 15)) * KS + ko]);
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        bh[c] = *reinterpret_cast<const bf16x8*>(&Bt[(brow + c * 16 + (lane & 15)) * KS + ko]);
        if (SPLIT) bl[c] = *reinterpret_cast<const bf16x8*>(&Bt[BROWS * KS + (brow + c * 16 + (lane & 15)) * KS + ko]);
    }
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (SPLIT) {                                   // small terms first
                acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[r], bh[c], acc[r][c], 0, 0, 0);
                acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[r], bl[c], acc[r][c], 0, 0, 0);
            }
            acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[r], bh[c], acc[r][c], 0, 0, 0);
        }
}

// ------------------------------------------------------------------------------------------
// k_fgemm -- out = X M with X_n = EI_n (x) phiI_n, 16 RT WR images x 16 CT WC columns per workgroup; TO == 1 is the environment shift
// (fp32 pipe in every mode), TO == 2 the forward feature GEMM (BASELINE config 5's "bf16 MFMA bond contraction" when ARITH is not AR_F32,
// a tolerance study).  On the bf16 pipe X is formed in fp32 and then rounded (round to nearest even), so is every element of the bond matrix.
// ------------------------------------------------------------------------------------------
template <int RT, int CT, int WR, int WC, int TO, int ARITH>
__global__ __launch_bounds__(64 * WR * WC) void k_fgemm(FgemmArgs A) {
    constexpr int T = 64 * WR * WC, BM = 16 * RT * WR, BN = 16 * CT * WC;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid / WC, wc = wid % WC;
    const int n0 = blockIdx.x * BM, j0 = blockIdx.y * BN, l = blockIdx.z;
    const float* E = A.EI + (size_t)l * A.EI_lstride;
    const float* M = A.M + (size_t)l * A.M_lstride;
    const int NTp = A.NTp;

    f32x4 acc[RT][CT];
    clear_acc(acc);

    if constexpr (ARITH == AR_F32) {
        constexpr int KT = 16;
        constexpr int XS = BM + 16;                         // row stride == 16 (mod 32): conflict-free fragment reads
        constexpr int MS = BN + ((BN % 32 == 16) ? 0 : 16);
        __shared__ __attribute__((aligned(16))) float lds[KT * XS + KT * MS];
        float* Xs = lds;
        float* Ms = lds + KT * XS;
        for (int k0 = 0; k0 < A.Kp; k0 += KT) {
            // stage X: KT/2 environment rows, each expanded to its two site-index rows
            for (int idx = tid; idx < (KT / 2) * (BM / 4); idx += T) {
                const int ar = idx / (BM / 4), c4 = idx % (BM / 4);
                float4 x0, x1;
                load_x(E, k0 / 2 + ar, A.mI, A.phiI, NTp, n0 + c4 * 4, x0, x1);
                *reinterpret_cast<float4*>(&Xs[(2 * ar) * XS + c4 * 4]) = x0;
                *reinterpret_cast<float4*>(&Xs[(2 * ar + 1) * XS + c4 * 4]) = x1;
            }
            // stage M: KT rows of the (zero padded) bond matrix
            for (int idx = tid; idx < KT * (BN / 4); idx += T) {
                const int r = idx / (BN / 4), c4 = idx % (BN / 4);
                const int j = j0 + c4 * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j < A.Np) v = *reinterpret_cast<const float4*>(M + (size_t)(k0 + r) * A.Np + j);
                *reinterpret_cast<float4*>(&Ms[r * MS + c4 * 4]) = v;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KT; kk += 4) {
                float a[RT], b[CT];
                const int krow = kk + (lane >> 4);
#pragma unroll
                for (int r = 0; r < RT; ++r) a[r] = Xs[krow * XS + (wr * RT + r) * 16 + (lane & 15)];
#pragma unroll
                for (int c = 0; c < CT; ++c) b[c] = Ms[krow * MS + (wc * CT + c) * 16 + (lane & 15)];
#pragma unroll
                for (int r = 0; r < RT; ++r)
#pragma unroll
                    for (int c = 0; c < CT; ++c) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[c], acc[r][c], 0, 0, 0);
            }
            __syncthreads();
        }
    } else {
        constexpr bool SPLIT = ARITH == AR_BF16X3;
        constexpr int KT = 32, KS = KT + 8, NP = SPLIT ? 2 : 1;     // KS: row stride in bf16 elements
        __shared__ __attribute__((aligned(16))) unsigned short lds[NP * (BM + BN) * KS];
        unsigned short* Xs = lds;                               // [NP][BM][KS]
        unsigned short* Ms = lds + NP * BM * KS;                // [NP][BN][KS]
        for (int k0 = 0; k0 < A.Kp; k0 += KT) {
            // stage X: KT/2 environment rows, each expanded to its two site-index rows, transposed to [image][k]
            for (int idx = tid; idx < (KT / 2) * (BM / 4); idx += T) {
                const int ar = idx / (BM / 4), c4 = idx % (BM / 4);
                float4 x0, x1;
                load_x(E, k0 / 2 + ar, A.mI, A.phiI, NTp, n0 + c4 * 4, x0, x1);
                const float xs[4][2] = {{x0.x, x1.x}, {x0.y, x1.y}, {x0.z, x1.z}, {x0.w, x1.w}};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned short h0 = f2bf(xs[q][0]), h1 = f2bf(xs[q][1]);
                    *reinterpret_cast<unsigned*>(&Xs[(c4 * 4 + q) * KS + 2 * ar]) = bf_pack(h0, h1);
                    if (SPLIT) *reinterpret_cast<unsigned*>(&Xs[BM * KS + (c4 * 4 + q) * KS + 2 * ar]) = bf_pack(bf_lo(xs[q][0], h0), bf_lo(xs[q][1], h1));
                }
            }
            // stage M: KT rows of the (zero padded) bond matrix, transposed to [column][k]
            for (int idx = tid; idx < KT * (BN / 4); idx += T) {
                const int r = idx / (BN / 4), c4 = idx % (BN / 4);
                const int j = j0 + c4 * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j < A.Np) v = *reinterpret_cast<const float4*>(M + (size_t)(k0 + r) * A.Np + j);
                const float mv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned short h = f2bf(mv[q]);
                    Ms[(c4 * 4 + q) * KS + r] = h;
                    if (SPLIT) Ms[BN * KS + (c4 * 4 + q) * KS + r] = bf_lo(mv[q], h);
                }
            }
            __syncthreads();
            bf16_step<RT, CT, BM, BN, KS, SPLIT>(Xs, Ms, wr * RT * 16, wc * CT * 16, lane, acc);
            __syncthreads();
        }
    }

    // epilogue: a C fragment (of either pipe) is 4 consecutive images (rows) x 1 column per lane.  TO == 2: column j = 2q + t carries the
    // output site index, contracted with phiO between neighbouring lanes
    float* out = A.out + (size_t)l * A.out_lstride;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int n = n0 + (wr * RT + r) * 16 + (lane >> 4) * 4;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int j = j0 + (wc * CT + c) * 16 + (lane & 15);
            if (TO == 2) {
                const int t = j & 1, q = j >> 1;
                const float4 ph = *reinterpret_cast<const float4*>(A.phiO + (size_t)t * NTp + n);
                float4 v = make_float4(acc[r][c][0] * ph.x, acc[r][c][1] * ph.y, acc[r][c][2] * ph.z, acc[r][c][3] * ph.w);
                v.x += __shfl_xor(v.x, 1); v.y += __shfl_xor(v.y, 1);
                v.z += __shfl_xor(v.z, 1); v.w += __shfl_xor(v.w, 1);
                if (t == 0 && q < A.mO) *reinterpret_cast<float4*>(out + (size_t)q * NTp + n) = v;
            } else {
                if (j < A.mO)
                    *reinterpret_cast<float4*>(out + (size_t)j * NTp + n) = make_float4(acc[r][c][0], acc[r][c][1], acc[r][c][2], acc[r][c][3]);
            }
        }
    }
}

// one forward / shift tile class in one arithmetic; shift is null on the bf16 pipe
struct FgemmKern {
    int BM, BN, threads;
    void (*shift)(FgemmArgs);
    void (*fwd)(FgemmArgs);
};
template <int RT, int CT, int WR, int WC, int ARITH>
static constexpr FgemmKern fkern() {
    if constexpr (ARITH == AR_F32) return {16 * RT * WR, 16 * CT * WC, 64 * WR * WC, k_fgemm<RT, CT, WR, WC, 1, ARITH>, k_fgemm<RT, CT, WR, WC, 2, ARITH>};
    else return {16 * RT * WR, 16 * CT * WC, 64 * WR * WC, nullptr, k_fgemm<RT, CT, WR, WC, 2, ARITH>};
}
static const FgemmKern fgemm_tab[4][3] = {                  // [tile class][ARITH]
    {fkern<4, 5, 2, 3, AR_F32>(), {}, {}},                                                              // 128 x 240
    {fkern<4, 4, 2, 2, AR_F32>(), fkern<4, 4, 2, 2, AR_BF16>(), fkern<4, 4, 2, 2, AR_BF16X3>()},        // 128 x 128
    {fkern<4, 2, 2, 2, AR_F32>(), fkern<4, 2, 2, 2, AR_BF16>(), fkern<4, 2, 2, 2, AR_BF16X3>()},        // 128 x 64
    {fkern<4, 1, 2, 2, AR_F32>(), {}, {}},                                                              // 128 x 32
};

int launch_fgemm(tnml_ctx* c, const FgemmArgs& a) {
    ProfScope ps(c, a.phiO ? KC_FGEMM_FWD : KC_FGEMM_SHIFT);
    if (a.NTp % TNML_NTPAD) return tnml_fail(c, "fgemm: NTp not padded");
    const int arith = a.phiO ? c->bf16() : AR_F32;          // the bf16 modes run the forward pass on the bf16 matrix pipe, the shift on the fp32 pipe
    int cls;
    if (arith != AR_F32) {                                  // the reduction runs in chunks of 32: Kp is a multiple of 16, the bond plan pads to 32 in these modes
        if (a.Kp % 32) return tnml_fail(c, "fgemm (bf16): the padded reduction dimension %d is not a multiple of 32", a.Kp);
        cls = a.Np > 64 ? 1 : 2;
    } else if (a.Np == 240) cls = 0;                        // m = 120: exactly 15 column tiles, no padding waste
    else if (a.Np > 64)     cls = 1;
    else if (a.Np > 32)     cls = 2;
    else                    cls = 3;
    const FgemmKern& k = fgemm_tab[cls][arith];
    if (!(a.phiO ? k.fwd : k.shift)) return tnml_fail(c, "fgemm: no kernel for tile class %d in arithmetic %d (%s)", cls, arith, a.phiO ? "forward" : "shift");
    const dim3 grid(a.NTp / k.BM, (a.Np + k.BN - 1) / k.BN, a.L);
    hipLaunchKernelGGL(a.phiO ? k.fwd : k.shift, grid, dim3(k.threads), 0, c->stream, a);
    HIPCK(c, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
struct BgemmKArgs {
    BgemmArgs a;
    float* slab;
    int nsplit, imgs_per_split;
};

// k_bgemm -- the gradient GEMM dP*dag(t.v) (fixedL.cc:379,418), split-K over the images into slabs: 16 RT WR rows x 16 CT WC columns per
// workgroup.  Both operands are formed in fp32 (X_n = EI_n (x) phiI_n, Z_n phiO_n w_n) while they are staged.  The reduction index is the
// image, which is already the contiguous index of both operands in memory.  On the bf16 pipe (TNML_BF16 / TNML_BF16X3) the operands are
// then rounded to bf16 (AR_BF16X3: hi + lo), an A / B fragment is 8 consecutive images of one row and one 32-image chunk is ONE MFMA step
// per tile.  With k_fgemm this puts the whole bond contraction of the bf16 modes on the bf16 pipe.
template <int RT, int CT, int WR, int WC, int ARITH>
__global__ __launch_bounds__(64 * WR * WC) void k_bgemm(BgemmKArgs K) {
    constexpr int T = 64 * WR * WC, BMr = 16 * RT * WR, BNc = 16 * CT * WC, KTn = 32;
    const BgemmArgs& A = K.a;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid / WC, wc = wid % WC;
    const int i0 = blockIdx.x * BMr, j0 = blockIdx.y * BNc;
    const int split = blockIdx.z % K.nsplit, l = blockIdx.z / K.nsplit;
    const int NTp = A.NTp;
    const int nbeg = split * K.imgs_per_split;
    const int nend = min(nbeg + K.imgs_per_split, NTp);
    const float* w = A.w ? A.w + (size_t)l * A.w_lstride : nullptr;

    f32x4 acc[RT][CT];
    clear_acc(acc);

    if constexpr (ARITH == AR_F32) {
        constexpr int ST = KTn + 4;
        __shared__ __attribute__((aligned(16))) float lds[(BMr + BNc) * ST];
        float* As = lds;
        float* Bs = lds + BMr * ST;
        for (int nb = nbeg; nb < nend; nb += KTn) {
            for (int idx = tid; idx < (BMr / 2) * (KTn / 4); idx += T) {
                const int ar = idx / (KTn / 4), c4 = idx % (KTn / 4);
                float4 x0, x1;
                load_x(A.EI, i0 / 2 + ar, A.mI, A.phiI, NTp, nb + c4 * 4, x0, x1);
                *reinterpret_cast<float4*>(&As[(2 * ar) * ST + c4 * 4]) = x0;
                *reinterpret_cast<float4*>(&As[(2 * ar + 1) * ST + c4 * 4]) = x1;
            }
            for (int idx = tid; idx < (BNc / 2) * (KTn / 4); idx += T) {
                const int qr = idx / (KTn / 4), c4 = idx % (KTn / 4);
                float4 y0, y1;
                load_zw(A.Zq, j0 / 2 + qr, A.mO, w, A.phiO, NTp, nb + c4 * 4, y0, y1);
                *reinterpret_cast<float4*>(&Bs[(2 * qr) * ST + c4 * 4]) = y0;
                *reinterpret_cast<float4*>(&Bs[(2 * qr + 1) * ST + c4 * 4]) = y1;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KTn; kk += 16) {
                // lane group g = lane>>4 owns images kk+4g..kk+4g+3; MFMA step e uses element e of every
                // group (a permutation of the reduction index, identical for A and B)
                float4 a[RT], b[CT];
                const int ko = kk + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < RT; ++r) a[r] = *reinterpret_cast<const float4*>(&As[((wr * RT + r) * 16 + (lane & 15)) * ST + ko]);
#pragma unroll
                for (int c = 0; c < CT; ++c) b[c] = *reinterpret_cast<const float4*>(&Bs[((wc * CT + c) * 16 + (lane & 15)) * ST + ko]);
#pragma unroll
                for (int r = 0; r < RT; ++r)
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].x, b[c].x, acc[r][c], 0, 0, 0);
                        acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].y, b[c].y, acc[r][c], 0, 0, 0);
                        acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].z, b[c].z, acc[r][c], 0, 0, 0);
                        acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].w, b[c].w, acc[r][c], 0, 0, 0);
                    }
            }
            __syncthreads();
        }
    } else {
        constexpr bool SPLIT = ARITH == AR_BF16X3;
        constexpr int KS = KTn + 8, NP = SPLIT ? 2 : 1;         // KS: row stride in bf16 elements (80 bytes)
        __shared__ __attribute__((aligned(16))) unsigned short lds[NP * (BMr + BNc) * KS];
        unsigned short* As = lds;                               // [NP][BMr][KS]
        unsigned short* Bs = lds + NP * BMr * KS;               // [NP][BNc][KS]
        auto put4 = [&](unsigned short* dst, unsigned short* dst_lo, float4 v) {          // four consecutive images of one row
            const float x[4] = {v.x, v.y, v.z, v.w};
            unsigned short hi[4], lo[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { hi[q] = f2bf(x[q]); lo[q] = bf_lo(x[q], hi[q]); }
            *reinterpret_cast<uint2*>(dst) = make_uint2(bf_pack(hi[0], hi[1]), bf_pack(hi[2], hi[3]));
            if (SPLIT) *reinterpret_cast<uint2*>(dst_lo) = make_uint2(bf_pack(lo[0], lo[1]), bf_pack(lo[2], lo[3]));
        };
        for (int nb = nbeg; nb < nend; nb += KTn) {
            for (int idx = tid; idx < (BMr / 2) * (KTn / 4); idx += T) {
                const int ar = idx / (KTn / 4), c4 = idx % (KTn / 4);
                float4 x0, x1;
                load_x(A.EI, i0 / 2 + ar, A.mI, A.phiI, NTp, nb + c4 * 4, x0, x1);
                put4(&As[(2 * ar) * KS + c4 * 4], &As[BMr * KS + (2 * ar) * KS + c4 * 4], x0);
                put4(&As[(2 * ar + 1) * KS + c4 * 4], &As[BMr * KS + (2 * ar + 1) * KS + c4 * 4], x1);
            }
            for (int idx = tid; idx < (BNc / 2) * (KTn / 4); idx += T) {
                const int qr = idx / (KTn / 4), c4 = idx % (KTn / 4);
                float4 y0, y1;
                load_zw(A.Zq, j0 / 2 + qr, A.mO, w, A.phiO, NTp, nb + c4 * 4, y0, y1);
                put4(&Bs[(2 * qr) * KS + c4 * 4], &Bs[BNc * KS + (2 * qr) * KS + c4 * 4], y0);
                put4(&Bs[(2 * qr + 1) * KS + c4 * 4], &Bs[BNc * KS + (2 * qr + 1) * KS + c4 * 4], y1);
            }
            __syncthreads();
            bf16_step<RT, CT, BMr, BNc, KS, SPLIT>(As, Bs, wr * RT * 16, wc * CT * 16, lane, acc);
            __syncthreads();
        }
    }

    float* slab = K.slab + ((size_t)split * A.L + l) * A.Kp * A.Np;
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int j = j0 + (wc * CT + c) * 16 + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + (wr * RT + r) * 16 + (lane >> 4) * 4 + e;
                if (i < A.Kp && j < A.Np) slab[(size_t)i * A.Np + j] = acc[r][c][e];
            }
        }
}

__global__ void k_slab_reduce(const float* __restrict__ slab, double* __restrict__ G, size_t n, int nsplit) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.;
    for (int k = 0; k < nsplit; ++k) s += (double)slab[(size_t)k * n + i];
    G[i] = s;
}

struct BgemmKern {                                          // one gradient tile class
    int BMr, BNc, threads;
    void (*fn[3])(BgemmKArgs);                              // [ARITH]
};
template <int RT, int CT, int WR, int WC>
static constexpr BgemmKern bkern() {
    return {16 * RT * WR, 16 * CT * WC, 64 * WR * WC, {k_bgemm<RT, CT, WR, WC, AR_F32>, k_bgemm<RT, CT, WR, WC, AR_BF16>, k_bgemm<RT, CT, WR, WC, AR_BF16X3>}};
}
static const BgemmKern bgemm_tab[3] = {bkern<1, 5, 5, 1>(), bkern<2, 2, 2, 2>(), bkern<1, 1, 2, 2>()};      // 80 x 80, 64 x 64, 32 x 32

int launch_bgemm(tnml_ctx* c, const BgemmArgs& a, double* G) {
    const BgemmKern& k = bgemm_tab[(a.Kp % 80 == 0 && a.Np % 80 == 0) ? 0         // 80 x 80 tiles (m = 40k: 240 = 3*80)
                                   : (a.Kp > 32 && a.Np > 32) ? 1 : 2];
    const int tiles = ((a.Kp + k.BMr - 1) / k.BMr) * ((a.Np + k.BNc - 1) / k.BNc) * a.L;
    int nsplit = (1024 + tiles - 1) / tiles;
    const int chunks = a.NTp / 32;
    if (nsplit > chunks) nsplit = chunks;
    if (nsplit < 1) nsplit = 1;
    const size_t n = (size_t)a.L * a.Kp * a.Np;
    const size_t cap = c->slab_bytes / sizeof(float);
    while (nsplit > 1 && (size_t)nsplit * n > cap) --nsplit;
    if ((size_t)nsplit * n > cap) return tnml_fail(c, "bgemm: slab workspace too small");
    int per = ((chunks + nsplit - 1) / nsplit) * 32;
    nsplit = (a.NTp + per - 1) / per;
    BgemmKArgs K{a, (float*)c->slab, nsplit, per};
    {
        ProfScope ps(c, KC_BGEMM);
        dim3 grid((a.Kp + k.BMr - 1) / k.BMr, (a.Np + k.BNc - 1) / k.BNc, nsplit * a.L);
        hipLaunchKernelGGL(k.fn[a.bf16 == 2 ? AR_BF16X3 : a.bf16 == 1 ? AR_BF16 : AR_F32], grid, dim3(k.threads), 0, c->stream, K);
    }
    {
        ProfScope ps(c, KC_SLABRED);
        hipLaunchKernelGGL(k_slab_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const float*)c->slab, G, n, nsplit);
    }
    HIPCK(c, hipGetLastError());
    return 0;
}
