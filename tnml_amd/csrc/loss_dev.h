// loss_dev.h -- softmax cross-entropy of one image (option "loss" = TNML_LOSS_SOFTMAX), for k_site_backward and k_eval_tally.
//
// Only __device__ functions, fp64, compiled with -ffp-contract=off like the files that include it: every operation below is ONE IEEE
// rounding (add, subtract, multiply, divide, v_rndne_f64; v_ldexp_f64 is exact here), so that tests/loss_model.py restates them in
// numpy bit for bit.  No call into the device library's exp or log: their last bits are not ours to state.
//
//   exp_fixed(x), x <= 0:   0 for x < -708 (tested before anything else: -Inf never reaches a conversion to int); otherwise
//                           k = rint(x LOG2E), r = (x - k LN2_HI) - k LN2_LO, p = sum_{n=0..13} E_n r^n by Horner from E_13 down,
//                           E_n = fl(1 / n!), result ldexp(p, k).  |r| <= (ln 2) / 2 (1 + small), k >= -1022: the result is a normal number.
//   log_fixed(S), 1 <= S <= 10: k = 0; while S >= SQRT2: S <- S / 2, k <- k + 1 (at most 4 passes); f = (S - 1) / (S + 1), z = f f,
//                           q = sum_{n=0..11} L_n z^n by Horner from L_11 down, L_n = fl(1 / (2 n + 1)); result fl(fl(k LN2) + fl(fl(2 f) q)).
//
// The image (w_0..w_9 its weights, y its label, beta = option "loss_beta"):
//   m   = first maximum of w_l, l ascending (m = w_0; then w_l > m ? w_l : m)
//   d   = the first l with w_l == m                 the signed decision (0 when no l compares equal: m is NaN)
//   x_l = fl(beta fl(w_l - m))                      <= 0, x_d = 0
//   e_l = exp_fixed(x_l),  S = e_0 + e_1 + ... + e_9 (left to right; 1 <= S <= 10),  p_l = e_l / S
//   c_l = fl(beta fl(p_l - [l == y]))               dC/dW_l
//   C   = fl(log_fixed(S) - x_y)                    the image's cost, >= 0
// A weight that is not finite: every c_l and C are NaN (tested first; nothing is converted to an integer).
#pragma once
#include "tnml_internal.h"

#define LOSS_LOG2E  0x1.71547652b82fep+0
#define LOSS_LN2_HI 0x1.62e42fee00000p-1
#define LOSS_LN2_LO 0x1.a39ef35793c76p-33
#define LOSS_LN2    0x1.62e42fefa39efp-1
#define LOSS_SQRT2  0x1.6a09e667f3bcdp+0

static __device__ __forceinline__ double exp_fixed(double x) {
    if (x < -708.0) return 0.0;
    // E_n = fl(1 / n!): n! is exact in fp64 up to 18!, the quotient is rounded once by the compiler
    constexpr double E[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
                              1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    const double k = __builtin_rint(x * LOSS_LOG2E);
    const double r = (x - k * LOSS_LN2_HI) - k * LOSS_LN2_LO;
    double p = E[13];
#pragma unroll
    for (int n = 12; n >= 0; --n) p = p * r + E[n];
    return __builtin_ldexp(p, (int)k);
}

static __device__ __forceinline__ double log_fixed(double S) {
    constexpr double L[12] = {1.0, 1.0 / 3.0, 1.0 / 5.0, 1.0 / 7.0, 1.0 / 9.0, 1.0 / 11.0, 1.0 / 13.0, 1.0 / 15.0, 1.0 / 17.0, 1.0 / 19.0, 1.0 / 21.0, 1.0 / 23.0};
    double k = 0.0;
    while (S >= LOSS_SQRT2) { S = 0.5 * S; k = k + 1.0; }
    const double f = __ddiv_rn(S - 1.0, S + 1.0), z = f * f;
    double q = L[11];
#pragma unroll
    for (int n = 10; n >= 0; --n) q = q * z + L[n];
    return k * LOSS_LN2 + (2.0 * f) * q;
}

// w: the image's weights, overwritten by its coefficients c; -> its cost C; *d: its signed decision
static __device__ __forceinline__ double loss_softmax(double (&w)[TNML_NL], int y, double beta, int* d) {
    bool finite = true;
#pragma unroll
    for (int l = 0; l < TNML_NL; ++l) finite = finite && __builtin_isfinite(w[l]);
    double m = w[0];
#pragma unroll
    for (int l = 1; l < TNML_NL; ++l) m = w[l] > m ? w[l] : m;
    int dec = 0;
#pragma unroll
    for (int l = TNML_NL - 1; l >= 0; --l) dec = w[l] == m ? l : dec;
    *d = dec;
    if (!finite) {
        const double nan = __builtin_nan("");
#pragma unroll
        for (int l = 0; l < TNML_NL; ++l) w[l] = nan;
        return nan;
    }
    double S = 0.0, xy = 0.0;
#pragma unroll
    for (int l = 0; l < TNML_NL; ++l) {
        const double x = beta * (w[l] - m);
        xy = l == y ? x : xy;
        w[l] = exp_fixed(x);
        S = l == 0 ? w[0] : S + w[l];
    }
#pragma unroll
    for (int l = 0; l < TNML_NL; ++l) w[l] = beta * (__ddiv_rn(w[l], S) - (l == y ? 1.0 : 0.0));
    return log_fixed(S) - xy;
}
