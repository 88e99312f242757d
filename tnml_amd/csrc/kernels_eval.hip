// kernels_eval.hip -- streamed evaluation (tnml_evaluate_u8 / tnml_evaluate_phi): the tallies of a held-out report over the
// results k_chain left for a chunk.
//
// k_eval_tally, ONE workgroup of EVAL_THREADS threads per chunk, on the context's stream right behind the chunk's chain launch:
//   cost      label_cost[l] collects the images whose true label is l, as the reports of training do in both modes.  Thread t walks
//             its images t, t + EVAL_THREADS, ... in ascending order; an image's cost is the sum of (w_l - y_l)^2 over l = 0..9 in index
//             order (one term in the per-label variant) and goes to the thread's partial sum of the image's true label; the ten partial
//             sums are kept label by label.  The EVAL_THREADS partial sums of a label are then added by a fixed tree in LDS (stride
//             EVAL_THREADS / 2, ..., 1: element t += element t + stride), and thread 0 adds the chunk's ten sums to the running totals
//             in the accumulator block.  Chunks share the stream, so they are added in chunk order.  No floating-point atomic anywhere:
//             the totals are the same bits on every repeat and do not depend on predict_tile (k_chain's results do not).  They do depend
//             on where the chunks are cut: another predict_chunk may change the last bits of the costs.
//   integers  count, nincorrect and confusion are counted in LDS with integer atomics and added to the accumulator block by one thread
//             per counter: exact, whatever the chunking.
// Plain loads and stores; the single workgroup exchanges nothing with any other and waits for nothing.
//
// k_eval_tally<1> (option "loss" = TNML_LOSS_SOFTMAX; never the per-label variant): the image's term is the cross-entropy C of loss_dev.h
// in place of the sum of squares, added into the same partial sums and carried through the same tree and chunk order; nincorrect and
// confusion count the signed decision d of loss_dev.h, not pred.  k_eval_tally<0> is the code as it was.
#include <hip/hip_runtime.h>

#include "loss_dev.h"

#define EVAL_THREADS 256
#define EVAL_NCNT (2 * TNML_NL + TNML_NL * TNML_NL)      // LDS counters: count | nincorrect | confusion

template <int LOSS>
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_tally(const double* __restrict__ w, const int* __restrict__ pred, const int* __restrict__ lab,
                                                             int cnt, int nl, int single, int target, double beta, EvalAcc* __restrict__ acc) {
    __shared__ double red[TNML_NL][EVAL_THREADS];
    __shared__ int tally[EVAL_NCNT];
    const int t = threadIdx.x;
    for (int k = t; k < EVAL_NCNT; k += EVAL_THREADS) tally[k] = 0;
    __syncthreads();
    double s[TNML_NL];
#pragma unroll
    for (int l = 0; l < TNML_NL; ++l) s[l] = 0.;
    for (int i = t; i < cnt; i += EVAL_THREADS) {
        const int y = lab[i];
        int p = pred[i];
        bool wrong;
        if constexpr (LOSS == 1) {
            const double* wi = w + (size_t)i * nl;
            double wv[TNML_NL];
#pragma unroll
            for (int l = 0; l < TNML_NL; ++l) wv[l] = wi[l];
            const double per = loss_softmax(wv, y, beta, &p);
#pragma unroll
            for (int l = 0; l < TNML_NL; ++l) s[l] += l == y ? per : 0.;
            wrong = p != y;
        } else if (single) {
            const int yt = y == target ? 1 : 0;
            const double d = w[i] - (double)yt, dd = d * d;
#pragma unroll
            for (int l = 0; l < TNML_NL; ++l) s[l] += l == y ? dd : 0.;          // (+ 0 leaves a partial sum as it is)
            wrong = p != yt;
        } else {
            const double* wi = w + (size_t)i * nl;
            double per = 0.;
#pragma unroll
            for (int l = 0; l < TNML_NL; ++l) { const double d = wi[l] - (l == y ? 1. : 0.); per += d * d; }
#pragma unroll
            for (int l = 0; l < TNML_NL; ++l) s[l] += l == y ? per : 0.;
            wrong = p != y;
        }
        atomicAdd(&tally[y], 1);
        if (wrong) atomicAdd(&tally[TNML_NL + y], 1);
        if (p >= 0 && p < TNML_NL) atomicAdd(&tally[2 * TNML_NL + y * TNML_NL + p], 1);
    }
#pragma unroll
    for (int l = 0; l < TNML_NL; ++l) red[l][t] = s[l];
    __syncthreads();
    for (int stride = EVAL_THREADS / 2; stride > 0; stride >>= 1) {
        if (t < stride) {
#pragma unroll
            for (int l = 0; l < TNML_NL; ++l) red[l][t] += red[l][t + stride];
        }
        __syncthreads();
    }
    if (t == 0) {
        for (int l = 0; l < TNML_NL; ++l) acc->label_cost[l] += red[l][0];
    }
    for (int k = t; k < EVAL_NCNT; k += EVAL_THREADS) {                          // one thread per counter: no other workgroup writes the block
        long long* dst = k < TNML_NL ? &acc->count[k] : k < 2 * TNML_NL ? &acc->nincorrect[k - TNML_NL] : &acc->confusion[0][0] + (k - 2 * TNML_NL);
        *dst += tally[k];
    }
}

// loss, beta: options "loss" and "loss_beta" of the context
int launch_eval_tally(tnml_ctx* c, const double* w, const int* pred, const int* lab, int cnt, int nl, int single, int target, EvalAcc* acc, int loss, double beta) {
    if (cnt <= 0) return 0;
    if (nl != (single ? 1 : TNML_NL)) return tnml_fail(c, "launch_eval_tally: label extent %d", nl);
    if (loss != TNML_LOSS_QUADRATIC && (loss != TNML_LOSS_SOFTMAX || single)) return tnml_fail(c, "launch_eval_tally: loss %d%s", loss, single ? " in the per-label variant" : "");
    ProfScope ps(c, KC_EVAL_TALLY);
    hipLaunchKernelGGL(loss == TNML_LOSS_SOFTMAX ? k_eval_tally<1> : k_eval_tally<0>, dim3(1), dim3(EVAL_THREADS), 0, c->stream, w, pred, lab, cnt, nl, single, target, beta, acc);
    HIPCK(c, hipGetLastError());
    return 0;
}
