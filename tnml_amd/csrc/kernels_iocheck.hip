// kernels_iocheck.hip -- the value checks of the device-resident calls (tnml_*_dev, tnml.h).
//
// The host-pointer calls walk labels / coef / which on the CPU and refuse before any work.  Arrays that live on the device are walked
// here instead: ONE launch of k_check_batch (class io_check) over the whole batch, before the chunk loop.
//   labels [n]      : offends when outside 0 .. TNML_NL - 1
//   coef   [n][nl]  : offends when not finite (all exponent bits set: the test is on the bit pattern, nothing floating-point is done)
//   which  [n]      : offends when outside 0 .. nl - 1
// Every thread walks the three arrays with a grid-stride loop and keeps the smallest offending index it has met; a thread that has met
// one lowers the array's word of the 24-byte block `blk` (three unsigned 64-bit words, set to all ones by the host before the launch)
// with a 64-bit integer atomicMin.  The host reads the block once: a word that is still all ones means the array is clean, otherwise
// it is the smallest offending flat index -- what the host loops report.
#include <algorithm>

#include "tnml_internal.h"

__global__ __launch_bounds__(256) void k_check_batch(const int* __restrict__ labels, const double* __restrict__ coef, const int* __restrict__ which,
                                                     long long n, int nl, unsigned long long* __restrict__ blk) {
    const unsigned long long none = ~0ull;
    const size_t t0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    if (labels) {
        unsigned long long bad = none;
        for (size_t i = t0; i < (size_t)n; i += step) {
            const int v = labels[i];
            if ((v < 0 || v >= TNML_NL) && bad == none) bad = i;          // ascending i: the first hit of this thread is its smallest
        }
        if (bad != none) atomicMin(blk + 0, bad);
    }
    if (coef) {
        unsigned long long bad = none;
        const size_t total = (size_t)n * nl;
        for (size_t i = t0; i < total; i += step) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(coef[i]);
            if ((bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull && bad == none) bad = i;
        }
        if (bad != none) atomicMin(blk + 1, bad);
    }
    if (which) {
        unsigned long long bad = none;
        for (size_t i = t0; i < (size_t)n; i += step) {
            const int v = which[i];
            if ((v < 0 || v >= nl) && bad == none) bad = i;
        }
        if (bad != none) atomicMin(blk + 2, bad);
    }
}

int launch_check_batch(tnml_ctx* c, const int* labels, const double* coef, const int* which, int64_t n, int nl, unsigned long long* blk) {
    if (!blk || n < 1) return tnml_fail(c, "check of the batch: null argument");
    ProfScope ps(c, KC_IO_CHECK);
    const size_t total = labels || coef || which ? (size_t)n * (coef ? nl : 1) : 1;    // (no array: one workgroup that finds nothing to walk)
    const int grid = (int)std::min<size_t>((total + 255) / 256, 1024);
    hipLaunchKernelGGL(k_check_batch, dim3(grid), dim3(256), 0, c->stream, labels, coef, which, (long long)n, nl, blk);
    HIPCK(c, hipGetLastError());
    return 0;
}
