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

// ---- tnml_set_sites_dev: many site tensors in ONE launch (class sites_copy) ----
// Workgroup b serves the table entry with the last blk0 <= b (the entries' blk0 ascend from 0) and, of its elems doubles, those from
// (b - blk0) SITES_COPY_BLOCK on: plain 8-byte vector loads and stores, consecutive lanes on consecutive doubles.  The host has checked that
// every source holds its elems doubles; the destinations are W's own buffers at the shapes W has.
__global__ __launch_bounds__(256) void k_sites_gather(const SiteCopy* __restrict__ tab, int count) {
    int lo = 0, hi = count;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tab[mid].blk0 <= (long long)blockIdx.x) lo = mid; else hi = mid; }
    const SiteCopy e = tab[lo];
    const long long first = ((long long)blockIdx.x - e.blk0) * SITES_COPY_BLOCK;
    const long long last = first + SITES_COPY_BLOCK < e.elems ? first + SITES_COPY_BLOCK : e.elems;
    for (long long i = first + threadIdx.x; i < last; i += 256) e.dst[i] = e.src[i];
}

int launch_sites_gather(tnml_ctx* c, const SiteCopy* tab, int count, long long nblocks) {
    if (!tab || count < 1 || nblocks < 1 || nblocks > 0x7fffffffll) return tnml_fail(c, "copy of the sites: %d sites in %lld blocks", count, nblocks);
    ProfScope ps(c, KC_SITES_COPY);
    hipLaunchKernelGGL(k_sites_gather, dim3((unsigned)nblocks), dim3(256), 0, c->stream, tab, count);
    HIPCK(c, hipGetLastError());
    return 0;
}
