"""Timing of the linear classifier's CG (kernels_linear.hip) at MNIST size: 60 000 images x 784 pixels (uint8), K = 1 and K = 10.

    python tools/time_linear.py [--passes 500] [--nt 60000] [--timeout 300]

Each K runs in a child process of its own under `timeout`; a child that fails or hangs ends the tool (nothing more is started on the
GPU).  Reports passes/s, microseconds per pass and the time of one 5 000-pass run (linear.cc's default Nlinear_iter) for all K columns,
next to the roofs of DESIGN.md (fp64 matrix 78.6 TF, HBM 8 TB/s).  Per-kernel times: run the tool under
`rocprofv3 --kernel-trace --stats -- python tools/time_linear.py`.  Separate from bench.py, which times fixedL."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(K, NT, passes):
    sys.path.insert(0, ROOT)
    import numpy as np
    from tnml_amd import synth
    from tnml_amd.linear import LinearCG
    N = 784
    labels = synth.synthetic_labels(NT)
    pixels = synth.synthetic_images(N, labels)
    cols = list(range(K))
    V0 = np.random.default_rng(1).uniform(size=(K, N + 1))
    V0 /= np.linalg.norm(V0, axis=1, keepdims=True)
    cg = LinearCG(labels, cols, pixels=pixels, device=0)
    cg.start(V0, 0.0)
    cg.run(20)                                           # warm-up (code objects, caches)
    t0 = time.perf_counter()
    costs = cg.run(passes)                               # one device round trip at the end
    dt = time.perf_counter() - t0
    Dp = (N + 1 + 15) // 16 * 16
    NTp = (NT + 1023) // 1024 * 1024
    ncol_a = 16 if K <= 8 else 32                        # stream A columns [W | p], padded
    flops_mfma = 2.0 * NTp * Dp * (ncol_a + 16)          # matrix-pipe work as issued (padding included)
    flops_useful = 2.0 * NT * (N + 1) * 3 * K            # the two streams' useful work (2K + K columns)
    bytes_x = 2.0 * NT * N                               # X read twice per pass (uint8)
    us = dt / passes * 1e6
    out = dict(K=K, NT=NT, N=N, passes=passes, seconds=dt, passes_per_s=passes / dt, us_per_pass=us,
               s_per_5000_passes=5000 * dt / passes, last_cost=[float(c) for c in costs[-1]],
               issued_tflops=flops_mfma / (us * 1e-6) / 1e12, useful_tflops=flops_useful / (us * 1e-6) / 1e12,
               compute_floor_us_useful=flops_useful / 78.6e12 * 1e6, memory_floor_us_hbm=bytes_x / 8e12 * 1e6,
               memory_floor_us_6tbs=bytes_x / 6e12 * 1e6)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=500)
    ap.add_argument("--nt", type=int, default=60000)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--ks", default="1,10")
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.nt, a.passes)
        return 0
    results = []
    for K in [int(k) for k in a.ks.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", str(K),
               "--nt", str(a.nt), "--passes", str(a.passes)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("K=%d failed (exit %d)\n%s\n%s" % (K, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            return 1
        r = json.loads(line[0][7:])
        results.append(r)
        print("K=%2d  NT=%d N=%d: %.1f passes/s, %.1f us/pass (floors: compute %.1f us useful fp64 @ 78.6 TF, memory %.1f us @ 8 TB/s, "
              "%.1f us @ 6 TB/s), %.3f s per 5000 passes, %.1f TF issued / %.1f TF useful"
              % (K, r["NT"], r["N"], r["passes_per_s"], r["us_per_pass"], r["compute_floor_us_useful"], r["memory_floor_us_hbm"],
                 r["memory_floor_us_6tbs"], r["s_per_5000_passes"], r["issued_tflops"], r["useful_tflops"]), flush=True)
    print(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
