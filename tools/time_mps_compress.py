"""Timing of the W0..W9 start of fixedL at MNIST length: N = 784, ten random per-label weight MPS of bond 4, 10, 20, 40 and 120 summed
and compressed (Cutoff 1E-10, no Maxm) on the device (tnml_mps_place + tnml_mps_compress) and -- bond 4 and 10 only -- on the host
(tnmlh_mps_sum, part by part, what the fixedL driver's host path runs); and overlap(W,W) of a bond-120 W on the device against the
host contraction measured at bond 60 on six sites.

    python tools/time_mps_compress.py [--bonds 4,10,20,40,120] [--host-bonds 4,10] [--timeout 600] [--legs device,host,overlap]

Each leg runs in a child process of its own under `timeout`; a device leg that fails or hangs ends the tool (nothing more is started on
the GPU), a leg that runs into its timeout is reported as such.  Device seconds are wall-clock around the calls with the profile API on
(two event records per launch); the classes it separates: `svd` = the split of every bond (Gram matrix, eigensolver, factors -- the
profile API does not divide these further), `small_gemm` = the products A_b A_{b+1} (and the transfer steps of the overlap), the rest =
host time between launches, copies of eigenvalues, placement kernels.  Separate from bench.py, which times the sweep."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 784


def _parts(m, K=10, seed=1):
    import numpy as np
    rng = np.random.default_rng(seed)
    s = 1.0 / (2 * m) ** 0.5                              # transfer eigenvalue ~ 1: the norm stays in range over 784 sites
    return [[rng.standard_normal((1 if j == 0 else m, 2, 1 if j == N - 1 else m)) * s for j in range(N)] for _ in range(K)]


def child_device_sum(m):
    sys.path.insert(0, ROOT)
    import numpy as np
    from tnml_amd.fixedl import TrainStates
    parts = _parts(m)
    t0 = time.perf_counter()
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, 10 * m, no_data=True)
    t_create = time.perf_counter() - t0
    t0 = time.perf_counter()
    ts.set_sum(parts)
    ts.synchronize()
    t_place = time.perf_counter() - t0
    ts.profile(True)
    ts.profile_reset()
    t0 = time.perf_counter()
    rep = ts.compress(1e-10)
    t_comp = time.perf_counter() - t0
    prof = ts.profile_read()
    ts.profile_reset()
    t0 = time.perf_counter()
    ovl = ts.overlap()
    t_ovl = time.perf_counter() - t0
    prof_ovl = ts.profile_read()
    ts.profile(False)
    out = dict(leg="device_sum", bond=m, sum_bond=rep["maxm_before"], bond_after=rep["maxm_after"], discarded=rep["truncerr_sum"],
               fallbacks=rep["fallbacks"], create_s=t_create, place_s=t_place, compress_s=t_comp, overlap_s=t_ovl, overlap=ovl,
               svd_ms=prof["svd"][1], svd_calls=prof["svd"][0], products_ms=prof["small_gemm"][1],
               rest_s=t_comp - (prof["svd"][1] + prof["small_gemm"][1]) * 1e-3, overlap_kernels_ms=prof_ovl["small_gemm"][1],
               device_bytes=ts.device_bytes())
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def child_device_overlap(m):
    sys.path.insert(0, ROOT)
    import numpy as np
    from tnml_amd.fixedl import TrainStates
    rng = np.random.default_rng(3)
    s = 1.0 / (2 * m) ** 0.5
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, m, no_data=True)
    for j in range(1, N + 1):
        shape = (1 if j == 1 else m, 2, 1 if j == N else m) + ((10,) if j == N // 2 else ())
        ts.set_site(j, rng.standard_normal(shape) * (s / 10 ** 0.5 if j == N // 2 else s))
    ts.overlap()                                          # warm-up (code objects)
    ts.profile(True)
    ts.profile_reset()
    t0 = time.perf_counter()
    ovl = ts.overlap()
    dt = time.perf_counter() - t0
    prof = ts.profile_read()
    ts.close()
    print("RESULT " + json.dumps(dict(leg="device_overlap", bond=m, sites=N, seconds=dt, kernels_ms=prof["small_gemm"][1], overlap=ovl)), flush=True)


def child_host_overlap(m, sites):
    sys.path.insert(0, ROOT)
    import numpy as np
    from tnml_amd import hostlib
    rng = np.random.default_rng(3)
    n = 2 * sites + 2                                     # Label site beyond the timed ones: `sites` Label-free bulk sites are measured
    W = [rng.standard_normal((1 if j == 1 else m, 2, 1 if j == n else m) + ((10,) if j == n // 2 else ())) / (2 * m) ** 0.5 for j in range(1, n + 1)]
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "W")
        hostlib.write_mps(f, W)
        t0 = time.perf_counter()
        hostlib.mps_overlap(f, 1)
        t_read = time.perf_counter() - t0                 # reading the file + one edge site
        t0 = time.perf_counter()
        hostlib.mps_overlap(f, sites)
        dt = time.perf_counter() - t0 - t_read
    per_site = dt / (sites - 2)                           # site 1 has a 1 x 1 environment, the last kept site a 1-dimensional right link
    print("RESULT " + json.dumps(dict(leg="host_overlap", bond=m, sites=sites, seconds=dt, s_per_bulk_site=per_site,
                                      extrapolated_m120_N784_s=per_site * (120 / m) ** 4 * (N - 2), law="O(m^4) per site")), flush=True)


def child_host_sum(m):
    sys.path.insert(0, ROOT)
    from tnml_amd import hostlib
    parts = _parts(m)
    with tempfile.TemporaryDirectory() as d:
        files = []
        for k, P in enumerate(parts):
            files.append(os.path.join(d, "W%d" % k))
            hostlib.write_mps(files[-1], P)
        t0 = time.perf_counter()
        md = hostlib.mps_sum(files, os.path.join(d, "W"), cutoff=1e-10, one_shot=False)
        dt = time.perf_counter() - t0
        t0 = time.perf_counter()
        ovl = hostlib.mps_overlap(os.path.join(d, "W"))
        t_ovl = time.perf_counter() - t0
    print("RESULT " + json.dumps(dict(leg="host_sum", bond=m, sum_bond=10 * m, bond_after=md, seconds=dt, overlap_s=t_ovl, overlap=ovl)), flush=True)


def run_leg(args, timeout):
    """(result dict or None, 'ok' | 'timeout' | 'failed', tail of the output)"""
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + args
    t0 = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode in (124, 137):
        return dict(seconds=dt), "timeout", ""
    if p.returncode != 0 or not line:
        return None, "failed", "exit %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return json.loads(line[0][7:]), "ok", ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bonds", default="4,10,20,40,120")
    ap.add_argument("--host-bonds", default="4,10")
    ap.add_argument("--overlap-bond", type=int, default=120)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--legs", default="device,overlap,host")
    ap.add_argument("--child", default="")
    ap.add_argument("--bond", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        {"device_sum": lambda: child_device_sum(a.bond), "device_overlap": lambda: child_device_overlap(a.bond),
         "host_overlap": lambda: child_host_overlap(a.bond, 6), "host_sum": lambda: child_host_sum(a.bond)}[a.child]()
        return 0
    legs = a.legs.split(",")
    results = []
    print("N = %d, ten random parts per leg, Cutoff 1E-10, no Maxm; per-leg timeout %d s" % (N, a.timeout), flush=True)
    if "device" in legs:
        for m in [int(x) for x in a.bonds.split(",") if x]:
            r, st, tail = run_leg(["--child", "device_sum", "--bond", str(m)], a.timeout)
            if st == "failed":
                print("device sum, bond %d: FAILED -- nothing more is started on the GPU\n%s" % (m, tail))
                return 1
            if st == "timeout":
                print("device sum, parts of bond %3d (sum bond %4d): TIMED OUT after %d s -- nothing more is started on the GPU" % (m, 10 * m, a.timeout), flush=True)
                results.append(dict(leg="device_sum", bond=m, timeout_s=a.timeout))
                return 1
            results.append(r)
            print("device sum, parts of bond %3d (sum bond %4d -> %4d): place %.3f s, compress %.3f s = split %.3f (%d calls) + products %.3f + rest %.3f; "
                  "overlap of the result %.4f s; discarded weight %.2e, fallbacks %d, context %.2f GB (created in %.2f s)"
                  % (m, r["sum_bond"], r["bond_after"], r["place_s"], r["compress_s"], r["svd_ms"] * 1e-3, r["svd_calls"], r["products_ms"] * 1e-3,
                     r["rest_s"], r["overlap_s"], r["discarded"], r["fallbacks"], r["device_bytes"] / 2 ** 30, r["create_s"]), flush=True)
    if "overlap" in legs:
        r, st, tail = run_leg(["--child", "device_overlap", "--bond", str(a.overlap_bond)], a.timeout)
        if st != "ok":
            print("device overlap, bond %d: %s\n%s" % (a.overlap_bond, st.upper(), tail))
            return 1
        results.append(r)
        print("device overlap(W,W), W of bond %d, %d sites: %.4f s (kernels %.4f s)" % (r["bond"], r["sites"], r["seconds"], r["kernels_ms"] * 1e-3), flush=True)
        r, st, tail = run_leg(["--child", "host_overlap", "--bond", "60"], a.timeout)
        if st == "ok":
            results.append(r)
            print("host overlap(W,W), bond 60, %d sites MEASURED: %.3f s = %.4f s per bulk site; EXTRAPOLATED (not measured) with the %s law to bond 120 "
                  "and %d sites: %.0f s" % (r["sites"], r["seconds"], r["s_per_bulk_site"], r["law"], N, r["extrapolated_m120_N784_s"]), flush=True)
        else:
            print("host overlap, bond 60: %s\n%s" % (st.upper(), tail), flush=True)
    if "host" in legs:
        for m in [int(x) for x in a.host_bonds.split(",") if x]:
            r, st, tail = run_leg(["--child", "host_sum", "--bond", str(m)], a.timeout)
            if st == "timeout":
                results.append(dict(leg="host_sum", bond=m, timeout_s=a.timeout))
                print("host sum, parts of bond %3d (sum bond %4d): TIMED OUT after %d s (not finished; no time is reported)" % (m, 10 * m, a.timeout), flush=True)
            elif st == "ok":
                results.append(r)
                print("host sum, parts of bond %3d (sum bond %4d -> %4d), part by part: %.1f s; host overlap of the result %.2f s"
                      % (m, r["sum_bond"], r["bond_after"], r["seconds"], r["overlap_s"]), flush=True)
            else:
                print("host sum, bond %d: FAILED\n%s" % (m, tail), flush=True)
    print(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
