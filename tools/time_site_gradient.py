"""Site gradients from bytes at N = 784, m = 120 (fp64): tnml_site_gradient_u8 in the labels mode against tnml_response_u8 on the same
data-less context, for n = 256 and 10 000 images.

    python tools/time_site_gradient.py [--n 256,10000] [--repeats 3] [--chunk C] [--timeout 300] [--out profiles/site_gradient_time.txt]

Every leg runs in a child process of its own under `timeout`; a child that fails or hangs ends the tool (nothing more is started on
the GPU).  Per image count: one warm-up leg of each path (discarded), then the two paths alternated, `--repeats` legs each.  A leg
builds its context, makes one untimed call (code objects, first-touch allocations: the workspace is allocated there), times one call,
and repeats the call with the profile API on for the kernel time by class.  --chunk sets option gradient_chunk of the gradient legs
(0: the library's default); the response legs keep response_chunk's default.  The share of the fp64 matrix peak counts the
multiply-adds of the definition, 4 ml mr (x 10 on the Label site) per site and image, not the padded tiles the kernel executes.
No pass / fail time: the figures are written down with the spread of the repeats."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 784, 120
PEAK_TF = 78.6                                    # fp64 matrix peak of the MI355X


def child(path, n, chunk):
    sys.path.insert(0, ROOT)
    import numpy as np
    from tnml_amd import synth
    from tnml_amd.fixedl import TrainStates
    labels = np.ascontiguousarray(synth.synthetic_labels(n), dtype=np.int32)
    pixels = np.ascontiguousarray(synth.synthetic_images(N, labels), dtype=np.uint8)
    W = synth.random_mps(N, M, seed=1)
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, M, no_data=True, device=0)
    ts.set_mps(W)
    if chunk and path == "gradient":
        ts.set_option("gradient_chunk", chunk)

    def call():
        if path == "gradient":
            g, (w, pred) = ts.site_gradient(labels=labels, pixels=pixels, want_weights=True)
            return g, w, pred
        r, (w, pred) = ts.site_response(pixels=pixels, want_weights=True)
        return r, w, pred
    call()
    ts.synchronize()
    t0 = time.perf_counter()
    r, w, pred = call()
    ts.synchronize()
    dt = time.perf_counter() - t0
    ts.profile(True)
    ts.profile_reset()
    call()
    prof = {k: v for k, v in ts.profile_read().items() if v[0]}
    ts.profile(False)
    out = dict(path=path, n=n, seconds_call=dt, device_bytes=ts.device_bytes(), launches={k: v[0] for k, v in prof.items()},
               kernel_ms={k: v[1] for k, v in prof.items()}, checksum=float(np.abs(w).sum()), pred_hist=np.bincount(pred, minlength=10).tolist())
    if path == "gradient":                        # the Euler identity at three sites: sum A_j G_j = sum c W, c = 2 (W - y)
        c = 2. * (w - np.eye(10)[labels])
        want = float((c * w).sum())
        euler = max(abs(float((W[j] * r[j]).sum()) - want) for j in (0, N // 2 - 1, N - 1)) / abs(want)
        out.update(euler=euler, grad_sum=float(sum(np.abs(g).sum() for g in r)), flops=float(sum(2. * A.size for A in W)) * n)
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="256,10000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=0, help="option gradient_chunk of the gradient legs (0: the library's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_gradient_time.txt"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        path, n = a.child.split(",")
        child(path, int(n), a.chunk)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()

    def say(s):                                   # to the terminal and, line by line, to the output file
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    def leg(path, n):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "%s,%d" % (path, n), "--chunk", str(a.chunk)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            say("leg %s n = %d failed (exit %d)\n%s\n%s" % (path, n, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            return None
        return json.loads(line[0][len("RESULT "):])

    def med(v):
        return sorted(v)[len(v) // 2]

    def spread(v, unit="s"):
        return "%.4f %s (min %.4f, max %.4f)" % (med(v), unit, min(v), max(v))
    say("site gradients from bytes (labels mode), N = %d, m = %d, fp64: tnml_site_gradient_u8 against tnml_response_u8; per leg one untimed call, one timed call; median (min, max) of %d legs%s"
        % (N, M, a.repeats, "; gradient_chunk = %d" % a.chunk if a.chunk else ""))
    paths = ("response", "gradient")
    results = []
    for n in (int(x) for x in a.n.split(",")):
        if any(leg(path, n) is None for path in paths):      # warm-up of each shape, discarded
            return 1
        res = {path: [] for path in paths}
        for _ in range(a.repeats):
            for path in paths:
                r = leg(path, n)
                if r is None:
                    return 1
                res[path].append(r)
        p, q = res["response"], res["gradient"]
        tp, tq = [r["seconds_call"] for r in p], [r["seconds_call"] for r in q]
        kp = [r["kernel_ms"].get("site_resp", 0.) for r in p]
        kb, kg = [r["kernel_ms"].get("site_bwd", 0.) for r in q], [r["kernel_ms"].get("site_grad", 0.) for r in q]
        say("n = %d" % n)
        say("  tnml_response_u8      call %s = %.0f images/s; launches %s; device bytes %d"
            % (spread(tp), n / med(tp), json.dumps(p[0]["launches"], sort_keys=True), p[0]["device_bytes"]))
        say("  tnml_site_gradient_u8 call %s = %.0f images/s; launches %s; device bytes %d"
            % (spread(tq), n / med(tq), json.dumps(q[0]["launches"], sort_keys=True), q[0]["device_bytes"]))
        say("  kernel time per call: class site_resp under response %s; class site_bwd %s; class site_grad %s; class pack under gradient %.3f ms"
            % (spread(kp, "ms"), spread(kb, "ms"), spread(kg, "ms"), q[0]["kernel_ms"].get("pack", 0.)))
        tf = q[0]["flops"] / (med(kg) * 1e-3) / 1e12
        say("  site_bwd / site_resp = %.2f; site_grad / site_resp = %.2f; (site_bwd + site_grad) / site_resp = %.2f; gradient / response (call alone) = %.2f"
            % (med(kb) / med(kp), med(kg) / med(kp), (med(kb) + med(kg)) / med(kp), med(tq) / med(tp)))
        say("  site_grad: %.3e multiply-add flops per call = %.2f TF = %.3f of the fp64 matrix peak (%.1f TF); weights agree: %s; Euler identity at sites 1, %d, %d: %.2e; sum |G| %.12e"
            % (q[0]["flops"], tf, tf / PEAK_TF, PEAK_TF, p[0]["checksum"] == q[0]["checksum"] and p[0]["pred_hist"] == q[0]["pred_hist"], N // 2, N, q[0]["euler"], q[0]["grad_sum"]))
        results.append(dict(n=n, response=p, gradient=q))
    with open(a.out, "a") as f:
        f.write(json.dumps(results) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
