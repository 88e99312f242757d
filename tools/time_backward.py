"""The streamed backward pass from bytes at N = 784, m = 120 (fp64), labels mode, on one data-less context, for n = 256 and 10 000 images:

    dphi       tnml_backward_u8 with dphi alone (no gradient GEMM)
    grad       tnml_backward_u8 with grad alone
    both       tnml_backward_u8 with grad and dphi
    sitegrad   tnml_site_gradient_u8, the call grad must equal
    resp10     ten tnml_response_u8 calls, which = 0 .. 9: the only route to dphi before tnml_backward_*

    python tools/time_backward.py [--n 256,10000] [--repeats 3] [--chunk C] [--timeout 300] [--out profiles/backward_time.txt]

Every leg runs in a child process of its own under `timeout`; a child that fails or hangs ends the tool (nothing more is started on
the GPU).  Per image count: one warm-up leg of each path (discarded), then the paths alternated, `--repeats` legs each.  A leg builds its
context, makes one untimed call (code objects, first-touch allocations), times one call, and repeats the call with the profile API on
for the kernel time by class.  --chunk sets option gradient_chunk (0: the library's default); the response legs keep response_chunk's
default.  The share of the fp64 matrix peak of class input_grad counts the multiply-adds of the definition, 4 ml mr (x 10 on the Label
site) per site and image -- the count of class site_grad -- not the padded tiles the kernel executes.
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
PATHS = ("resp10", "sitegrad", "grad", "dphi", "both")


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
    if chunk and path != "resp10":
        ts.set_option("gradient_chunk", chunk)

    def call():
        """-> (grads | None, dphi | None or the ten responses, weights, pred)"""
        if path == "resp10":
            out = []
            for l in range(10):
                r, (w, pred) = ts.site_response(pixels=pixels, which=np.full(n, l, dtype=np.int32), want_weights=True)
                out.append(r)
            return None, out, w, pred
        if path == "sitegrad":
            g, (w, pred) = ts.site_gradient(labels=labels, pixels=pixels, want_weights=True)
            return g, None, w, pred
        g, d, (w, pred) = ts.backward(labels=labels, pixels=pixels, want_sites=path != "dphi", want_inputs=path != "grad", want_weights=True)
        return g, d, w, pred
    call()
    ts.synchronize()
    t0 = time.perf_counter()
    g, d, w, pred = call()
    ts.synchronize()
    dt = time.perf_counter() - t0
    ts.profile(True)
    ts.profile_reset()
    call()
    prof = {k: v for k, v in ts.profile_read().items() if v[0]}
    ts.profile(False)
    out = dict(path=path, n=n, seconds_call=dt, device_bytes=ts.device_bytes(), launches={k: v[0] for k, v in prof.items()},
               kernel_ms={k: v[1] for k, v in prof.items()}, checksum=float(np.abs(w).sum()), pred_hist=np.bincount(pred, minlength=10).tolist(),
               flops=float(sum(2. * A.size for A in W)) * n)
    c = 2. * (w - np.eye(10)[labels])
    if path == "resp10":                          # the host arithmetic that turns the ten responses into dphi
        d = sum(c[:, l, None, None] * r for l, r in enumerate(d))
    if d is not None:                             # the Euler tie at three sites: sum_s phi_s dphi_s = sum_l c_l W_l per image; phi of the bytes is (1, x / 255 / 255 / 4)
        want = (c * w).sum(axis=1)
        x = pixels.astype(np.float64) / 255. / 255. / 4.
        euler = max(float(np.abs(d[:, j, 0] + x[:, j] * d[:, j, 1] - want).max()) for j in (0, N // 2 - 1, N - 1)) / float(np.abs(want).max())
        out.update(euler=euler, dphi_sum=float(np.abs(d).sum()))
    if g is not None:
        out.update(grad_sum=float(sum(np.abs(a).sum() for a in g)))
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="256,10000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=0, help="option gradient_chunk of the gradient and backward legs (0: the library's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backward_time.txt"))
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
    say("streamed backward pass from bytes (labels mode), N = %d, m = %d, fp64; per leg one untimed call, one timed call; median (min, max) of %d legs%s"
        % (N, M, a.repeats, "; gradient_chunk = %d" % a.chunk if a.chunk else ""))
    names = dict(resp10="10 x tnml_response_u8", sitegrad="tnml_site_gradient_u8", grad="tnml_backward_u8 grad", dphi="tnml_backward_u8 dphi",
                 both="tnml_backward_u8 both")
    results = []
    for n in (int(x) for x in a.n.split(",")):
        if any(leg(path, n) is None for path in PATHS):      # warm-up of each shape, discarded
            return 1
        res = {path: [] for path in PATHS}
        for _ in range(a.repeats):
            for path in PATHS:
                r = leg(path, n)
                if r is None:
                    return 1
                res[path].append(r)
        say("n = %d" % n)
        t = {path: [r["seconds_call"] for r in res[path]] for path in PATHS}
        for path in PATHS:
            classes = ("site_resp",) if path == "resp10" else ("site_bwd", "site_grad", "input_grad", "pack")
            km = ", ".join("%s %s" % (k, spread([r["kernel_ms"].get(k, 0.) for r in res[path]], "ms")) for k in classes if any(r["kernel_ms"].get(k) for r in res[path]))
            say("  %-22s call %s = %.0f images/s; launches %s; device bytes %d" % (names[path], spread(t[path]), n / med(t[path]), json.dumps(res[path][0]["launches"], sort_keys=True), res[path][0]["device_bytes"]))
            say("  %-22s kernel time per call: %s" % ("", km))
        ki = med([r["kernel_ms"]["input_grad"] for r in res["both"]])
        kg = med([r["kernel_ms"]["site_grad"] for r in res["both"]])
        kb = med([r["kernel_ms"]["site_bwd"] for r in res["both"]])
        tf = res["both"][0]["flops"] / (ki * 1e-3) / 1e12
        say("  input_grad: %.3e multiply-add flops per call = %.2f TF = %.3f of the fp64 matrix peak (%.1f TF); input_grad / site_grad = %.2f; input_grad / site_bwd = %.3f"
            % (res["both"][0]["flops"], tf, tf / PEAK_TF, PEAK_TF, ki / kg, ki / kb))
        say("  calls: dphi / resp10 = %.3f; both / sitegrad = %.3f; grad / sitegrad = %.3f; dphi / sitegrad = %.3f"
            % (med(t["dphi"]) / med(t["resp10"]), med(t["both"]) / med(t["sitegrad"]), med(t["grad"]) / med(t["sitegrad"]), med(t["dphi"]) / med(t["sitegrad"])))
        same_w = all(res[p][0]["checksum"] == res["sitegrad"][0]["checksum"] and res[p][0]["pred_hist"] == res["sitegrad"][0]["pred_hist"] for p in PATHS)
        say("  weights agree across the paths: %s; sum |G| grad / both / sitegrad: %.12e / %.12e / %.12e; sum |dphi| dphi / both / resp10: %.12e / %.12e / %.12e"
            % (same_w, res["grad"][0]["grad_sum"], res["both"][0]["grad_sum"], res["sitegrad"][0]["grad_sum"], res["dphi"][0]["dphi_sum"], res["both"][0]["dphi_sum"], res["resp10"][0]["dphi_sum"]))
        say("  Euler tie at sites 1, %d, %d, worst over the images relative to the largest sum: dphi %.2e, resp10 %.2e" % (N // 2, N, res["dphi"][0]["euler"], res["resp10"][0]["euler"]))
        results.append(dict(n=n, **res))
    with open(a.out, "a") as f:
        f.write(json.dumps(results) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
