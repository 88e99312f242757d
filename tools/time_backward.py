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
No pass / fail time: the figures are written down with the spread of the repeats.

    python tools/time_backward.py --dtype f64,f32 [--parent DIR] [--n 256,10000] [--repeats 3] [--out profiles/backward_time_f32.txt]

The second form compares option gradient_dtype.  Per image count the legs `both` (tnml_backward_u8 with grad and dphi) of each dtype --
and, with --parent DIR (a checkout of the parent commit with its library built), the fp64 leg on that build -- are alternated, each a child
process under `timeout`: call time, kernel time by class, tnml_device_bytes.  The fp64 legs of this build are then said to lie inside or
outside the parent's min-max, with the distance.  Then one `acc` leg per image count (fp64 and fp32 on one context: relmax of G and of
dphi, fp32 against fp64, and the Euler tie at three sites under each) and one fp32-only leg at a bond above 512 (N = 64, m = 600, 256
images), which fp64 refuses."""
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


def child(path, n, chunk, dtype="", root=ROOT, sites=N, bond=M):
    """dtype "" (the first form: the option is never touched), "f64" or "f32"; root: the checkout whose package and library are used;
    path "acc": both dtypes on one context, nothing timed"""
    sys.path.insert(0, root)
    import numpy as np
    from tnml_amd import synth
    from tnml_amd.fixedl import TrainStates
    N, M = sites, bond
    labels = np.ascontiguousarray(synth.synthetic_labels(n), dtype=np.int32)
    pixels = np.ascontiguousarray(synth.synthetic_images(N, labels), dtype=np.uint8)
    W = synth.random_mps(N, M, seed=1)
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, M, no_data=True, device=0)
    ts.set_mps(W)
    if chunk and path != "resp10":
        ts.set_option("gradient_chunk", chunk)
    x = pixels.astype(np.float64) / 255. / 255. / 4.

    def euler_of(d, w, f32):
        """the Euler tie at three sites: sum_s phi_s dphi_s = sum_l c_l W_l per image, worst over the images relative to the largest sum"""
        c = 2. * (w - np.eye(10)[labels])
        if f32:
            c = c.astype(np.float32).astype(np.float64)
        want = (c * w).sum(axis=1)
        return max(float(np.abs(d[:, j, 0] + x[:, j] * d[:, j, 1] - want).max()) for j in (0, N // 2 - 1, N - 1)) / float(np.abs(want).max())
    if path == "acc":
        g64, d64, (w64, _) = ts.backward(labels=labels, pixels=pixels, want_weights=True, dtype="f64")
        g32, d32, (w32, _) = ts.backward(labels=labels, pixels=pixels, want_weights=True, dtype="f32")
        out = dict(path=path, n=n, relmax_G=max(float(np.abs(a - b).max()) for a, b in zip(g32, g64)) / max(float(np.abs(b).max()) for b in g64),
                   relmax_G_site=max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g32, g64)),
                   relmax_dphi=float(np.abs(d32 - d64).max() / np.abs(d64).max()), relmax_w=float(np.abs(w32 - w64).max() / np.abs(w64).max()),
                   euler64=euler_of(d64, w64, False), euler32=euler_of(d32, w32, True))
        ts.close()
        print("RESULT " + json.dumps(out), flush=True)
        return
    if dtype == "f32" or (dtype == "f64" and root == ROOT):
        ts.set_option("gradient_dtype", 1 if dtype == "f32" else 0)

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
    if d is not None:                             # (phi of the bytes is (1, x / 255 / 255 / 4))
        out.update(euler=euler_of(d, w, dtype == "f32"), dphi_sum=float(np.abs(d).sum()))
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
    ap.add_argument("--dtype", default="", help="f64,f32: the second form, option gradient_dtype compared on the leg `both`")
    ap.add_argument("--parent", default="", help="second form: a checkout of the parent commit with tnml_amd/libtnml.so built; its fp64 legs are timed in the same alternation")
    ap.add_argument("--child-dtype", default="")
    ap.add_argument("--child-root", default=ROOT)
    ap.add_argument("--child-shape", default="%d,%d" % (N, M))
    a = ap.parse_args()
    if a.child:
        path, n = a.child.split(",")
        sites, bond = (int(v) for v in a.child_shape.split(","))
        child(path, int(n), a.chunk, a.child_dtype, a.child_root, sites, bond)
        return 0
    if a.dtype:
        if a.out == os.path.join(ROOT, "profiles", "backward_time.txt"):
            a.out = os.path.join(ROOT, "profiles", "backward_time_f32.txt")
        return main_dtype(a)
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


def main_dtype(a):
    """the second form (the module's header)"""
    dtypes = [d for d in a.dtype.split(",") if d]
    if any(d not in ("f64", "f32") for d in dtypes):
        print("--dtype takes f64, f32 or both")
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()

    def say(s):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    def leg(path, n, dtype="", root=ROOT, shape=(N, M)):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "%s,%d" % (path, n), "--chunk", str(a.chunk),
               "--child-dtype", dtype, "--child-root", root, "--child-shape", "%d,%d" % shape]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            say("leg %s %s n = %d failed (exit %d)\n%s\n%s" % (path, dtype, n, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            return None
        return json.loads(line[0][len("RESULT "):])

    def med(v):
        return sorted(v)[len(v) // 2]

    def spread(v, unit="s"):
        return "%.4f %s (min %.4f, max %.4f)" % (med(v), unit, min(v), max(v))
    kinds = [(d, ROOT) for d in dtypes] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
    say("streamed backward pass from bytes (labels mode, grad and dphi), N = %d, m = %d, option gradient_dtype; per leg one untimed call, one timed call; median (min, max) of %d legs%s"
        % (N, M, a.repeats, "; gradient_chunk = %d" % a.chunk if a.chunk else ""))
    classes = ("site_bwd", "site_grad", "input_grad", "pack")
    for n in (int(v) for v in a.n.split(",")):
        run = lambda kind, root: leg("both", n, "f64" if kind == "parent" else kind, root)
        if any(run(kind, root) is None for kind, root in kinds):             # warm-up of each, discarded
            return 1
        res = {kind: [] for kind, _ in kinds}
        for _ in range(a.repeats):
            for kind, root in kinds:
                r = run(kind, root)
                if r is None:
                    return 1
                res[kind].append(r)
        say("n = %d" % n)
        for kind, _ in kinds:
            name = "fp64 on the parent's build" if kind == "parent" else "gradient_dtype = %s" % kind
            say("  %-26s call %s; device bytes %d; launches %s" % (name, spread([r["seconds_call"] for r in res[kind]]), res[kind][0]["device_bytes"], json.dumps(res[kind][0]["launches"], sort_keys=True)))
            say("  %-26s kernel time per call: %s" % ("", ", ".join("%s %s" % (k, spread([r["kernel_ms"].get(k, 0.) for r in res[kind]], "ms")) for k in classes)))
        if "f64" in res and "f32" in res:
            say("  fp64 / fp32: call %.3f; %s; device bytes %.3f; Euler tie fp64 %.2e, fp32 %.2e" % (
                med([r["seconds_call"] for r in res["f64"]]) / med([r["seconds_call"] for r in res["f32"]]),
                ", ".join("%s %.3f" % (k, med([r["kernel_ms"][k] for r in res["f64"]]) / med([r["kernel_ms"][k] for r in res["f32"]])) for k in classes[:3]),
                res["f64"][0]["device_bytes"] / res["f32"][0]["device_bytes"], res["f64"][0]["euler"], res["f32"][0]["euler"]))
        if "f64" in res and "parent" in res:
            for k in ("call",) + classes[:3]:
                now = [r["seconds_call"] * 1e3 if k == "call" else r["kernel_ms"][k] for r in res["f64"]]
                par = [r["seconds_call"] * 1e3 if k == "call" else r["kernel_ms"][k] for r in res["parent"]]
                m_ = med(now)
                where = "inside" if min(par) <= m_ <= max(par) else ("%.4f ms above" % (m_ - max(par)) if m_ > max(par) else "%.4f ms below" % (min(par) - m_))
                say("  default path, %-10s now %s, parent %s: the median now lies %s the parent's min-max" % (k, spread(now, "ms"), spread(par, "ms"), where))
            same = res["f64"][0]["grad_sum"] == res["parent"][0]["grad_sum"] and res["f64"][0]["dphi_sum"] == res["parent"][0]["dphi_sum"] and res["f64"][0]["checksum"] == res["parent"][0]["checksum"]
            say("  default path, sums of |G|, |dphi| and |w| equal to the parent's: %s" % same)
        if "f64" in dtypes and "f32" in dtypes:
            r = leg("acc", n)
            if r is None:
                return 1
            say("  accuracy, fp32 against fp64 on the same inputs: relmax G %.2e of the largest element (worst site against its own largest: %.2e), relmax dphi %.2e, relmax w %.2e; Euler tie at sites 1, %d, %d: fp64 %.2e, fp32 %.2e"
                % (r["relmax_G"], r["relmax_G_site"], r["relmax_dphi"], r["relmax_w"], N // 2, N, r["euler64"], r["euler32"]))
    if "f32" in dtypes:
        shape = (64, 600)
        if leg("both", 256, "f32", ROOT, shape) is None:
            return 1
        big = [leg("both", 256, "f32", ROOT, shape) for _ in range(a.repeats)]
        if any(r is None for r in big):
            return 1
        say("fp32 only, N = %d, m = %d (fp64 refuses bonds above 512), 256 images: call %s; device bytes %d" % (shape[0], shape[1], spread([r["seconds_call"] for r in big]), big[0]["device_bytes"]))
        say("  kernel time per call: %s; Euler tie %.2e" % (", ".join("%s %s" % (k, spread([r["kernel_ms"].get(k, 0.) for r in big], "ms")) for k in classes), big[0]["euler"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
