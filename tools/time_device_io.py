"""Host pointers against device-resident tensors at N = 784, m = 120 (fp64), from features, coef mode, for n = 256 and 10 000 images:

  (a) TrainStates.backward in three forms -- grad alone, dphi alone, both -- with
        host     numpy arrays          (tnml_backward_phi: staged chunk by chunk, results copied back)
        device   torch CUDA tensors    (tnml_backward_dev: read and written where they lie)
        parent   numpy arrays on a checkout of the parent commit with its own library built (--parent DIR; left out when not given):
                 the host-pointer calls run through the code they now share with the device calls, and must not have become slower
  (b) one training step of MPSLayer(train_sites=True) under torch.optim.SGD -- forward, backward, optimiser step, sync_sites() -- with
        layer_cpu      CPU parameters, CPU phi
        layer_device   device parameters (MPSLayer(.., device="cuda")), device phi

    python tools/time_device_io.py [--n 256,10000] [--repeats 3] [--timeout 600] [--parent DIR] [--out profiles/device_io_time.txt]

Every leg runs in a child process of its own under `timeout`; a child that fails or hangs ends the tool (nothing more is started on
the GPU).  Per image count: one warm-up leg of each path (discarded), then the paths alternated, `--repeats` legs each.  A leg builds
its context, and per form makes one untimed call (code objects, first-touch allocations), times one call (the device synchronised
before and after), and repeats the call with the profile API on for the kernel time and the launches by class.
No pass / fail time: the figures are written down with the spread of the repeats.

--taped (needs --parent; writes profiles/taped_backward_time.txt): the backward from the forward's tape against the parent commit, features
on the device, n = 256 and 64 (--n), fp64 and fp32, the legs of this build and of the parent's alternated:
  (a) kernel time by class of forward_taped + backward_taped (fwd_taped, site_out, site_grad, input_grad) against the parent's
      predict + backward (chain, site_bwd, site_grad, input_grad);
  (b) one MPSLayer(train_sites=True, device="cuda") step under torch.optim.SGD, taped=True here against the parent's layer: wall and
      kernel time, sync_sites() apart;
  (c) the untouched calls predict, backward and gradient_step on both builds: the median now inside the parent's min-max, or by how much not."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 784, 120
FORMS = (("grad", True, False), ("dphi", False, True), ("both", True, True))
PATHS = ("host", "device", "parent", "layer_cpu", "layer_device")


def child(path, n, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from tnml_amd import synth
    from tnml_amd.fixedl import TrainStates
    rng = np.random.default_rng(3)
    labels = np.ascontiguousarray(synth.synthetic_labels(n), dtype=np.int32)
    pixels = synth.synthetic_images(N, labels)
    g = pixels.astype(np.float64) / 255.
    phi = np.ascontiguousarray(np.stack([np.ones_like(g), (g / 255.) / 4.], axis=-1))
    coef = rng.standard_normal((n, 10)) * 1e-3
    W = synth.random_mps(N, M, seed=1)
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, M, no_data=True, device=0)
    ts.set_mps(W)

    def host(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ts.profile(True)
        ts.profile_reset()
        fn()
        prof = {k: v for k, v in ts.profile_read().items() if v[0]}
        ts.profile(False)
        return out, dict(seconds_call=dt, launches={k: v[0] for k, v in prof.items()}, kernel_ms={k: v[1] for k, v in prof.items()})

    out = dict(path=path, n=n, forms={})
    if path in ("host", "device", "parent"):
        if path == "device":
            phi_a, coef_a = torch.from_numpy(phi).cuda(), torch.from_numpy(coef).cuda()
        else:
            phi_a, coef_a = phi, coef
        for form, sites, inputs in FORMS:
            (grads, dphi), r = timed(lambda: ts.backward(coef=coef_a, phi=phi_a, want_sites=sites, want_inputs=inputs))
            if grads is not None:
                r["grad_sum"] = float(sum(float(np.abs(host(a)).sum()) for a in grads))
            if dphi is not None:
                r["dphi_sum"] = float(np.abs(host(dphi)).sum())
            out["forms"][form] = r
    else:
        from tnml_amd.torch_layer import MPSLayer
        on_dev = path == "layer_device"
        layer = MPSLayer(ts, train_sites=True, device="cuda") if on_dev else MPSLayer(ts, train_sites=True)
        opt = torch.optim.SGD(layer.parameters(), lr=2.0 ** -20)
        x = torch.from_numpy(phi).cuda() if on_dev else torch.from_numpy(phi)
        go = torch.from_numpy(coef).cuda() if on_dev else torch.from_numpy(coef)

        def step():
            opt.zero_grad()
            o = layer(x)
            (o * go).sum().backward()
            opt.step()
            layer.sync_sites()
            return o
        o, r = timed(step)
        r["out_sum"] = float(np.abs(host(o)).sum())
        out["forms"]["step"] = r
    out["device_bytes"] = ts.device_bytes()
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def taped_child(build, n, root):
    """one leg of --taped: (a), (c) and (b) in fp64 and in fp32 on the package under root (build "parent": its API only)"""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from tnml_amd import synth
    from tnml_amd.fixedl import TrainStates
    from tnml_amd.torch_layer import MPSLayer
    rng = np.random.default_rng(3)
    labels = np.ascontiguousarray(synth.synthetic_labels(n), dtype=np.int32)
    g = synth.synthetic_images(N, labels).astype(np.float64) / 255.
    x = torch.from_numpy(np.ascontiguousarray(np.stack([np.ones_like(g), (g / 255.) / 4.], axis=-1))).cuda()
    coef = torch.from_numpy(rng.standard_normal((n, 10)) * 1e-3).cuda()
    W = synth.random_mps(N, M, seed=1)
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, M, no_data=True, device=0)
    ts.set_mps(W)
    now = build == "now"

    def timed(fn, extra=None):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ts.profile(True)
        ts.profile_reset()
        fn()
        prof = {k: v for k, v in ts.profile_read().items() if v[0]}
        ts.profile(False)
        return dict(seconds_call=dt, kernel_ms={k: v[1] for k, v in prof.items()}, **(extra() if extra else {}))

    out = dict(build=build, n=n, forms={})
    for dtype in ("f64", "f32"):
        def pair():
            if now:
                _, _, t = ts.forward_taped(phi=x, dtype=dtype)
                return ts.backward_taped(t, coef)
            ts.predict(phi=x, dtype=dtype)
            ts.set_option("predict_dtype", 0)
            return ts.backward(coef=coef, phi=x, dtype=dtype)

        def predict():
            ts.predict(phi=x, dtype=dtype)
            ts.set_option("predict_dtype", 0)
        out["forms"]["pair_" + dtype] = timed(pair)
        out["forms"]["predict_" + dtype] = timed(predict)
        out["forms"]["backward_" + dtype] = timed(lambda: ts.backward(coef=coef, phi=x, dtype=dtype))
        out["forms"]["gradient_step_" + dtype] = timed(lambda: ts.gradient_step(coef=coef, phi=x, lr=2.0 ** -40, dtype=dtype))
        ts.set_option("gradient_dtype", 0)
        kw = dict(taped=True) if now else {}
        layer = MPSLayer(ts, train_sites=True, device="cuda", compute_dtype=dtype, **kw)
        opt = torch.optim.SGD(layer.parameters(), lr=2.0 ** -20)
        sync = []

        def step():
            opt.zero_grad()
            (layer(x) * coef).sum().backward()
            opt.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            layer.sync_sites()
            torch.cuda.synchronize()
            sync.append(time.perf_counter() - t0)
        out["forms"]["step_" + dtype] = timed(step, lambda: dict(seconds_sync=sync[1]))
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def taped_main(a, say, med, spread):
    """the alternation and the report of --taped"""
    if not a.parent:
        say("--taped needs --parent DIR (a checkout of the parent commit with its library built)")
        return 1

    def leg(build, n):
        root = os.path.abspath(a.parent) if build == "parent" else ROOT
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--taped-child", "%s,%d,%s" % (build, n, root)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            say("leg %s n = %d failed (exit %d)\n%s\n%s" % (build, n, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            return None
        print("  (leg %s, n = %d: done)" % (build, n), flush=True)
        return json.loads(line[0][len("RESULT "):])
    say("backward from the forward's tape against the parent commit; N = %d, m = %d, features on the device; per leg and form one untimed call, "
        "one timed call, one profiled call; median (min, max) of %d child processes per leg, this build and the parent's alternated" % (N, M, a.repeats))
    results = []
    for n in (int(v) for v in a.n.split(",")):
        res = {"now": [], "parent": []}
        for _ in range(a.repeats):
            for build in ("now", "parent"):
                r = leg(build, n)
                if r is None:
                    return 1
                res[build].append(r)
        say("n = %d" % n)
        for dtype in ("f64", "f32"):
            def col(build, form, key="seconds_call"):
                return [r["forms"][form + "_" + dtype][key] for r in res[build]]

            def kern(build, form, classes):
                return {k: [r["forms"][form + "_" + dtype]["kernel_ms"].get(k, 0.) for r in res[build]] for k in classes}
            ka, kp = kern("now", "pair", ("fwd_taped", "site_out", "site_grad", "input_grad")), kern("parent", "pair", ("chain", "site_bwd", "site_grad", "input_grad"))
            say("  %s (a) taped forward + backward, kernels: %s" % (dtype, ", ".join("%s %s" % (k, spread(v, "ms")) for k, v in ka.items())))
            say("  %s (a) parent predict + backward, kernels: %s" % (dtype, ", ".join("%s %s" % (k, spread(v, "ms")) for k, v in kp.items())))
            two_now, two_par = med(ka["fwd_taped"]) + med(ka["site_out"]), med(kp["chain"]) + med(kp["site_bwd"])
            say("  %s (a) fwd_taped + site_out = %.3f ms, chain + site_bwd = %.3f ms: %.2f of the parent's; site_out / site_bwd = %.2f; calls %s against %s"
                % (dtype, two_now, two_par, two_now / two_par, med(ka["site_out"]) / med(kp["site_bwd"]), spread(col("now", "pair")), spread(col("parent", "pair"))))
            for build in ("now", "parent"):
                ks = [sum(r["forms"]["step_" + dtype]["kernel_ms"].values()) for r in res[build]]
                say("  %s (b) layer step, %-6s: wall %s, kernels %s, of the wall time sync_sites %s" % (dtype, build, spread(col(build, "step")), spread(ks, "ms"), spread(col(build, "step", "seconds_sync"))))
            say("  %s (b) layer step: now / parent = %.2f" % (dtype, med(col("now", "step")) / med(col("parent", "step"))))
            for form in ("predict", "backward", "gradient_step"):
                h, p = col("now", form), col("parent", form)
                inside = min(p) <= med(h) <= max(p)
                off = (med(h) - max(p)) if med(h) > max(p) else (med(h) - min(p))
                say("  %s (c) %-13s now %s, parent %s: the median now lies %s the parent's min-max%s"
                    % (dtype, form, spread(h), spread(p), "inside" if inside else "outside", "" if inside else " by %+.4f s (%+.1f %%)" % (off, 100. * off / (max(p) if off > 0 else min(p)))))
        results.append(dict(n=n, **res))
    with open(a.out, "a") as f:
        f.write(json.dumps(results) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="256,10000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--parent", default="", help="a checkout of the parent commit with tnml_amd/libtnml.so built: its host-pointer legs are timed in the same alternation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_io_time.txt"))
    ap.add_argument("--child", default="")
    ap.add_argument("--taped", action="store_true", help="the legs of the backward from the forward's tape against --parent (see the header)")
    ap.add_argument("--taped-child", default="")
    a = ap.parse_args()
    if a.child:
        path, n, root = a.child.split(",", 2)
        child(path, int(n), root)
        return 0
    if a.taped_child:
        build, n, root = a.taped_child.split(",", 2)
        taped_child(build, int(n), root)
        return 0
    if a.taped and a.out == os.path.join(ROOT, "profiles", "device_io_time.txt"):
        a.out = os.path.join(ROOT, "profiles", "taped_backward_time.txt")
    if a.taped and a.n == "256,10000":
        a.n = "256,64"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    paths = [p for p in PATHS if p != "parent" or a.parent]

    def say(s):                                   # to the terminal and, line by line, to the output file
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    def leg(path, n):
        root = os.path.abspath(a.parent) if path == "parent" else ROOT
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "%s,%d,%s" % (path, n, root)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            say("leg %s n = %d failed (exit %d)\n%s\n%s" % (path, n, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            return None
        print("  (leg %s, n = %d: done)" % (path, n), flush=True)      # progress, to the terminal only
        return json.loads(line[0][len("RESULT "):])

    def med(v):
        return sorted(v)[len(v) // 2]

    def spread(v, unit="s"):
        return "%.4f %s (min %.4f, max %.4f)" % (med(v), unit, min(v), max(v))
    if a.taped:
        return taped_main(a, say, med, spread)
    say("host pointers against device-resident tensors, backward from features (coef mode) and one MPSLayer training step; N = %d, m = %d, fp64;"
        " per leg and form one untimed call, one timed call, one profiled call; median (min, max) of %d legs" % (N, M, a.repeats))
    results = []
    for n in (int(x) for x in a.n.split(",")):
        if any(leg(path, n) is None for path in paths):          # warm-up of each path, discarded
            return 1
        res = {path: [] for path in paths}
        for _ in range(a.repeats):
            for path in paths:
                r = leg(path, n)
                if r is None:
                    return 1
                res[path].append(r)
        say("n = %d" % n)
        for path in paths:
            for form in res[path][0]["forms"]:
                rows = [r["forms"][form] for r in res[path]]
                classes = sorted({k for r in rows for k in r["kernel_ms"]})
                ksum = [sum(r["kernel_ms"].values()) for r in rows]
                t = [r["seconds_call"] for r in rows]
                say("  %-12s %-5s call %s; kernels by class, summed: %s = %.3f of the call; launches %s"
                    % (path, form, spread(t), spread(ksum, "ms"), med(ksum) * 1e-3 / med(t), json.dumps(rows[0]["launches"], sort_keys=True)))
                say("  %-12s %-5s kernel time per call: %s" % ("", "", ", ".join("%s %s" % (k, spread([r["kernel_ms"].get(k, 0.) for r in rows], "ms")) for k in classes)))
        for form, _, _ in FORMS:
            h = [r["forms"][form]["seconds_call"] for r in res["host"]]
            d = [r["forms"][form]["seconds_call"] for r in res["device"]]
            kd = med([sum(r["forms"][form]["kernel_ms"].values()) for r in res["device"]]) * 1e-3
            say("  backward %-4s: host / device = %.2f; device call - its kernels = %.4f s (%.3f of the call)" % (form, med(h) / med(d), med(d) - kd, (med(d) - kd) / med(d)))
            same = all(res["host"][0]["forms"][form].get(k) == res["device"][0]["forms"][form].get(k) for k in ("grad_sum", "dphi_sum"))
            say("  backward %-4s: sum |G| and sum |dphi| agree between host and device arguments: %s" % (form, same))
            if a.parent:
                p = [r["forms"][form]["seconds_call"] for r in res["parent"]]
                inside = min(p) <= med(h) <= max(p)
                say("  backward %-4s: host-pointer call now %s, on the parent's build %s: the median now lies %s the parent's min-max%s"
                    % (form, spread(h), spread(p), "inside" if inside else "outside", "" if inside else " by %+.4f s (%+.1f %%)" % (
                        (med(h) - max(p)) if med(h) > max(p) else (med(h) - min(p)), 100. * ((med(h) - max(p)) / max(p) if med(h) > max(p) else (med(h) - min(p)) / min(p)))))
        c = [r["forms"]["step"]["seconds_call"] for r in res["layer_cpu"]]
        d = [r["forms"]["step"]["seconds_call"] for r in res["layer_device"]]
        say("  layer step: CPU parameters / device parameters = %.2f; outputs agree: %s" % (med(c) / med(d), res["layer_cpu"][0]["forms"]["step"]["out_sum"] == res["layer_device"][0]["forms"]["step"]["out_sum"]))
        results.append(dict(n=n, **res))
    with open(a.out, "a") as f:
        f.write(json.dumps(results) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
