"""Gradient steps from bytes at N = 784, m = 120 (fp64), labels mode, Adam: the step on the device (tnml_site_step_u8) against the
host path it replaces (tnml_site_gradient_u8, the update of tests/sitestep_model.py in numpy, tnml_set_site on every site) and against
a plain tnml_site_gradient_u8 call on the same images, on the same data-less context, for n = 256 and 512 images.

    python tools/time_site_step.py [--n 256,512] [--repeats 3] [--timeout 300] [--out profiles/site_step_time.txt]

Every leg runs in a child process of its own under `timeout`; a child that fails or hangs ends the tool (nothing more is started on
the GPU).  Per image count: one warm-up leg of each path (discarded), then the paths alternated, `--repeats` legs each.  A leg builds
its context and takes three steps (calls) from the same start: the first untimed (code objects, first-touch allocations: workspace
and optimiser state are allocated there), the second timed, the third with the profile API on for the kernel time by class.  The
device and the host legs report a digest of W after their three steps: the two must agree bit for bit, the host path being the model
the device is tested against.  No pass / fail time: the figures are written down with the spread of the repeats.

    python tools/time_site_step.py --loss quadratic,softmax [--loss-beta 8] [--n 256] [--out profiles/site_step_loss_time.txt]

times the device step alone under each of the named losses (option loss; softmax: the cross-entropy of tnml_amd/csrc/loss_dev.h), the
losses alternated leg by leg as the paths are above.  A loss may be named twice: the two series of legs then show the spread of one
and the same code."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 784, 120
LR = 1e-3
PATHS = ("gradient", "host", "device")


def child(path, n, loss="quadratic", beta=1.0):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import sitestep_model as st
    from tnml_amd import synth
    from tnml_amd.fixedl import TrainStates
    labels = np.ascontiguousarray(synth.synthetic_labels(n), dtype=np.int32)
    pixels = np.ascontiguousarray(synth.synthetic_images(N, labels), dtype=np.uint8)
    W = synth.random_mps(N, M, seed=1)
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, M, no_data=True, device=0)
    ts.set_mps(W)
    if loss != "quadratic":
        ts.set_loss(loss, beta)
    box = dict(W=W, state=None, rep=None)

    def call():
        if path == "gradient":
            ts.site_gradient(labels=labels, pixels=pixels)
        elif path == "device":
            box["rep"] = ts.gradient_step(labels=labels, pixels=pixels, method="adam", lr=LR, scale=1. / n)
        else:
            g = st.flat(ts.site_gradient(labels=labels, pixels=pixels))
            if box["state"] is None:
                box["state"] = st.new_state("adam", g.size)
            box["W"], box["state"], box["rep"] = st.step(box["W"], g, box["state"], method="adam", lr=LR, scale=1. / n)
            ts.set_mps(box["W"])
    call()
    ts.synchronize()
    t0 = time.perf_counter()
    call()
    ts.synchronize()
    dt = time.perf_counter() - t0
    ts.profile(True)
    ts.profile_reset()
    call()
    prof = {k: v for k, v in ts.profile_read().items() if v[0]}
    ts.profile(False)
    out = dict(path=path, n=n, loss=loss, seconds_call=dt, device_bytes=ts.device_bytes(), launches={k: v[0] for k, v in prof.items()},
               kernel_ms={k: v[1] for k, v in prof.items()})
    if path != "gradient":
        h = hashlib.sha256()
        for A in ts.get_mps():
            h.update(np.ascontiguousarray(A.ravel(order="F")).tobytes())
        rep = box["rep"]
        out.update(digest=h.hexdigest(), grad_norm=rep.grad_norm if path == "device" else rep["grad_norm"], t=rep.t if path == "device" else rep["t"])
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="256,512")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_step_time.txt"))
    ap.add_argument("--loss", default="", help="comma-separated losses: time the device step under each, alternated")
    ap.add_argument("--loss-beta", type=float, default=8.0)
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        path, n, loss = a.child.split(",")
        child(path, int(n), loss, a.loss_beta)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()

    def say(s):                                   # to the terminal and, line by line, to the output file
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    def leg(path, n, loss="quadratic"):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--loss-beta", repr(a.loss_beta), "--child", "%s,%d,%s" % (path, n, loss)]
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

    def kernels(legs, classes):
        return "; ".join("%s %s" % (k, spread([r["kernel_ms"].get(k, 0.) for r in legs], "ms")) for k in classes)
    if a.loss:
        return loss_legs(a, say, leg, spread, kernels)
    say("gradient steps from bytes (labels mode, Adam, lr = %g, scale = 1 / n), N = %d, m = %d, fp64: tnml_site_step_u8 against site_gradient + numpy update + set_mps "
        "and against a plain tnml_site_gradient_u8 call; per leg three steps from the same start: one untimed, one timed, one profiled; median (min, max) of %d legs"
        % (LR, N, M, a.repeats))
    results = []
    for n in (int(x) for x in a.n.split(",")):
        if any(leg(path, n) is None for path in PATHS):       # warm-up of each path, discarded
            return 1
        res = {path: [] for path in PATHS}
        for _ in range(a.repeats):
            for path in PATHS:
                r = leg(path, n)
                if r is None:
                    return 1
                res[path].append(r)
        g, h, d = res["gradient"], res["host"], res["device"]
        tg, th, td = ([r["seconds_call"] for r in x] for x in (g, h, d))
        ksum = [sum(r["kernel_ms"].values()) for r in d]
        say("n = %d" % n)
        say("  tnml_site_gradient_u8 (no step)  call %s; launches %s; device bytes %d" % (spread(tg), json.dumps(g[0]["launches"], sort_keys=True), g[0]["device_bytes"]))
        say("  host path                        step %s; launches %s; device bytes %d" % (spread(th), json.dumps(h[0]["launches"], sort_keys=True), h[0]["device_bytes"]))
        say("  tnml_site_step_u8                step %s; launches %s; device bytes %d" % (spread(td), json.dumps(d[0]["launches"], sort_keys=True), d[0]["device_bytes"]))
        say("  kernel time per device step: %s" % kernels(d, ("pack", "site_bwd", "site_grad", "eval_tally", "step_norm", "site_step")))
        say("  sum of the kernel classes %s; step - kernels = %.4f ms (staging copies, launches, table uploads, synchronisations, the report)"
            % (spread(ksum, "ms"), med(td) * 1e3 - med(ksum)))
        say("  device step / plain gradient call = %.3f; device step / host path = %.4f; optimiser state and tallies on the device: %d bytes"
            % (med(td) / med(tg), med(td) / med(th), d[0]["device_bytes"] - g[0]["device_bytes"]))
        same = len({r["digest"] for r in h + d}) == 1
        say("  W after three steps, device against host path: %s (t = %d, grad_norm of the third step %.17g device, %.17g host)"
            % ("bit for bit the same" if same else "DIFFERENT", d[0]["t"], d[0]["grad_norm"], h[0]["grad_norm"]))
        results.append(dict(n=n, gradient=g, host=h, device=d, same=same))
    with open(a.out, "a") as f:
        f.write(json.dumps(results) + "\n")
    return 0


def loss_legs(a, say, leg, spread, kernels):
    """--loss: the device step under each named loss (series k of the list: a loss named twice gives two series), alternated"""
    losses = a.loss.split(",")
    say("gradient steps from bytes (labels mode, Adam, lr = %g, scale = 1 / n), N = %d, m = %d, fp64: tnml_site_step_u8 under option loss = %s (loss_beta = %g), "
        "the series alternated leg by leg; per leg three steps from the same start: one untimed, one timed, one profiled; median (min, max) of %d legs"
        % (LR, N, M, " | ".join(losses), a.loss_beta, a.repeats))
    results = []
    for n in (int(x) for x in a.n.split(",")):
        if any(leg("device", n, loss) is None for loss in dict.fromkeys(losses)):      # warm-up of each loss, discarded
            return 1
        res = [[] for _ in losses]
        for _ in range(a.repeats):
            for k, loss in enumerate(losses):
                r = leg("device", n, loss)
                if r is None:
                    return 1
                res[k].append(r)
        say("n = %d" % n)
        for k, loss in enumerate(losses):
            say("  series %d, loss = %-9s  step %s; kernels: %s" % (k, loss, spread([r["seconds_call"] for r in res[k]]), kernels(res[k], ("site_bwd", "site_grad", "eval_tally", "step_norm", "site_step"))))
        results.append(dict(n=n, losses=losses, legs=res))
    with open(a.out, "a") as f:
        f.write(json.dumps(results) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
