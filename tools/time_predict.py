"""Inference from bytes at N = 784, m = 120 (fp64): tnml_classify on a context that holds the images against tnml_predict_u8 on a
data-less context, for n = 256, 10 000 and 60 000 images.

    python tools/time_predict.py [--n 256,10000,60000] [--repeats 3] [--chunk C] [--timeout 300] [--out profiles/predict_time.txt]

Every leg runs in a child process of its own under `timeout`; a child that fails or hangs ends the tool (nothing more is started on
the GPU).  Per image count: one warm-up leg of each path (discarded), then the two paths alternated, `--repeats` legs each.  A leg
builds its context, makes one untimed call (code objects, first-touch allocations: the predict workspace is allocated there), times
one call, and repeats the call with the profile API on to count the launches by kernel class.
  classify leg: seconds of tnml_create + tnml_set_data_u8 (what a new image set costs that path), seconds of the tnml_classify call alone;
  predict leg:  seconds of the tnml_predict_u8 call alone (staging, chain kernel and copy back of every chunk); its context does not
                depend on the images.
The classify legs run code this tool's subject does not touch: they are the baseline.  No pass / fail time: the figures are written
down with the spread of the repeats."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 784, 120


def child(path, n, chunk=0):
    sys.path.insert(0, ROOT)
    import numpy as np
    from tnml_amd import synth
    from tnml_amd.fixedl import TrainStates
    labels = synth.synthetic_labels(n)
    pixels = np.ascontiguousarray(synth.synthetic_images(N, labels), dtype=np.uint8)
    W = synth.random_mps(N, M, seed=1)
    t0 = time.perf_counter()
    if path == "classify":
        ts = TrainStates(labels, N, M, pixels=pixels, device=0)
    else:
        ts = TrainStates(np.zeros(1, dtype=np.int32), N, M, no_data=True, device=0)
    ts.synchronize()
    t_ctx = time.perf_counter() - t0
    ts.set_mps(W)
    if chunk and path == "predict":
        ts.set_option("predict_chunk", chunk)

    def call():
        return ts.classify()[:2] if path == "classify" else ts.predict(pixels=pixels)
    call()
    ts.synchronize()
    t0 = time.perf_counter()
    w, pred = call()
    ts.synchronize()
    dt = time.perf_counter() - t0
    ts.profile(True)
    ts.profile_reset()
    call()
    prof = {k: v for k, v in ts.profile_read().items() if v[0]}
    ts.profile(False)
    out = dict(path=path, n=n, seconds_call=dt, images_per_s=n / dt, seconds_context=t_ctx, device_bytes=ts.device_bytes(),
               launches={k: v[0] for k, v in prof.items()}, kernel_ms={k: v[1] for k, v in prof.items()},
               checksum=float(np.abs(w).sum()), pred_hist=np.bincount(pred, minlength=10).tolist())
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="256,10000,60000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_time.txt"))
    ap.add_argument("--chunk", type=int, default=0, help="option predict_chunk of the predict legs (0: the library's default)")
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

    def spread(v):
        return "%.4f s (min %.4f, max %.4f)" % (sorted(v)[len(v) // 2], min(v), max(v))
    say("inference from bytes, N = %d, m = %d, fp64; per leg one untimed call, one timed call; median (min, max) of %d legs%s" % (N, M, a.repeats, "; predict_chunk = %d" % a.chunk if a.chunk else ""))
    rc = 0
    results = []
    for n in (int(x) for x in a.n.split(",")):
        if leg("classify", n) is None or leg("predict", n) is None:      # warm-up of each shape, discarded
            rc = 1
            break
        res = {"classify": [], "predict": []}
        for _ in range(a.repeats):
            for path in ("classify", "predict"):
                r = leg(path, n)
                if r is None:
                    rc = 1
                    break
                res[path].append(r)
            if rc:
                break
        if rc:
            break
        c, p = res["classify"], res["predict"]
        tc, tp, tx = [r["seconds_call"] for r in c], [r["seconds_call"] for r in p], [r["seconds_context"] for r in c]
        say("n = %d" % n)
        say("  tnml_classify   call %s = %.0f images/s; context + upload %s; launches %s; device bytes %d"
            % (spread(tc), n / sorted(tc)[len(tc) // 2], spread(tx), json.dumps(c[0]["launches"], sort_keys=True), c[0]["device_bytes"]))
        say("  tnml_predict_u8 call %s = %.0f images/s; context (data-less) %s; launches %s; device bytes %d"
            % (spread(tp), n / sorted(tp)[len(tp) // 2], spread([r["seconds_context"] for r in p]), json.dumps(p[0]["launches"], sort_keys=True), p[0]["device_bytes"]))
        say("  chain kernel %.3f ms, staging pre-kernel (class pack) %.3f ms per call; predictions agree: %s; sum |w| classify %.12e predict %.12e"
            % (p[0]["kernel_ms"].get("chain", 0.), p[0]["kernel_ms"].get("pack", 0.), c[0]["pred_hist"] == p[0]["pred_hist"], c[0]["checksum"], p[0]["checksum"]))
        med_c, med_p = sorted(tc)[len(tc) // 2], sorted(tp)[len(tp) // 2]
        say("  predict / classify (call alone) = %.2f; classify's own spread %.4f s; predict is %s"
            % (med_p / med_c, max(tc) - min(tc), "slower by more than that spread" if med_p - med_c > max(tc) - min(tc) else "not slower beyond that spread"))
        results.append(dict(n=n, classify=c, predict=p))
    with open(a.out, "a") as f:
        f.write(json.dumps(results) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
