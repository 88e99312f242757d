"""Inference from bytes at N = 784, m = 120 (fp64): tnml_classify on a context that holds the images against tnml_predict_u8 on a
data-less context, for n = 256, 10 000 and 60 000 images.

    python tools/time_predict.py [--n 256,10000,60000] [--repeats 3] [--chunk C] [--timeout 300] [--out profiles/predict_time.txt]
                                 [--dtype f64,f32] [--big N,m,n] [--evaluate]

--dtype f64,f32 adds a predict leg under option predict_dtype = 1 (the fp32 chain kernel) to the alternation, prints its chain time next
to the fp64 one, and ends with `--repeats` legs at a bond dimension the fp64 path refuses (--big, default N = 196, m = 600, n = 2048;
fp32 only; "" leaves them out); the default output is then profiles/predict_time_f32.txt.

--evaluate times tnml_evaluate_u8 (labels in, only the report back) against tnml_predict_u8 on the same images instead: the two
alternated, no classify legs; the default image count is then 10 000 and the default output profiles/evaluate_time.txt.

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


def child(path, n, chunk=0, N=N, M=M):
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
    if chunk and path in ("predict", "evaluate"):
        ts.set_option("predict_chunk", chunk)

    def call():
        if path == "evaluate":                    # only the report comes back: (report, None) in the place of (weights, pred)
            return ts.evaluate(labels, pixels=pixels), None
        return ts.classify()[:2] if path == "classify" else ts.predict(pixels=pixels)
    if path == "predict_f32":
        ts.set_option("predict_dtype", 1)
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
               launches={k: v[0] for k, v in prof.items()}, kernel_ms={k: v[1] for k, v in prof.items()})
    if path == "evaluate":
        out.update(ncorrect=w.ncorrect, cost=w.cost, pred_hist=w.confusion.sum(axis=0).tolist())
    else:
        out.update(checksum=float(np.abs(w).sum()), pred_hist=np.bincount(pred, minlength=10).tolist())
        if path == "predict":                     # what an evaluation of these images has to report
            out.update(ncorrect=int((pred == labels).sum()), cost=float(((w - np.eye(10)[labels]) ** 2).sum()))
    if path == "predict_f32" and M <= 512:        # the fp64 chain kernel on the same context: where do the two disagree
        w64, p64 = ts.predict(pixels=pixels, dtype="f64")
        top = np.sort(np.abs(w64), axis=1)
        gap = (top[:, -1] - top[:, -2]) / np.abs(w64).max()
        differ = pred != p64
        out.update(relmax_f64=float(np.abs(w - w64).max() / np.abs(w64).max()), pred_differ=int(differ.sum()),
                   largest_gap_where_differ=float(gap[differ].max()) if differ.any() else 0., smallest_gap=float(gap.min()))
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="")
    ap.add_argument("--evaluate", action="store_true", help="tnml_evaluate_u8 against tnml_predict_u8, alternated (default --n 10000)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default="")
    ap.add_argument("--dtype", default="f64", help="f64, or f64,f32: also the fp32 chain kernel (option predict_dtype)")
    ap.add_argument("--big", default="196,600,2048", help="N,m,n of the fp32-only legs at a bond dimension above 512 (with f32 in --dtype)")
    ap.add_argument("--chunk", type=int, default=0, help="option predict_chunk of the predict legs (0: the library's default)")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        f = a.child.split(",")
        child(f[0], int(f[1]), a.chunk, *[int(x) for x in f[2:]])
        return 0
    dtypes = a.dtype.split(",")
    if dtypes not in (["f64"], ["f64", "f32"]):
        ap.error("--dtype must be f64 or f64,f32")
    f32 = "f32" in dtypes
    if a.evaluate and f32:
        ap.error("--evaluate takes --dtype f64")
    a.n = a.n or ("10000" if a.evaluate else "256,10000,60000")
    a.out = a.out or os.path.join(ROOT, "profiles", "evaluate_time.txt" if a.evaluate else "predict_time_f32.txt" if f32 else "predict_time.txt")
    paths = ("predict", "evaluate") if a.evaluate else ("classify", "predict", "predict_f32") if f32 else ("classify", "predict")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()

    def say(s):                                   # to the terminal and, line by line, to the output file
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    def leg(path, n, shape=()):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", ",".join(str(x) for x in (path, n) + tuple(shape)), "--chunk", str(a.chunk)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            say("leg %s n = %d failed (exit %d)\n%s\n%s" % (path, n, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            return None
        return json.loads(line[0][len("RESULT "):])

    def spread(v):
        return "%.4f s (min %.4f, max %.4f)" % (sorted(v)[len(v) // 2], min(v), max(v))
    say("%s from bytes, N = %d, m = %d, %s; per leg one untimed call, one timed call; median (min, max) of %d legs%s"
        % ("tnml_evaluate_u8 against tnml_predict_u8" if a.evaluate else "inference", N, M, "fp64 and fp32 (option predict_dtype)" if f32 else "fp64", a.repeats, "; predict_chunk = %d" % a.chunk if a.chunk else ""))
    rc = 0
    results = []
    for n in (int(x) for x in a.n.split(",")):
        if any(leg(path, n) is None for path in paths):      # warm-up of each shape, discarded
            rc = 1
            break
        res = {path: [] for path in paths}
        for _ in range(a.repeats):
            for path in paths:
                r = leg(path, n)
                if r is None:
                    rc = 1
                    break
                res[path].append(r)
            if rc:
                break
        if rc:
            break
        if a.evaluate:
            p, e = res["predict"], res["evaluate"]
            tp, te = [r["seconds_call"] for r in p], [r["seconds_call"] for r in e]
            say("n = %d" % n)
            say("  tnml_predict_u8  call %s = %.0f images/s; launches %s; device bytes %d"
                % (spread(tp), n / sorted(tp)[len(tp) // 2], json.dumps(p[0]["launches"], sort_keys=True), p[0]["device_bytes"]))
            say("  tnml_evaluate_u8 call %s = %.0f images/s; launches %s; device bytes %d"
                % (spread(te), n / sorted(te)[len(te) // 2], json.dumps(e[0]["launches"], sort_keys=True), e[0]["device_bytes"]))
            say("  chain kernel %.3f ms under predict, %.3f ms under evaluate; tally kernel (class eval_tally) %.3f ms per call"
                % (p[0]["kernel_ms"].get("chain", 0.), e[0]["kernel_ms"].get("chain", 0.), e[0]["kernel_ms"].get("eval_tally", 0.)))
            med_p, med_e = sorted(tp)[len(tp) // 2], sorted(te)[len(te) // 2]
            say("  evaluate / predict (call alone) = %.3f; evaluate's median is %s predict's own min-max; ncorrect evaluate %d, from predict's output %d; cost %.12e, from predict's output %.12e"
                % (med_e / med_p, "inside" if min(tp) <= med_e <= max(tp) else "below" if med_e < min(tp) else "above", e[0]["ncorrect"], p[0]["ncorrect"], e[0]["cost"], p[0]["cost"]))
            results.append(dict(n=n, predict=p, evaluate=e))
            continue
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
        if f32:
            q = res["predict_f32"]
            tq = [r["seconds_call"] for r in q]
            k64, k32 = [r["kernel_ms"].get("chain", 0.) for r in p], [r["kernel_ms"].get("chain", 0.) for r in q]
            say("  tnml_predict_u8, predict_dtype = 1 (fp32): call %s = %.0f images/s; launches %s; device bytes %d"
                % (spread(tq), n / sorted(tq)[len(tq) // 2], json.dumps(q[0]["launches"], sort_keys=True), q[0]["device_bytes"]))
            say("  chain kernel fp64 %.3f ms (min %.3f, max %.3f), fp32 %.3f ms (min %.3f, max %.3f): fp64 / fp32 = %.2f; class pack under fp32 (staging + the fp32 copy of W) %.3f ms"
                % (sorted(k64)[len(k64) // 2], min(k64), max(k64), sorted(k32)[len(k32) // 2], min(k32), max(k32),
                   sorted(k64)[len(k64) // 2] / sorted(k32)[len(k32) // 2], q[0]["kernel_ms"].get("pack", 0.)))
            say("  fp32 against fp64 on the same context: relmax %.3e of max|w|; predictions differ on %d of %d images, whose fp64 top-two gap is at most %.3e of max|w| (smallest gap of all images %.3e); sum |w| fp32 %.12e"
                % (q[0]["relmax_f64"], q[0]["pred_differ"], n, q[0]["largest_gap_where_differ"], q[0]["smallest_gap"], q[0]["checksum"]))
            results.append(dict(n=n, classify=c, predict=p, predict_f32=q))
            continue
        results.append(dict(n=n, classify=c, predict=p))
    if f32 and a.big and not rc:
        bN, bM, bn = (int(x) for x in a.big.split(","))
        q = []
        for _ in range(a.repeats):
            r = leg("predict_f32", bn, (bN, bM))
            if r is None:
                rc = 1
                break
            q.append(r)
        if not rc:
            k32 = [r["kernel_ms"].get("chain", 0.) for r in q]
            tq = [r["seconds_call"] for r in q]
            say("N = %d, m = %d (above the fp64 path's 512), n = %d, predict_dtype = 1 only" % (bN, bM, bn))
            say("  tnml_predict_u8 call %s = %.0f images/s; chain kernel %.3f ms (min %.3f, max %.3f); class pack %.3f ms; launches %s; device bytes %d"
                % (spread(tq), bn / sorted(tq)[len(tq) // 2], sorted(k32)[len(k32) // 2], min(k32), max(k32), q[0]["kernel_ms"].get("pack", 0.),
                   json.dumps(q[0]["launches"], sort_keys=True), q[0]["device_bytes"]))
            results.append(dict(n=bn, N=bN, m=bM, predict_f32=q))
    with open(a.out, "a") as f:
        f.write(json.dumps(results) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
