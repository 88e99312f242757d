"""The device input map (tnml_set_input_map) against the fp64 feature path, feature = normal:

  leg a  data set-up for 60 000 x 784: host features (the drivers' all_features) + tnml_set_data_phi against map + tnml_set_data_u8
  leg b  predict at N = 784, m = 120 for 256, 10 000 and 60 000 images: tnml_predict_phi (host features counted, and not) against
         tnml_predict_u8 under a map
  leg c  the 28 -> 14 case (N = 196): both of the above for 60 000 images

    python tools/time_input_map.py [--legs a,b,c] [--n 256,10000,60000] [--repeats 3] [--timeout 300] [--out profiles/input_map_time.txt]

Every measurement runs in a child process of its own under `timeout`; a child that fails or hangs ends the tool (nothing more is started
on the GPU).  Per row: one warm-up child of each path (discarded), then the two paths alternated, `--repeats` children each.  A child
builds its context, makes one untimed call, times one call with a host clock around work that ends in a device synchronise, and repeats
the call with the profile API on for the launches and device milliseconds by kernel class.  No pass / fail time: the figures are
written down with the spread of the repeats."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 120


def child(what, path, n, imglen):
    sys.path.insert(0, ROOT)
    import numpy as np
    from tnml_amd import hostlib, synth
    from tnml_amd import lib as _lib
    from tnml_amd.fixedl import TrainStates
    from tnml_amd.input_map import InputMap
    labels = synth.synthetic_labels(n)
    raw = np.ascontiguousarray(synth.synthetic_images(784, labels), dtype=np.uint8)
    N = imglen * imglen
    out = dict(what=what, path=path, n=n, N=N)

    def host_features():                                    # what the drivers do without a map: reduce() + all_features on the host
        t0 = time.perf_counter()
        phi = hostlib.features(raw, "normal", imglen=0 if imglen == 28 else imglen)
        return phi, time.perf_counter() - t0

    def profiled(ts, call):
        ts.profile(True)
        ts.profile_reset()
        call()
        prof = {k: v for k, v in ts.profile_read().items() if v[0]}
        ts.profile(False)
        out["launches"] = {k: v[0] for k, v in prof.items()}
        out["kernel_ms"] = {k: v[1] for k, v in prof.items()}

    if what == "setup":
        ts = TrainStates(labels, N, 8, no_data=True, device=0)          # sized for the n images; the data go in below, timed
        lab = labels.ctypes.data_as(C.POINTER(C.c_int32))
        ts.synchronize()
        if path == "phi":
            phi, out["seconds_host"] = host_features()
            phi = np.ascontiguousarray(phi)

            def call():
                ts._ck(ts._L.tnml_set_data_phi(ts._h, _lib.dptr(phi), lab))
        else:
            t0 = time.perf_counter()
            m = InputMap.from_imglen(28, imglen, "normal")
            ts.set_input_map(m)
            out["seconds_host"] = time.perf_counter() - t0

            def call():
                ts._ck(ts._L.tnml_set_data_u8(ts._h, raw.ctypes.data_as(C.POINTER(C.c_uint8)), lab))
        call()
        ts.synchronize()
        t0 = time.perf_counter()
        call()
        ts.synchronize()
        out["seconds_call"] = time.perf_counter() - t0
        profiled(ts, call)
        out["checksum"] = 0.0
    else:
        W = synth.random_mps(N, M, seed=1)
        ts = TrainStates(np.zeros(1, dtype=np.int32), N, M, no_data=True, device=0)
        ts.set_mps(W)
        if path == "phi":
            phi, out["seconds_host"] = host_features()

            def call():
                return ts.predict(phi=phi)
        else:
            t0 = time.perf_counter()
            ts.set_input_map(InputMap.from_imglen(28, imglen, "normal"))
            out["seconds_host"] = time.perf_counter() - t0

            def call():
                return ts.predict(pixels=raw)
        call()
        ts.synchronize()
        t0 = time.perf_counter()
        w, pred = call()
        ts.synchronize()
        out["seconds_call"] = time.perf_counter() - t0
        profiled(ts, call)
        out["checksum"] = float(np.abs(w).sum())
        out["pred_hist"] = np.bincount(pred, minlength=10).tolist()
    out["device_bytes"] = ts.device_bytes()
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--n", default="256,10000,60000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_map_time.txt"))
    ap.add_argument("--append", action="store_true", help="keep what the output file already holds")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        what, path, n, imglen = a.child.split(",")
        child(what, path, int(n), int(imglen))
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not a.append:
        open(a.out, "w").close()

    def say(s):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    def run(what, path, n, imglen):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "%s,%s,%d,%d" % (what, path, n, imglen)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            say("child %s %s n = %d imglen = %d failed (exit %d)\n%s\n%s" % (what, path, n, imglen, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            return None
        return json.loads(line[0][len("RESULT "):])

    def med(v):
        return sorted(v)[len(v) // 2]

    def spread(v):
        return "%.4f s (min %.4f, max %.4f)" % (med(v), min(v), max(v))

    def ms(rows, k):
        v = [r["kernel_ms"].get(k, 0.) for r in rows]
        return "%.3f ms (min %.3f, max %.3f)" % (med(v), min(v), max(v))

    def row(what, n, imglen):
        """warm-up of each path, then the paths alternated; None once a child has failed"""
        if run(what, "phi", n, imglen) is None or run(what, "map", n, imglen) is None:
            return None
        res = {"phi": [], "map": []}
        for _ in range(a.repeats):
            for path in ("phi", "map"):
                r = run(what, path, n, imglen)
                if r is None:
                    return None
                res[path].append(r)
        return res

    legs = a.legs.split(",")
    ns = [int(x) for x in a.n.split(",")]
    results = []
    say("input map against the fp64 feature path, feature = normal, fp64; per child one untimed call, one timed call; median (min, max) of %d children" % a.repeats)
    plan = []
    if "a" in legs:
        plan.append(("a", "setup", 60000, 28))
    if "b" in legs:
        plan += [("b", "predict", n, 28) for n in ns]
    if "c" in legs:
        plan += [("c", "setup", 60000, 14), ("c", "predict", 60000, 14)]
    for leg, what, n, imglen in plan:
        res = row(what, n, imglen)
        if res is None:
            return 1
        f, m = res["phi"], res["map"]
        hf, hm = [r["seconds_host"] for r in f], [r["seconds_host"] for r in m]
        cf, cm = [r["seconds_call"] for r in f], [r["seconds_call"] for r in m]
        say("leg %s: %s, n = %d, 28 x 28 bytes -> N = %d%s" % (leg, "data set-up" if what == "setup" else "predict, m = %d" % M, n, imglen * imglen, "" if imglen == 28 else " (2 x 2 block means)"))
        if what == "setup":
            say("  host features + tnml_set_data_phi: host %s, call %s, together %.4f s; pack %s" % (spread(hf), spread(cf), med(hf) + med(cf), ms(f, "pack")))
            say("  input map + tnml_set_data_u8:      host (table + tnml_set_input_map) %s, call %s, together %.4f s; pack (stage + look-up) %s"
                % (spread(hm), spread(cm), med(hm) + med(cm), ms(m, "pack")))
        else:
            say("  tnml_predict_phi:            call %s = %.0f images/s; host features %s, together %.4f s; pack %s; chain %s; launches %s; device bytes %d"
                % (spread(cf), n / med(cf), spread(hf), med(hf) + med(cf), ms(f, "pack"), ms(f, "chain"), json.dumps(f[0]["launches"], sort_keys=True), f[0]["device_bytes"]))
            say("  tnml_predict_u8 under a map: call %s = %.0f images/s; host (table + tnml_set_input_map) %s; pack %s; chain %s; launches %s; device bytes %d"
                % (spread(cm), n / med(cm), spread(hm), ms(m, "pack"), ms(m, "chain"), json.dumps(m[0]["launches"], sort_keys=True), m[0]["device_bytes"]))
            same = f[0]["pred_hist"] == m[0]["pred_hist"] and f[0]["checksum"] == m[0]["checksum"]
            say("  same predictions and same sum |w| bit for bit: %s (%.17g against %.17g)" % (same, f[0]["checksum"], m[0]["checksum"]))
        results.append(dict(leg=leg, what=what, n=n, imglen=imglen, phi=f, map=m))
    with open(a.out, "a") as fh:
        fh.write(json.dumps(results) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
