"""What predicted splits (option spec_predict) buy or cost on the reference's default truncation: whole sweeps of the SURVEY.md 8(d)
settings -- N = 784, maxm = 120, minm = 60, cutoff = 1E-10, Npass = 4, lambda = 1E-3, fp64, random-init W at m = 120 -- at

  (a) 7 500 images -- the per-rank share of 60 000 images over 8 GPUs;
  (b) 60 000 images on one GPU,

with the option off and on.

    python tools/time_spec_predict.py [--sweeps 3] [--repeats 3] [--timeout 900] [--legs a,b]

Every leg runs in a child process of its own under `timeout`; a child that fails or hangs ends the tool (nothing more is started on
the GPU).  The legs of one size are interleaved (off, on, off, on, ...) so that drift of the machine hits both alike.  A sweep is
timed as the fixedL driver runs it: pipelined inside a sweep, nothing in flight across a sweep boundary.  The first sweep cannot
predict anything (a bond needs two finished visits); it is reported with the others, per sweep: bond updates/s, predicted and
mispredicted splits so far and the device time of the repeated work (tnml_spec_predict_stats), speculative splits and roll-backs of
every kind (tnml_split_stats).  The final cost of the off and on runs must agree to the last bit: the tool says so.  Separate from
bench.py, whose `--workload 8d` window times 60 interior bond updates of the second sweep."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"a": 7500, "b": 60000}
N, M = 784, 120
SWEEP = (M, M // 2, 1e-10, 4, 1e-3, 1e-10)          # maxm, minm, cutoff, Npass, lambda, cconv


def child(nt, on, sweeps):
    sys.path.insert(0, ROOT)
    from tnml_amd import lib, synth
    from tnml_amd.fixedl import TrainStates
    labels = synth.synthetic_labels(nt)
    ts = TrainStates(labels, N, M, pixels=synth.synthetic_images(N, labels), device=0)
    ts.set_option("spec_predict", on)
    ts.set_mps(synth.random_mps(N, M, seed=1))
    ts.init()
    ts.synchronize()
    per_sweep = []
    rep = None
    for sw in range(1, sweeps + 1):
        sched, b, ha = [], 1, 1
        while ha <= 2:
            sched.append((b, ha))
            b, ha = lib.sweepnext(b, ha, N)
        t0 = time.perf_counter()
        newm = []
        for k, (bb, hh) in enumerate(sched):
            ts.bond_update_begin(bb, hh, *SWEEP)
            if k > 0:
                rep = ts.bond_update_end()
                newm.append(rep["newm"])
        rep = ts.bond_update_end()
        newm.append(rep["newm"])
        ts.synchronize()
        dt = time.perf_counter() - t0
        per_sweep.append(dict(sweep=sw, bond_updates=len(sched), seconds=dt, bond_updates_per_s=len(sched) / dt, pred=ts.spec_predict_stats(),
                              split=ts.split_stats(), fallbacks=ts.svd_stats()["fallbacks"], newm_min=min(newm), newm_max=max(newm),
                              newm_median=sorted(newm)[len(newm) // 2], cost=rep["cost"] / nt))
    ts.close()
    print("RESULT " + json.dumps(dict(nt=nt, spec_predict=on, sweeps=per_sweep)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        nt, on = (int(x) for x in a.child.split(","))
        child(nt, on, a.sweeps)
        return 0

    def leg(nt, on):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "%d,%d" % (nt, on), "--sweeps", str(a.sweeps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("leg %d images, spec_predict = %d failed (exit %d)\n%s\n%s" % (nt, on, p.returncode, p.stdout[-2000:], p.stderr[-2000:]), flush=True)
            return None
        return json.loads(line[0][len("RESULT "):])
    results = []
    for name in a.legs.split(","):
        nt = SIZES[name]
        runs = {0: [], 1: []}
        for _ in range(a.repeats):
            for on in (0, 1):
                r = leg(nt, on)
                if r is None:
                    return 1
                runs[on].append(r)
        for sw in range(a.sweeps):
            for on in (0, 1):
                rates = [r["sweeps"][sw]["bond_updates_per_s"] for r in runs[on]]
                s = runs[on][-1]["sweeps"][sw]
                print("(%s) %d images, sweep %d, spec_predict = %d: %s bond updates/s (median %.1f, spread %.1f %%); predicted %d, mispredicted %d, "
                      "redo %.2f ms; speculative splits %d, roll-backs %d, solver fallbacks %d; new m %d..%d (median %d)"
                      % (name, nt, sw + 1, on, " / ".join("%.1f" % x for x in rates), sorted(rates)[len(rates) // 2],
                         100.0 * (max(rates) - min(rates)) / min(rates), s["pred"]["predicted"], s["pred"]["mispredicted"], s["pred"]["redo_ms"],
                         s["split"]["speculative_splits"], s["split"]["roll_backs"], s["fallbacks"], s["newm_min"], s["newm_max"], s["newm_median"]), flush=True)
        same = all(x["cost"] == y["cost"] for x, y in zip(runs[0][-1]["sweeps"], runs[1][-1]["sweeps"]))
        print("(%s) cost after every sweep, off against on: %s" % (name, "bit-identical" if same else "DIFFERENT"), flush=True)
        results.append(dict(size=name, images=nt, off=runs[0], on=runs[1], same_cost=same))
    print(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
