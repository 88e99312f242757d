"""Cost of held-out evaluation during training (tnml_heldout_attach): bond updates/s at m = 120, fp64, N = 784, with and without a
held-out context attached, at two sizes:

  (a) 7 500 training + 1 250 held-out images -- the per-rank share of 60 000 / 10 000 images over 8 GPUs;
  (b) 60 000 training + 5 000 held-out images on one GPU.

    python tools/time_heldout.py [--steps 60] [--warmup 10] [--timeout 400] [--legs a,b]

Every leg runs in a child process of its own under `timeout`; a child that fails or hangs ends the tool (nothing more is started on
the GPU).  The sweep is timed as the fixedL driver runs it: pipelined (bond k+1 begun before bond k is ended) and, with a held-out
context, the held-out values of every bond read right after its end.  The warm-up bond updates bring the sweep to the 120 x 120 bonds
(bond 8 on).  When the two contexts of (b) do not fit into 0.97 x the free HBM by tnml_estimate_bytes, the training context gets an
`env_budget_mb` cap (its farthest environments live in host memory) and the tool says so; both runs of that size then use the same cap.
A last leg per size repeats the held-out run with the profile API on the held-out context (its own stream): the held-out kernels' time
per bond update by kernel class.  Separate from bench.py, which times training alone."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"a": (7500, 1250), "b": (60000, 5000)}
N, M = 784, 120


def child(nt, nh, with_ho, prof, budget_mb, steps, warmup):
    sys.path.insert(0, ROOT)
    from tnml_amd import lib, synth
    from tnml_amd.fixedl import TrainStates
    labels = synth.synthetic_labels(nt)
    ts = TrainStates(labels, N, M, pixels=synth.synthetic_images(N, labels), device=0)
    if budget_mb:
        ts.set_option("env_budget_mb", budget_mb)
    ts.set_mps(synth.random_mps(N, M, seed=1))
    ts.init()
    hs = None
    if with_ho:
        hl = synth.synthetic_labels(nh, seed=7)
        hs = TrainStates(hl, N, M, pixels=synth.synthetic_images(N, hl, seed=7), device=0)
        if prof:
            hs.profile(True)
        ts.attach_heldout(hs)
    sched, b, ha = [], 1, 1
    for _ in range(warmup + steps):
        sched.append((b, ha))
        b, ha = lib.sweepnext(b, ha, N)
    last = {}

    def run(part):
        for k, (bb, hh) in enumerate(part):
            ts.bond_update_begin(bb, hh, M, M, 1e-10, 4, 1e-3, 1e-10)
            if k > 0:
                last["rep"] = ts.bond_update_end()
                if hs is not None:
                    last["ho"] = ts.heldout_report()
        last["rep"] = ts.bond_update_end()
        if hs is not None:
            last["ho"] = ts.heldout_report()
    run(sched[:warmup])
    ts.synchronize()
    if hs is not None:
        hs.synchronize()
        if prof:
            hs.profile_reset()
    t0 = time.perf_counter()
    run(sched[warmup:])
    ts.synchronize()
    if hs is not None:
        hs.synchronize()
    dt = time.perf_counter() - t0
    out = dict(nt=nt, nh=nh if with_ho else 0, steps=steps, warmup=warmup, env_budget_mb=budget_mb, seconds=dt, bond_updates_per_s=steps / dt,
               ms_per_step=1e3 * dt / steps, bonds=[sched[warmup][0], sched[-1][0]], last_cost=last["rep"]["cost"] / nt,
               mL=last["rep"]["mL"], mR=last["rep"]["mR"])
    if hs is not None:
        h = last["ho"]
        out.update(heldout_bond=h["bond"], heldout_cost=h["cost"] / h["count"], heldout_ncorrect=h["ncorrect"])
        if prof:
            out["heldout_kernels_ms_per_step"] = {k: v[1] / steps for k, v in hs.profile_read().items() if v[0]}
            out["heldout_launches_per_step"] = {k: v[0] / steps for k, v in hs.profile_read().items() if v[0]}
        ts.detach_heldout()
        hs.close()
    ts.close()
    print("RESULT " + json.dumps(out), flush=True)


def plan_budget(nt, nh):
    """0 when both contexts fit into 0.97 x free HBM, otherwise the env_budget_mb that makes them fit"""
    sys.path.insert(0, ROOT)
    import ctypes as C
    from tnml_amd import lib
    f, t = C.c_int64(), C.c_int64()
    if lib.load().tnml_device_memory(0, C.byref(f), C.byref(t)) != 0:
        raise SystemExit("tnml_device_memory failed")
    budget = 0.97 * f.value
    need_t, need_h = lib.estimate_bytes(N, nt, M), lib.estimate_bytes(N, nh, M)
    info = dict(free_gb=f.value / 1e9, total_gb=t.value / 1e9, train_gb=need_t / 1e9, heldout_gb=need_h / 1e9)
    if need_t + need_h <= budget:
        return 0, info
    ntp = (nt + 255) // 256 * 256
    slab = 10 * M * ntp * 8
    env_t = (0.55 * N + 3) * slab                                   # the environment slabs of tnml_estimate_bytes
    room = budget - need_h - (need_t - env_t)
    return max(int(room / 2**20) - 2 * int(slab / 2**20), 1024), info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--child", default="")
    ap.add_argument("--plan", default="")
    a = ap.parse_args()
    if a.child:
        nt, nh, with_ho, prof, budget = (int(x) for x in a.child.split(","))
        child(nt, nh, with_ho, prof, budget, a.steps, a.warmup)
        return 0
    if a.plan:
        nt, nh = (int(x) for x in a.plan.split(","))
        budget, info = plan_budget(nt, nh)
        print("PLAN " + json.dumps(dict(info, env_budget_mb=budget)), flush=True)
        return 0

    def leg(args, what):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)] + args + ["--steps", str(a.steps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith(what)]
        if p.returncode != 0 or not line:
            print("leg %s failed (exit %d)\n%s\n%s" % (" ".join(args), p.returncode, p.stdout[-2000:], p.stderr[-2000:]), flush=True)
            return None
        return json.loads(line[0][len(what):])
    results = []
    for name in a.legs.split(","):
        nt, nh = SIZES[name]
        plan = leg(["--plan", "%d,%d" % (nt, nh)], "PLAN ")
        if plan is None:
            return 1
        budget = plan["env_budget_mb"]
        print("(%s) %d training + %d held-out images, m = %d, fp64: estimate %.1f + %.1f GB, %.1f GB free of %.1f%s"
              % (name, nt, nh, M, plan["train_gb"], plan["heldout_gb"], plan["free_gb"], plan["total_gb"],
                 "" if not budget else "; both do not fit: env_budget_gb = %.1f on the training context (both runs)" % (budget / 1024.)), flush=True)
        base = leg(["--child", "%d,%d,0,0,%d" % (nt, nh, budget)], "RESULT ")
        if base is None:
            return 1
        ho = leg(["--child", "%d,%d,1,0,%d" % (nt, nh, budget)], "RESULT ")
        if ho is None:
            return 1
        pr = leg(["--child", "%d,%d,1,1,%d" % (nt, nh, budget)], "RESULT ")
        if pr is None:
            return 1
        over = base["bond_updates_per_s"] / ho["bond_updates_per_s"] - 1.0
        kern = pr["heldout_kernels_ms_per_step"]
        print("(%s) without held-out: %.1f bond updates/s (%.3f ms); with: %.1f bond updates/s (%.3f ms): overhead %+.1f %%; bonds %d..%d, "
              "%d x %d; held-out cost %.6f, %d/%d correct"
              % (name, base["bond_updates_per_s"], base["ms_per_step"], ho["bond_updates_per_s"], ho["ms_per_step"], 100 * over,
                 base["bonds"][0], base["bonds"][1], base["mL"], base["mR"], ho["heldout_cost"], ho["heldout_ncorrect"], nh), flush=True)
        print("(%s) held-out kernels per bond update (profile API, held-out stream; events cost time of their own: %.1f bond updates/s "
              "in that run): %s = %.3f ms" % (name, pr["bond_updates_per_s"], ", ".join("%s %.3f" % kv for kv in sorted(kern.items())),
                                               sum(kern.values())), flush=True)
        results.append(dict(size=name, plan=plan, without=base, with_heldout=ho, profiled=pr, overhead=over))
    print(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
