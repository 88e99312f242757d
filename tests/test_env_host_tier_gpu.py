"""The host tier of the environments (option env_budget_mb; tnml_env.hip: env_spill, env_fetch, slot_acquire, env_evict_slab,
env_lookahead) on every path that moves environments while kernels are in flight.  include/tnml.h promises "Results do not depend
on the budget".  Two yardsticks, both wherever they apply:

 1. the resident run -- the same calls in the same order with env_budget_mb left at 0 -- bit for bit: every report field (cost, newm,
    ncorrect, truncerr, the CG cost trace, held-out cost and #correct), every site tensor, every environment that is built at the end.
    The tier only copies bytes, so there is no tolerance.
 2. the oracle, for the environments themselves (two runs that read the same wrong buffer would pass 1.): a full sweep ends at bond 1
    of half 2, the environments of sites 3..N are then the right environments of the final W -- those of an oracle given that W.

Every budgeted run also proves from env_stats() that the tier did something: slabs <= cap, spills and fetches above a floor, and the
resident run allocated at least twice the cap without a spill.  Every case prints its numbers (run with -s to see them).

Base shape: 24 sites, 300 images (padded to 512), m = 12: a slab (one Label-carrying environment) is 10 x 12 x 512 doubles = 480 KiB,
env_budget_mb = 2 holds four, the resident chain takes at least eight.  With fp32-stored environments a slab is 240 KiB: env_budget_mb = 1."""
import functools
import hashlib

import numpy as np
import pytest

from conftest import make_problem
from test_gpu_parity import TOL, _relmax

pytestmark = pytest.mark.gpu

N, NT, M = 24, 300, 12
TRUNC, SPEC = M // 2, M                  # minm: a truncating sweep (every split synchronous) / minm = maxm (speculative splits)
NSPEC = 2 * (N - 1) - 4                  # speculative splits of one sweep with minm = maxm: the four chain-end splits are 2 x 2 and go to the stock solver
NS, MS, TARGET = 80, 6, 3                # the per-label chain: 80 units of one tenth of a slab (10 x 6 x 512 doubles = 240 KiB) = 8 slabs, the cap of 1 MiB is 4


@functools.lru_cache(maxsize=None)
def _problem(u8=False):
    """(pixels, labels, phi, W) of the base shape; u8: the features the device makes of the bytes (no boost)"""
    pixels, labels, phi, W = make_problem(N, NT, M, 11, pixel_boost=1.0 if u8 else 200.0)
    if u8:
        from oracle import pyoracle
        phi = pyoracle.features_series(pixels)
    return pixels, labels, phi, W


@functools.lru_cache(maxsize=None)
def _heldout_problem():
    return make_problem(N, 100, M, 12, pixel_boost=200.0)


@functools.lru_cache(maxsize=None)
def _single_problem():
    pixels, labels, phi, W = make_problem(NS, NT, MS, 5, pixel_boost=200.0)
    return pixels, labels, phi, [A[..., 0] if A.ndim == 4 else A for A in W]


def _budget_mb(dtype):
    return 2 if dtype == "f64" else 1


def _cap(budget_mb, maxm, nt, dtype="f64"):
    """whole slabs of 10 x maxm x (nt padded to 256) environment elements that fit the budget"""
    return (budget_mb << 20) // (10 * maxm * (-(-nt // 256) * 256) * (8 if dtype == "f64" else 4))


def _sweep(minm, maxm=M):
    """maxm, minm, cutoff, Npass, lambda, cconv (nsweep goes in front)"""
    return (maxm, minm, 1e-10, 3, 1e-3, 1e-10)


def _ctx(prob, maxm=M, dtype="f64", u8=False, single=None, budget=0, env_async=1, options=()):
    from tnml_amd.fixedl import TrainStates
    pixels, labels, phi, W = prob
    ts = TrainStates(labels, phi.shape[1], maxm, pixels=pixels if u8 else None, phi=None if u8 else phi, dtype=dtype, single_label=single)
    ts.set_option("env_budget_mb", budget)
    ts.set_option("env_async", env_async)                  # 1: evictions and look-ahead copies on a second stream; 0: on the compute stream
    for k, v in options:
        ts.set_option(k, v)
    return ts


def _envs(ts):
    from tnml_amd.fixedl import TnmlError
    out = {}
    for j in range(1, ts.N + 1):
        try:
            out[j] = ts.env(j)
        except TnmlError:                                  # never built
            pass
    return out


def _record(ts, reps, hs=None):
    """everything the yardsticks read; the statistics are taken before the environments are read back (reading them fetches too)"""
    ts.synchronize()
    rec = dict(reps=reps, stats=ts.env_stats(), dev=ts.device_bytes(), svd=ts.svd_stats(), split=ts.split_stats(), pred=ts.spec_predict_stats(),
               W=ts.get_mps(), envs=_envs(ts))
    rec["stats_end"] = ts.env_stats()
    if hs is not None:
        rec["hstats"] = hs.env_stats()
    return rec


def _assert_identical(a, b, tag=None):
    """yardstick 1: == and np.array_equal, nothing else"""
    assert [(r["bond"], r["half"]) for r in a["reps"]] == [(r["bond"], r["half"]) for r in b["reps"]], tag
    for x, y in zip(a["reps"], b["reps"]):
        at = (tag, x["bond"], x["half"])
        for f in ("cost", "newm", "ncorrect", "truncerr"):
            assert x[f] == y[f], at + (f, x[f], y[f])
        assert x["cg"]["cost"] == y["cg"]["cost"], at
        assert ("heldout" in x) == ("heldout" in y), at
        if "heldout" in x:
            for f in ("bond", "half", "count", "cost", "ncorrect"):
                assert x["heldout"][f] == y["heldout"][f], at + ("heldout", f, x["heldout"][f], y["heldout"][f])
    assert len(a["W"]) == len(b["W"])
    for j, (x, y) in enumerate(zip(a["W"], b["W"]), start=1):
        assert np.array_equal(x, y), (tag, "site", j)
    assert a["envs"].keys() == b["envs"].keys(), tag
    for j in a["envs"]:
        assert np.array_equal(a["envs"][j], b["envs"][j]), (tag, "environment", j)


def _assert_tier_worked(tag, tight, free, cap, floor=0, key="stats"):
    """conditions, not measurements: a run that does not meet them tests nothing"""
    st, fr = tight[key], free[key]
    print("ENVSTATS %s: cap %d, budgeted slabs %d spills %d fetches %d host_bytes %d; resident slabs %d spills %d"
          % (tag, cap, st["slabs"], st["spills"], st["fetches"], st["host_bytes"], fr["slabs"], fr["spills"]))
    assert st["slabs"] <= cap, (tag, st)
    assert st["spills"] > floor and st["fetches"] > floor, (tag, st)
    assert fr["spills"] == 0 and fr["slabs"] >= 2 * cap, (tag, fr)
    if key == "stats":
        assert tight["stats_end"]["slabs"] <= cap, (tag, tight["stats_end"])        # reading the environments back kept to the cap too


_ORACLE_ENVS = {}


def _assert_envs_are_the_oracles(tag, rec, prob, dtype, single=None):
    """yardstick 2.  The gate is TOL[dtype]["E"] of test_gpu_parity.py (1e-12 for fp64, 5e-6 for fp32-stored environments) times N / 12:
    that tolerance was set for the 12-site chain of test_envs_after_init, and the rounding error of a shifted environment grows with the
    number of shifts behind it."""
    from oracle import pyoracle
    pixels, labels, phi, _ = prob
    n = phi.shape[1]
    h = hashlib.sha1(phi.tobytes())
    for A in rec["W"]:
        h.update(np.ascontiguousarray(A).tobytes())
    key = (h.hexdigest(), single)
    if key not in _ORACLE_ENVS:                            # (runs that must agree bit for bit end at the same W: one oracle for all of them)
        o = pyoracle.Oracle(phi, labels) if single is None else pyoracle.SingleOracle(phi, labels, single)
        o.set_mps(rec["W"])
        o.init()
        _ORACLE_ENVS[key] = {j: o.env(j) for j in range(3, n + 1)}
    ref = _ORACLE_ENVS[key]
    gate = TOL[dtype]["E"] * n / 12
    worst = 0.0
    for j in range(3, n + 1):
        assert rec["envs"][j].shape == ref[j].shape, (tag, j)
        err = _relmax(rec["envs"][j], ref[j])
        worst = max(worst, err)
        assert err < gate, (tag, "environment", j, err, gate)
    print("ENVORACLE %s: worst environment error %.2e, gate %.2e" % (tag, worst, gate))


def _run(dtype="f64", pipelined=False, minm=TRUNC, nsweep=2, u8=False, budget=0, env_async=1, options=()):
    from tnml_amd.fixedl import mldmrg
    prob = _problem(u8)
    ts = _ctx(prob, dtype=dtype, u8=u8, budget=budget, env_async=env_async, options=options)
    ts.set_mps(prob[3])
    ts.init()
    reps = mldmrg(ts, nsweep, *_sweep(minm), pipelined=pipelined)
    rec = _record(ts, reps)
    ts.close()
    return rec


@functools.lru_cache(maxsize=None)
def _resident_cached(dtype, pipelined, minm, nsweep, u8, env_async, options):
    return _run(dtype, pipelined, minm, nsweep, u8, 0, env_async, options)


def _resident(dtype="f64", pipelined=False, minm=TRUNC, nsweep=2, u8=False, env_async=1, options=()):
    """the resident run of the same calls, made once for all the cases that share it"""
    return _resident_cached(dtype, pipelined, minm, nsweep, u8, env_async, options)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. sweeps on one rank
def _sweeps_case(dtype, pipelined, minm, env_async, u8=False):
    tag = "sweeps %s %s minm=%d env_async=%d%s" % (dtype, "pipelined" if pipelined else "sequential", minm, env_async, " u8" if u8 else "")
    free = _resident(dtype, pipelined, minm, 2, u8, env_async)
    tight = _run(dtype, pipelined, minm, 2, u8, _budget_mb(dtype), env_async)
    _assert_tier_worked(tag, tight, free, _cap(_budget_mb(dtype), M, NT, dtype), floor=20)
    assert tight["dev"] < free["dev"]
    assert tight["split"]["speculative_splits"] == free["split"]["speculative_splits"]
    # minm = m: every split but the 2 x 2 ones at the chain ends is speculative; minm = m / 2: only those near the chain ends that keep fewer columns than minm
    assert (tight["split"]["speculative_splits"] >= 2 * NSPEC) if minm == SPEC else (tight["split"]["speculative_splits"] < NSPEC // 2)
    _assert_identical(tight, free, tag)
    if dtype in TOL:
        _assert_envs_are_the_oracles(tag + " resident", free, _problem(u8), dtype)
        _assert_envs_are_the_oracles(tag, tight, _problem(u8), dtype)


@pytest.mark.parametrize("dtype", ["f64", "f64_e32"])
@pytest.mark.parametrize("env_async", [1, 0])
@pytest.mark.parametrize("minm", [TRUNC, SPEC], ids=["truncating", "speculative"])
@pytest.mark.parametrize("pipelined", [False, True], ids=["sequential", "pipelined"])
def test_sweeps_under_a_budget_are_the_resident_sweeps(pipelined, minm, env_async, dtype):
    """two sweeps under a budget of four slabs.  minm = m: the splits are speculative, tnml_bond_update_begin does not synchronise the
    host and the evictions of env_lookahead run beside a whole bond update; pipelined: the plan of the bond update in flight holds raw
    environment addresses while `begin` of the next one evicts; f64_e32: four-byte elements in the slab arithmetic"""
    _sweeps_case(dtype, pipelined, minm, env_async)


def test_sweeps_under_a_budget_with_fp32_arithmetic():
    """dtype f32: four-byte environments and the fp32 kernels; its CG is not expected to track the oracle, so yardstick 1 only"""
    _sweeps_case("f32", True, TRUNC, 1)


def test_sweeps_under_a_budget_on_byte_input():
    """the context is fed `pixels` (u8) and makes the features on the device; the oracle gets features_series of the same bytes"""
    _sweeps_case("f64", True, SPEC, 1, u8=True)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. roll-backs under a budget
@pytest.mark.parametrize("which", ["first", "interior", "last"])
@pytest.mark.parametrize("pipelined", [False, True], ids=["sequential", "pipelined"])
def test_a_failed_split_check_rolls_back_under_a_budget(pipelined, which):
    """debug_fail_split: the k-th speculative split reports a failed check; redo_bond_updates drops the bond update and the one begun
    after it -- with the copy stream in existence and its spills and look-ahead fetches in flight -- and repeats both"""
    fail = dict(first=0, interior=NSPEC // 2, last=NSPEC - 1)[which]
    tag = "failed split %d %s" % (fail, "pipelined" if pipelined else "sequential")
    plain = _resident("f64", pipelined, SPEC, 1)
    assert plain["split"]["speculative_splits"] == NSPEC and plain["split"]["roll_backs"] == 0
    hook = (("debug_fail_split", fail),)
    free = _resident("f64", pipelined, SPEC, 1, options=hook)
    tight = _run("f64", pipelined, SPEC, 1, budget=2, options=hook)
    _assert_tier_worked(tag, tight, free, _cap(2, M, NT))
    assert free["split"]["roll_backs"] >= 1 and free["svd"]["fallbacks"] >= plain["svd"]["fallbacks"] + 1
    assert tight["svd"]["fallbacks"] == free["svd"]["fallbacks"]
    assert (tight["split"]["speculative_splits"], tight["split"]["roll_backs"]) == (free["split"]["speculative_splits"], free["split"]["roll_backs"])
    _assert_identical(tight, free, tag)
    # against the run without the hook: the repeat takes the synchronous split, so costs agree to rounding only (the bound of
    # test_speculative_split_and_its_roll_back)
    assert [(r["bond"], r["newm"]) for r in tight["reps"]] == [(r["bond"], r["newm"]) for r in plain["reps"]]
    np.testing.assert_allclose([r["cost"] for r in tight["reps"]], [r["cost"] for r in plain["reps"]], rtol=1e-8)
    _assert_envs_are_the_oracles(tag, tight, _problem(), "f64")


@pytest.mark.parametrize("pipelined", [False, True], ids=["sequential", "pipelined"])
def test_a_mispredicted_split_rolls_back_under_a_budget(pipelined):
    """spec_predict = 1 on a truncating sweep: a split runs speculatively on the column count its bond kept at its last two visits (so
    only from the second sweep on); debug_mispredict moves the guess of an interior predicted split.  Every number is that of the run
    without the option and without a budget."""
    tag = "mispredicted split %s" % ("pipelined" if pipelined else "sequential")
    sync = _resident("f64", pipelined, TRUNC, 2)
    base = _resident("f64", pipelined, TRUNC, 2, options=(("spec_predict", 1),))
    npred = base["pred"]["predicted"]
    assert npred >= 3, base["pred"]
    hook = (("spec_predict", 1), ("debug_mispredict", npred // 2))
    free = _resident("f64", pipelined, TRUNC, 2, options=hook)
    tight = _run("f64", pipelined, TRUNC, 2, budget=2, options=hook)
    _assert_tier_worked(tag, tight, free, _cap(2, M, NT), floor=20)
    print("ENVSTATS %s: predicted %s" % (tag, tight["pred"]))
    assert tight["pred"]["predicted"] >= 1 and tight["pred"]["mispredicted"] == base["pred"]["mispredicted"] + 1
    assert (tight["pred"]["predicted"], tight["pred"]["mispredicted"]) == (free["pred"]["predicted"], free["pred"]["mispredicted"])
    assert tight["split"]["roll_backs"] == free["split"]["roll_backs"] >= 1
    _assert_identical(tight, free, tag)
    _assert_identical(tight, sync, tag + " against spec_predict = 0")
    _assert_envs_are_the_oracles(tag, tight, _problem(), "f64")


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. the per-label variant
def test_per_label_chain_spills_by_the_slab():
    """single_label: every environment has label extent 1 and takes one tenth of a slab; eviction is by whole slab.  The 80-site chain
    needs 80 units = 8 slabs, the budget of 1 MiB holds four slabs of ten units."""
    from tnml_amd.fixedl import mldmrg
    prob = _single_problem()
    cap = _cap(1, MS, NT)
    assert cap == 4
    out = []
    for budget in (0, 1):
        ts = _ctx(prob, maxm=MS, single=TARGET, budget=budget)
        ts.set_mps(prob[3])
        ts.init()
        reps = mldmrg(ts, 2, *_sweep(MS // 2, MS), pipelined=True)
        out.append(_record(ts, reps))
        ts.close()
    free, tight = out
    _assert_tier_worked("per-label", tight, free, cap)
    _assert_identical(tight, free, "per-label")
    _assert_envs_are_the_oracles("per-label resident", free, prob, "f64", single=TARGET)
    _assert_envs_are_the_oracles("per-label", tight, prob, "f64", single=TARGET)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. held-out contexts
def _run_heldout(pipelined, minm, budget, hbudget, options=()):
    from tnml_amd.fixedl import mldmrg
    prob, hprob = _problem(), _heldout_problem()
    ts = _ctx(prob, budget=budget, options=options)
    hs = _ctx(hprob, budget=hbudget)
    ts.set_mps(prob[3])
    ts.init()
    reps = mldmrg(ts, 1, *_sweep(minm), pipelined=pipelined, heldout=hs)
    rec = _record(ts, reps, hs)
    ts.close()
    hs.close()
    return rec


@functools.lru_cache(maxsize=None)
def _resident_heldout(pipelined, minm, options=()):
    return _run_heldout(pipelined, minm, 0, 0, options)


def _heldout_case(tag, pipelined, minm, where, options=()):
    free = _resident_heldout(pipelined, minm, options)
    tight = _run_heldout(pipelined, minm, 2 if where in ("train", "both") else 0, 1 if where in ("heldout", "both") else 0, options)
    assert all(r["heldout"]["count"] == 100 and (r["heldout"]["bond"], r["heldout"]["half"]) == (r["bond"], r["half"]) for r in tight["reps"])
    if where in ("train", "both"):
        _assert_tier_worked(tag + ", training context", tight, free, _cap(2, M, NT))
    else:
        assert tight["stats"]["spills"] == 0
    if where in ("heldout", "both"):                       # its slabs are sized by its own image count: 10 x 12 x 256 doubles = 240 KiB
        _assert_tier_worked(tag + ", held-out context", tight, free, _cap(1, M, 100), key="hstats")
    else:
        assert tight["hstats"]["spills"] == 0
    _assert_identical(tight, free, tag)
    return tight, free


@pytest.mark.parametrize("where", ["train", "heldout", "both"])
@pytest.mark.parametrize("pipelined", [False, True], ids=["sequential", "pipelined"])
def test_heldout_values_under_a_budget(pipelined, where):
    """a held-out context of 100 images follows the sweep (heldout_step: set_bond_impl and shift_env_impl on its own stream, never
    env_lookahead): the budget on the training context, on the held-out context, on both"""
    tag = "held-out, budget on %s, %s" % (where, "pipelined" if pipelined else "sequential")
    _heldout_case(tag, pipelined, TRUNC, where)


def test_heldout_values_after_a_rolled_back_split_under_budgets():
    """nothing of a rolled-back split may reach the held-out values"""
    hook = (("debug_fail_split", NSPEC // 2),)
    tight, free = _heldout_case("held-out, budget on both, failed split", True, SPEC, "both", hook)
    assert tight["split"]["roll_backs"] == free["split"]["roll_backs"] >= 1
    plain = _resident_heldout(True, SPEC)
    assert [r["heldout"]["ncorrect"] for r in tight["reps"]] == [r["heldout"]["ncorrect"] for r in plain["reps"]]
    np.testing.assert_allclose([r["heldout"]["cost"] for r in tight["reps"]], [r["heldout"]["cost"] for r in plain["reps"]], rtol=1e-8)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 5. options moved between sweeps
def _two_sweeps(first, second, after_init=False):
    """sweep, options `second`, sweep -- no synchronize() in between: the events of the first sweep's last copies are still pending
    (after_init: the options move between init() and the first sweep instead)"""
    from tnml_amd.fixedl import mldmrg
    prob = _problem()
    ts = _ctx(prob, budget=first["env_budget_mb"], env_async=first["env_async"])
    ts.set_mps(prob[3])
    ts.init()
    reps = [] if after_init else mldmrg(ts, 1, *_sweep(TRUNC), pipelined=True)
    mid = dict(stats=ts.env_stats(), dev=ts.device_bytes())
    for k, v in second.items():
        ts.set_option(k, v)
    if after_init:
        reps = mldmrg(ts, 1, *_sweep(TRUNC), pipelined=True)
    reps = reps + mldmrg(ts, 1, *_sweep(TRUNC), pipelined=True)
    rec = _record(ts, reps)
    rec["mid"] = mid
    ts.close()
    return rec


@functools.lru_cache(maxsize=None)
def _resident_two_sweeps():
    return _two_sweeps(dict(env_budget_mb=0, env_async=1), {})


@pytest.mark.parametrize("change", ["env_async 1 -> 0", "env_async 0 -> 1", "budget 2 -> 0", "budget 0 -> 2", "budget 0 -> 2 after init"])
def test_options_moved_between_sweeps(change):
    """sweep, change, sweep on one context against the resident context doing the same two sweeps.  A budget lowered below the slabs
    already allocated frees none of them (slot_acquire never does).  After a whole resident sweep the slabs that are there hold
    every environment of the next sweep too, so nothing has to move and only "no slab is added, same results" can be asked; lowered
    right after init() -- twelve slabs, three times the cap, but three short of what the sweep takes -- the missing ones must come
    from evictions."""
    free = _resident_two_sweeps()
    cap = _cap(2, M, NT)
    if change.startswith("env_async"):
        a = int(change[10])
        tight = _two_sweeps(dict(env_budget_mb=2, env_async=a), dict(env_async=1 - a))
        _assert_tier_worked(change, tight, free, cap, floor=20)
        assert tight["stats"]["spills"] > tight["mid"]["stats"]["spills"] > 0 and tight["stats"]["fetches"] > tight["mid"]["stats"]["fetches"] > 0
    elif change == "budget 2 -> 0":
        tight = _two_sweeps(dict(env_budget_mb=2, env_async=1), dict(env_budget_mb=0))
        mid, st = tight["mid"]["stats"], tight["stats"]
        print("ENVSTATS %s: after the budgeted sweep %s, after the resident one %s" % (change, mid, st))
        assert mid["slabs"] <= cap and mid["spills"] > 0 and mid["fetches"] > 0 and mid["host_bytes"] > 0
        # nothing is evicted any more, and the sweep has asked for every environment: all of them are back
        assert st["spills"] == mid["spills"] and st["fetches"] > mid["fetches"] and st["host_bytes"] == 0
        assert free["stats"]["spills"] == 0 and free["stats"]["slabs"] >= 2 * cap
    else:
        tight = _two_sweeps(dict(env_budget_mb=0, env_async=1), dict(env_budget_mb=2), after_init=change.endswith("after init"))
        mid, st = tight["mid"]["stats"], tight["stats"]
        print("ENVSTATS %s: resident part %s, at the end %s; the resident run ends with %d slabs" % (change, mid, st, free["stats"]["slabs"]))
        assert mid["spills"] == 0 and mid["slabs"] >= 2 * cap
        # slot_acquire never frees a slab: what the code promises is that none is added to those already there
        assert st["slabs"] == mid["slabs"] and tight["dev"] == tight["mid"]["dev"]
        if change.endswith("after init"):
            assert free["stats"]["slabs"] > mid["slabs"]
            assert st["spills"] > 20 and st["fetches"] > 20
    _assert_identical(tight, free, change)
    _assert_envs_are_the_oracles(change, tight, _problem(), "f64")


# ------------------------------------------------------------------------------------------------------------------------------------------
# 6. W replaced under a budget
@pytest.mark.parametrize("how", ["set_site", "gradient_step"])
def test_w_replaced_under_a_budget_drops_the_spilled_copies(how):
    """after a budgeted sweep part of the chain lives on the host; a call that changes W makes every one of those copies stale, and the
    init() that follows must rebuild every environment from the new W (slot_release: on_host = false) instead of fetching one back"""
    from tnml_amd.fixedl import mldmrg
    prob = _problem()
    pixels, labels, phi, W = prob
    ts = _ctx(prob, budget=2)
    ts.set_mps(W)
    ts.init()
    mldmrg(ts, 1, *_sweep(TRUNC), pipelined=True)
    before, W0 = ts.env_stats(), ts.get_mps()
    assert before["host_bytes"] > 0 and before["spills"] > 0
    if how == "set_site":
        j = N // 2 + 3                                     # a Label-free site in the middle of the chain
        A = ts.get_site(j)
        ts.set_site(j, A * (1.0 + 0.05 * np.random.default_rng(1).standard_normal(A.shape)))
    else:
        ts.gradient_step(labels=labels[:64], phi=phi[:64], method="sgd", lr=1e-2, clip=1.0)
    W1 = ts.get_mps()
    assert any(not np.array_equal(a, b) for a, b in zip(W1, W0))
    ts.init()
    tight = _record(ts, mldmrg(ts, 1, *_sweep(TRUNC), pipelined=True))
    ts.close()
    fresh = _ctx(prob)
    fresh.set_mps(W1)
    fresh.init()
    free = _record(fresh, mldmrg(fresh, 1, *_sweep(TRUNC), pipelined=True))
    fresh.close()
    tag = "W replaced by " + how
    _assert_tier_worked(tag, tight, free, _cap(2, M, NT))
    assert tight["stats"]["spills"] > before["spills"] and tight["stats"]["fetches"] > before["fetches"]
    _assert_identical(tight, free, tag)
    _assert_envs_are_the_oracles(tag, tight, prob, "f64")


def test_classify_in_the_middle_of_a_budgeted_sweep():
    """classify()'s three chain buffers come from the same slabs and may evict -- but not the operands of the bond that is set"""
    from tnml_amd import lib
    prob = _problem()
    out = []
    for budget in (0, 2):
        ts = _ctx(prob, budget=budget)
        ts.set_mps(prob[3])
        ts.init()
        reps, acc = [], []
        b, ha = 1, 1
        while ha <= 2:
            reps.append(ts.bond_update(b, ha, *_sweep(TRUNC)))
            if (b, ha) in ((N // 2 - 3, 1), (N - 1, 1), (N // 2 + 3, 2)):
                acc.append(ts.classify())
            b, ha = lib.sweepnext(b, ha, N)
        rec = _record(ts, reps)
        rec["acc"] = acc
        out.append(rec)
        ts.close()
    free, tight = out
    _assert_tier_worked("classify mid-sweep", tight, free, _cap(2, M, NT))
    assert len(tight["acc"]) == len(free["acc"]) == 3
    for x, y in zip(tight["acc"], free["acc"]):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    _assert_identical(tight, free, "classify mid-sweep")
    _assert_envs_are_the_oracles("classify mid-sweep", tight, prob, "f64")


# ------------------------------------------------------------------------------------------------------------------------------------------
# 7. the refusal
def test_a_budget_below_one_slab_is_refused_and_lifting_it_recovers():
    """1 100 images pad to 1 280: one slab of 10 x 12 x 1 280 doubles is 1.17 MiB, more than env_budget_mb = 1 -- an ordinary error return"""
    from tnml_amd.fixedl import TnmlError, mldmrg
    prob = make_problem(N, 1100, M, 11, pixel_boost=200.0)
    assert _cap(1, M, 1100) == 0

    def sweep(ts):
        ts.init()
        return _record(ts, mldmrg(ts, 1, *_sweep(TRUNC)))
    ts = _ctx(prob, budget=1)
    ts.set_mps(prob[3])
    with pytest.raises(TnmlError, match=r"budget of 1 MB holds no slab that could be evicted"):
        ts.init()
    assert ts.env_stats()["slabs"] == 0
    ts.set_option("env_budget_mb", 0)
    again = sweep(ts)
    ts.close()
    fresh = _ctx(prob)
    fresh.set_mps(prob[3])
    free = sweep(fresh)
    fresh.close()
    assert again["stats"]["spills"] == 0 and again["stats"]["slabs"] == free["stats"]["slabs"]
    _assert_identical(again, free, "after the refusal")
