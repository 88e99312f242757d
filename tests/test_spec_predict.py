"""Predicted splits (option spec_predict; svd.hip: k_truncate_verdict, tnml_update.hip: tnml_bond_update_end).  A truncating split
(minm < the columns it may keep) takes the speculative form -- no host synchronisation inside tnml_bond_update_begin -- on the column
count its bond kept at its last two finished visits; a kernel applies the truncation rule to the eigenvalues on the device and a
wrong guess is rolled back and repeated with the synchronous split.  Whatever is predicted, every number must be the one a run
without the option gives, bit for bit ("sync" below: spec_predict = 0)."""
import functools

import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

N, NT, M0, MAXM = 12, 200, 6, 12
# nsweep is put in front: maxm, minm, cutoff, Npass, lambda, cconv
TRUNC = (MAXM, 2, 1e-6, 3, 1e-3, 1e-10)          # most bonds keep a count strictly between minm and maxm; one changes on its last visit
STABLE = (MAXM, 2, 1e-4, 3, 1e-3, 1e-10)         # sweep 3 repeats sweep 2 on every bond, both halves of sweep 2 agree


@functools.lru_cache(maxsize=None)
def _problem(nt=NT):
    return make_problem(N, nt, M0, 5, pixel_boost=200.0)


def _run(nsweep, sweep, on, pipelined=True, mispredict=None, heldout=False):
    from tnml_amd.fixedl import TrainStates, mldmrg
    pixels, labels, phi, W = _problem()
    ts = TrainStates(labels, N, MAXM, phi=phi)
    hs = None
    if heldout:
        hpix, hlab, hphi, _ = make_problem(N, 50, M0, 11, pixel_boost=200.0)
        hs = TrainStates(hlab, N, MAXM, phi=hphi)
    ts.set_option("spec_predict", on)
    if mispredict is not None:
        ts.set_option("debug_mispredict", mispredict)
    ts.set_mps(W)
    ts.init()
    reps = mldmrg(ts, nsweep, *sweep, pipelined=pipelined, heldout=hs)
    ts.synchronize()
    out = dict(reps=reps, W=ts.get_mps(), svd=ts.svd_stats(), pred=ts.spec_predict_stats(), split=ts.split_stats())
    ts.close()
    if hs is not None:
        hs.close()
    return out


@functools.lru_cache(maxsize=None)
def _cached(nsweep, sweep, on, pipelined=True):
    return _run(nsweep, sweep, on, pipelined)


def _assert_bitwise(a, b):
    """newm, cost, #correct and the first CG cost equal, truncerr to 1e-12 (it is a host sum over mirrored or copied eigenvalues), every site tensor equal"""
    ra, rb = a["reps"], b["reps"]
    assert [(r["bond"], r["half"]) for r in ra] == [(r["bond"], r["half"]) for r in rb]
    assert [r["newm"] for r in ra] == [r["newm"] for r in rb]
    assert [r["cost"] for r in ra] == [r["cost"] for r in rb]
    assert [r["ncorrect"] for r in ra] == [r["ncorrect"] for r in rb]
    assert [r["cg"]["cost"] for r in ra] == [r["cg"]["cost"] for r in rb]
    np.testing.assert_allclose([r["truncerr"] for r in ra], [r["truncerr"] for r in rb], rtol=1e-12, atol=1e-300)
    assert len(a["W"]) == len(b["W"])
    for x, y in zip(a["W"], b["W"]):
        assert np.array_equal(x, y)


def _changes(reps):
    """visits whose newm differs from the previous visit of the same bond"""
    last, n = {}, 0
    for r in reps:
        if r["bond"] in last and last[r["bond"]] != r["newm"]:
            n += 1
        last[r["bond"]] = r["newm"]
    return n


def test_option_is_off_by_default_and_accepted():
    from tnml_amd.fixedl import TrainStates
    pixels, labels, phi, W = _problem()
    ts = TrainStates(labels, N, MAXM, phi=phi)
    assert ts.spec_predict_stats() == dict(predicted=0, mispredicted=0, redo_ms=0.0)
    ts.set_option("spec_predict", 1)
    ts.set_option("debug_mispredict", 0)
    ts.set_option("debug_mispredict", -1)
    ts.set_option("spec_predict", 0)
    ts.close()
    off = _cached(3, TRUNC, 0)                                       # a truncating sweep with the defaults
    assert off["pred"]["predicted"] == 0 and off["pred"]["mispredicted"] == 0
    assert any(TRUNC[1] < r["newm"] < MAXM for r in off["reps"])


def _spectra(n, rng):
    """ascending eigenvalue vectors as the eigensolver could leave them"""
    geo = np.sort(10.0 ** -np.linspace(0, 16, n))
    out = [geo, geo * 3.7e5, np.zeros(n)]
    z = geo.copy(); z[: n // 2] = 0.0
    out.append(z)
    t = geo.copy(); t[: max(1, n // 3)] = -1e-18 * np.arange(1, max(1, n // 3) + 1)[::-1]        # tiny negative values at the small end
    out.append(t)
    q = t.copy(); q[n // 2] = np.nan                                                             # ... and a NaN among them
    out.append(q)
    out.append(np.sort(np.full(n, 0.25)))                                                        # flat: the cutoff decides everything or nothing
    for _ in range(3):
        out.append(np.sort(rng.random(n) ** 12))
    for _ in range(2):
        out.append(np.sort(np.exp(-rng.random(n) * 40.0)) * rng.choice([1.0, 1e-3, 1e6]))
    return out


def test_verdict_kernel_repeats_the_host_rule():
    """k_truncate_verdict against tnml_truncate on what the host would hand it (largest first, !(lam > 0) -> 0): the kept count and the
    verdict on a guess are equal, exactly, for spectra and parameters that let maxm, minm and the cutoff each decide"""
    from tnml_amd import lib
    from tnml_amd.fixedl import TrainStates
    pixels, labels, phi, W = make_problem(8, 60, 4, 3)
    ts = TrainStates(labels, 8, 4, pixels=pixels)
    rng = np.random.default_rng(17)
    ncase, decided = 0, set()
    for n in (3, 17, 64, 240):
        params = [(n, 1, 1e-10), (n + 5, 0, 1e-6), (max(1, n // 2), 1, 0.0), (max(1, n // 2), max(1, n // 4), 1e-3),
                  (n, max(1, n // 3), 1.5), (n, n, 1e-2), (max(2, n - 1), 2, 1e-14), (1, 1, 1e-10)]
        for ev in _spectra(n, rng):
            p = ev[::-1].copy()
            p = np.where(p > 0, p, 0.0)
            for maxm, minm, cutoff in params:
                m_ref, _ = lib.truncate(p, maxm, min(minm, maxm), cutoff)
                for guess in (m_ref, m_ref - 1 if (ncase // 2) % 2 and m_ref > 1 else m_ref + 1):
                    m, wrong = ts.truncate_device(ev, maxm, min(minm, maxm), cutoff, guess)
                    assert (m, wrong) == (m_ref, int(guess != m_ref)), (n, maxm, minm, cutoff, guess, m, m_ref)
                    ncase += 1
                decided.add("maxm" if m_ref == maxm < n else "minm" if m_ref == min(minm, maxm) else "cutoff" if m_ref < min(n, maxm) else "all")
    ts.close()
    assert ncase >= 300 and decided == {"maxm", "minm", "cutoff", "all"}, (ncase, decided)


@pytest.mark.parametrize("pipelined", [False, True])
def test_truncating_sweeps_are_bitwise_those_of_the_synchronous_split(pipelined):
    sync = _cached(3, TRUNC, 0, pipelined)
    on = _cached(3, TRUNC, 1, pipelined)
    _assert_bitwise(on, sync)
    print("predicted", on["pred"], "split", on["split"], "changes in the sync trace", _changes(sync["reps"]), "newm", [r["newm"] for r in sync["reps"]])
    assert on["pred"]["predicted"] >= 1
    assert on["pred"]["mispredicted"] >= 1
    assert on["pred"]["mispredicted"] <= _changes(sync["reps"])
    assert on["svd"]["fallbacks"] == sync["svd"]["fallbacks"]
    assert on["split"]["speculative_splits"] >= on["pred"]["predicted"] and on["split"]["roll_backs"] >= on["pred"]["mispredicted"]
    assert sync["pred"]["predicted"] == 0
    ro = _oracle_trunc()
    assert [r["newm"] for r in on["reps"]] == [r["newm"] for r in ro] and [r["ncorrect"] for r in on["reps"]] == [r["ncorrect"] for r in ro]
    np.testing.assert_allclose([r["cost"] for r in on["reps"]], [r["cost"] for r in ro], rtol=1e-8)


@functools.lru_cache(maxsize=None)
def _oracle_trunc():
    from oracle import pyoracle
    pixels, labels, phi, W = _problem()
    o = pyoracle.Oracle(phi, labels, W, nthread=2)
    o.init()
    return o.mldmrg(3, *TRUNC)


def test_a_stable_run_mispredicts_nothing_more_in_its_third_sweep():
    two, three = _run(2, STABLE, 1), _run(3, STABLE, 1)
    _assert_bitwise(two, _run(2, STABLE, 0))
    _assert_bitwise(three, _run(3, STABLE, 0))
    print("two sweeps", two["pred"], "three sweeps", three["pred"])
    assert three["pred"]["mispredicted"] == two["pred"]["mispredicted"]
    assert three["pred"]["predicted"] > two["pred"]["predicted"]


def test_forced_mispredictions_roll_back_and_change_nothing():
    """debug_mispredict moves the guess of the first, an interior and the last predicted split of the run by one column"""
    sync = _cached(3, TRUNC, 0)
    base = _cached(3, TRUNC, 1)
    npred = base["pred"]["predicted"]
    assert npred >= 3
    for k in (0, npred // 2, npred - 1):
        forced = _run(3, TRUNC, 1, mispredict=k)
        _assert_bitwise(forced, sync)
        assert forced["pred"]["mispredicted"] == base["pred"]["mispredicted"] + 1, (k, forced["pred"], base["pred"])
        assert forced["svd"]["fallbacks"] == base["svd"]["fallbacks"], (k, forced["svd"], base["svd"])
        assert forced["pred"]["redo_ms"] > 0.0


def test_heldout_context_keeps_nothing_of_a_mispredicted_split():
    sync = _run(3, TRUNC, 0, heldout=True)
    forced = _run(3, TRUNC, 1, mispredict=1, heldout=True)
    _assert_bitwise(forced, sync)
    assert forced["pred"]["mispredicted"] >= 1
    for a, b in zip(forced["reps"], sync["reps"]):
        ha, hb = a["heldout"], b["heldout"]
        assert (ha["bond"], ha["half"], ha["count"]) == (hb["bond"], hb["half"], hb["count"]) and ha["count"] == 50
        assert ha["cost"] == hb["cost"] and ha["ncorrect"] == hb["ncorrect"], (a["bond"], a["half"], ha, hb)


@pytest.mark.parametrize("oneshot", [False, True])
def test_two_ranks_roll_a_misprediction_back_together(oneshot):
    """the verdict travels in a carried word of its own (summed over the ranks); debug_mispredict is set on EVERY rank -- ranks that keep
    different column counts would enter collectives of different sizes"""
    from test_multirank_one_gpu import _run_ranks
    from tnml_amd.fixedl import mldmrg
    pixels, labels, phi, W = _problem(151)

    def body(on, mispredict):
        def run(ts, r):
            ts.set_option("spec_predict", on)
            if mispredict is not None:
                ts.set_option("debug_mispredict", mispredict)
            ts.init()
            reps = mldmrg(ts, 3, *TRUNC, pipelined=True)
            ts.replica_check()
            return dict(reps=reps, W=ts.get_mps(), pred=ts.spec_predict_stats(), svd=ts.svd_stats())
        return run
    one = _run_ranks(1, labels, phi, W, N, MAXM, body(0, None))[0]
    sync = _run_ranks(2, labels, phi, W, N, MAXM, body(0, None), oneshot=oneshot)
    clean = _run_ranks(2, labels, phi, W, N, MAXM, body(1, None), oneshot=oneshot)
    forced = _run_ranks(2, labels, phi, W, N, MAXM, body(1, 2), oneshot=oneshot)
    assert clean[0]["pred"]["predicted"] >= 1
    assert forced[0]["pred"]["mispredicted"] >= 1
    for run in (clean, forced):
        for x in run:
            _assert_bitwise(x, run[0])                                # every rank holds rank 0's bits
            assert (x["pred"]["predicted"], x["pred"]["mispredicted"]) == (run[0]["pred"]["predicted"], run[0]["pred"]["mispredicted"])
        _assert_bitwise(run[0], sync[0])
        assert [r["newm"] for r in run[0]["reps"]] == [r["newm"] for r in one["reps"]]
        assert [r["ncorrect"] for r in run[0]["reps"]] == [r["ncorrect"] for r in one["reps"]]
        np.testing.assert_allclose([r["cost"] for r in run[0]["reps"]], [r["cost"] for r in one["reps"]], rtol=1e-9)


def test_predicted_split_at_the_one_workgroup_size():
    """n = 240, the largest matrix side one workgroup solves: bond 8 of a 20-site, m = 120 network updated six times in a zig-zag
    (ha = 1, 2, 1, 2, 1, 2) with maxm 120, minm 60.  The cutoff 1.8e-3 is taken from the CPU oracle, which keeps 120, 119, 119, 119, 118,
    118 columns on these inputs: the fourth visit is predicted right at 119, the fifth is predicted 119 and keeps 118."""
    from tnml_amd.fixedl import TrainStates
    n_sites, nt, m, cutoff = 20, 600, 120, 1.8e-3
    pixels, labels, phi, W = make_problem(n_sites, nt, m, 3, pixel_boost=200.0)

    def run(on):
        ts = TrainStates(labels, n_sites, m, phi=phi)
        ts.set_option("spec_predict", on)
        ts.set_mps(W)
        ts.init()
        for bb in range(1, 8):
            ts.shiftE(bb, True)
        reps = [ts.bond_update(8, ha, m, 60, cutoff, 3, 1e-3, 1e-10) for ha in (1, 2, 1, 2, 1, 2)]
        ts.synchronize()
        out = dict(reps=reps, W=ts.get_mps(), pred=ts.spec_predict_stats(), svd=ts.svd_stats())
        ts.close()
        return out
    sync = run(0)
    kept = [r["newm"] for r in sync["reps"]]
    print("sync run keeps", kept)
    assert any(60 < k < 120 for k in kept), "precondition: the cutoff no longer decides a count strictly between minm and maxm: %s" % kept
    assert any(kept[i - 1] == kept[i - 2] for i in range(2, 6)), "precondition: no visit follows two equal ones, nothing can be predicted: %s" % kept
    on = run(1)
    print("predicted", on["pred"])
    _assert_bitwise(on, sync)
    assert on["pred"]["predicted"] >= 1
    assert on["svd"]["fallbacks"] == sync["svd"]["fallbacks"]
