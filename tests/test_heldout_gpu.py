"""Held-out evaluation during training (tnml_heldout_attach / _read / _detach): a context of held-out images follows every bond update
of a training context on its own stream.  Its values are checked against full contractions of the W the training context holds after
each bond update, and the training context itself must not notice it."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

N, NT, NH, M = 12, 60, 40, 6
SWEEP = (6, 3, 1e-10, 3, 1e-3, 1e-10)        # maxm, minm, cutoff, npass, lambda, cconv


def _schedule(n_sites, nsweep=1):
    from tnml_amd import lib
    out = []
    for _ in range(nsweep):
        b, ha = 1, 1
        while ha <= 2:
            out.append((b, ha))
            b, ha = lib.sweepnext(b, ha, n_sites)
    return out


def _single_phi(pixels):
    from oracle import pyoracle
    phi = pyoracle.features_single(pixels, True).copy()
    phi[..., 1] *= 300.0
    return phi


def _problem(single, seed_train=3, seed_held=11, n_sites=N, nt=NT, nh=NH, m=4):
    """training (phi, labels), held-out (phi, labels) from another seed, initial W"""
    px, lab, phi, W = make_problem(n_sites, nt, m, seed_train, pixel_boost=200.0)
    pxh, labh, phih, _ = make_problem(n_sites, nh, m, seed_held, pixel_boost=200.0)
    if single:
        phi, phih = _single_phi(px), _single_phi(pxh)
        W[n_sites // 2 - 1] = W[n_sites // 2 - 1][..., 0] * 3.0
    return (phi, lab), (phih, labh), W


def _states(data, maxm, single, **kw):
    from tnml_amd.fixedl import TrainStates
    phi, lab = data
    return TrainStates(lab, phi.shape[1], maxm, phi=phi, single_label=3 if single else None, **kw)


def _outputs(W, phi, lab, single):
    """W_l(x_n) for every image without the library: the oracle's toverlap (fixedL) or a numpy contraction (per-label variant)"""
    if not single:
        from oracle import pyoracle
        o = pyoracle.Oracle(phi, lab, W)
        return np.stack([o.toverlap(i) for i in range(len(lab))])
    v = np.ones((len(lab), 1))
    for j, A in enumerate(W):
        v = np.einsum("na,nab->nb", v, np.einsum("ns,asb->nab", phi[:, j, :], A))
    return v


def _expected(W, phi, lab, single):
    f = _outputs(W, phi, lab, single)
    lab = np.asarray(lab)
    if single:
        y = (lab == 3).astype(float)[:, None]
        correct = (f[:, 0] > 0.5) == (lab == 3)
    else:
        y = np.eye(10)[lab]
        correct = np.abs(f).argmax(axis=1) == lab
    per = ((f - y) ** 2).sum(axis=1)
    label_cost = np.array([per[lab == l].sum() for l in range(10)])
    return dict(cost=per.sum(), label_cost=label_cost, ncorrect=int(correct.sum()), count=len(lab))


def _check(rep, exp, rtol=1e-10):
    assert rep["count"] == exp["count"]
    assert rep["ncorrect"] == exp["ncorrect"], (rep, exp)
    assert abs(rep["cost"] - exp["cost"]) <= rtol * abs(exp["cost"]), (rep["cost"], exp["cost"])
    np.testing.assert_allclose(rep["label_cost"], exp["label_cost"], rtol=rtol, atol=rtol * abs(exp["cost"]))


@pytest.mark.parametrize("single", [False, True])
def test_heldout_values_follow_every_bond_update(single):
    """one sweep, no pipelining: after attach and after every bond update the held-out values are those of the W the training context holds"""
    tr, ho, W = _problem(single)
    ts, hs = _states(tr, M, single), _states(ho, M, single)
    ts.set_mps(W)
    ts.init()
    ts.attach_heldout(hs)
    r0 = ts.heldout_report()
    assert (r0["bond"], r0["half"]) == (0, 0)
    _check(r0, _expected(W, *ho, single))
    for b, ha in _schedule(N):
        rep = ts.bond_update(b, ha, *SWEEP, report_costs=single)
        h = ts.heldout_report()
        assert (h["bond"], h["half"]) == (b, ha) and rep["bond"] == b
        _check(h, _expected(ts.get_mps(), *ho, single))
    ts.detach_heldout()
    ts.close(); hs.close()


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple, np.ndarray)):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def test_training_is_untouched_and_pipelining_gives_the_same_heldout_values():
    """two training contexts on the same inputs, pipelined, one with a held-out context: every report field and the final W are bitwise equal;
    the held-out values of the pipelined run are bitwise those of a non-pipelined run"""
    from tnml_amd.fixedl import mldmrg
    tr, ho, W = _problem(False)
    runs = {}
    for name, pipelined, with_ho in (("plain", True, False), ("ho", True, True), ("ho_seq", False, True)):
        ts = _states(tr, M, False)
        ts.set_mps(W)
        ts.init()
        hs = _states(ho, M, False) if with_ho else None
        reps = mldmrg(ts, 2, *SWEEP, pipelined=pipelined, heldout=hs)
        runs[name] = (reps, ts.get_mps())
        ts.close()
        if hs is not None:
            hs.close()
    plain, ho_run, seq = runs["plain"], runs["ho"], runs["ho_seq"]
    assert len(plain[0]) == len(ho_run[0]) == 2 * 2 * (N - 1)
    for a, b in zip(plain[0], ho_run[0]):
        assert "heldout" not in a
        b = dict(b)
        b.pop("heldout")
        assert _same(a, b), (a["bond"], a["half"])
    for a, b in zip(plain[1], ho_run[1]):
        assert np.array_equal(a, b)
    for a, b in zip(ho_run[0], seq[0]):
        assert _same(a["heldout"], b["heldout"])


def test_heldout_values_after_a_rolled_back_split():
    """a speculative split whose deferred check fails (debug_fail_split) is rolled back and repeated: the held-out context keeps nothing of it"""
    from tnml_amd.fixedl import mldmrg
    tr, ho, W = _problem(False, nt=200)
    sweep = (M, M, 1e-10, 3, 1e-3, 1e-10)                       # minm = maxm: speculative splits
    seq = []
    for fail in (0, 4):
        ts, hs = _states(tr, M, False), _states(ho, M, False)
        ts.set_option("debug_fail_split", fail)
        ts.set_mps(W)
        ts.init()
        ts.attach_heldout(hs)
        for b, ha in _schedule(N):
            ts.bond_update(b, ha, *sweep)
            h = ts.heldout_report()
            _check(h, _expected(ts.get_mps(), *ho, False))
            seq.append(h)
        assert ts.split_stats()["roll_backs"] >= 1
        ts.close(); hs.close()
        # the same with the next bond update begun before the failed one is ended: both are repeated
        ts, hs = _states(tr, M, False), _states(ho, M, False)
        ts.set_option("debug_fail_split", fail)
        ts.set_mps(W)
        ts.init()
        reps = mldmrg(ts, 1, *sweep, pipelined=True, heldout=hs)
        assert ts.split_stats()["roll_backs"] >= 1
        for r, h in zip(reps, seq[-len(reps):]):
            assert r["heldout"]["ncorrect"] == h["ncorrect"]
            assert abs(r["heldout"]["cost"] - h["cost"]) <= 1e-10 * h["cost"]
        ts.close(); hs.close()


def test_heldout_at_shape_takes_the_resident_forward():
    """7 700 held-out images and 40 x 40 bonds: the held-out forward pass runs on k_fwd_res; its values match a fresh context's tnml_classify"""
    from tnml_amd.fixedl import mldmrg
    n_sites, m = 20, 40
    tr, ho, W = _problem(False, n_sites=n_sites, nt=300, nh=7700, m=m)
    ts, hs = _states(tr, m, False), _states(ho, m, False)
    ts.set_mps(W)
    ts.init()
    hs.profile(True, only="fwd_res")
    reps = mldmrg(ts, 1, m, m, 1e-10, 2, 1e-3, 1e-10, max_bonds=10, heldout=hs)
    h = reps[-1]["heldout"]
    assert (h["bond"], h["half"]) == (10, 1)
    assert hs.profile_read()["fwd_res"][0] > 0
    fresh = _states(ho, m, False)
    fresh.set_mps(ts.get_mps())
    w, pred, cnt, ninc = fresh.classify()
    lab = np.asarray(ho[1])
    per = ((w - np.eye(10)[lab]) ** 2).sum(axis=1)
    assert h["count"] == int(cnt.sum()) and h["ncorrect"] == int(cnt.sum() - ninc.sum())
    assert abs(h["cost"] - per.sum()) <= 1e-10 * per.sum()
    np.testing.assert_allclose(h["label_cost"], [per[lab == l].sum() for l in range(10)], rtol=1e-10)
    for x in (ts, hs, fresh):
        x.close()


def test_two_ranks_on_one_gpu_sum_to_the_one_rank_values():
    """tnml_comm_init_local: every rank attaches its own shard of the held-out set; the sums over the ranks are the one-rank values"""
    from tnml_amd import lib
    from tnml_amd.fixedl import TrainStates, mldmrg
    tr, ho, W = _problem(False)
    (phi, lab), (phih, labh) = tr, ho

    def one_rank():
        ts, hs = _states(tr, M, False), _states(ho, M, False)
        ts.set_mps(W)
        ts.init()
        reps = mldmrg(ts, 1, *SWEEP, heldout=hs)
        ts.close(); hs.close()
        return [r["heldout"] for r in reps]
    ref = one_rank()
    nr = 2
    states, held = [], []
    for r in range(nr):
        lo, hi = lib.shard_bounds(NT, nr, r)
        states.append(TrainStates(lab[lo:hi], N, M, phi=phi[lo:hi], rank=r, nranks=nr, NT_total=NT))
        lo, hi = lib.shard_bounds(NH, nr, r)
        held.append(TrainStates(labh[lo:hi], N, M, phi=phih[lo:hi]))
    TrainStates.comm_init_local(states)
    out, err = [None] * nr, [None] * nr

    def work(r):
        try:
            states[r].set_mps(W)
            states[r].init()
            out[r] = [x["heldout"] for x in mldmrg(states[r], 1, *SWEEP, heldout=held[r])]
        except Exception as e:                                   # noqa: BLE001
            err[r] = e
    th = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not any(t.is_alive() for t in th), "a rank hung"
    for e in err:
        if e is not None:
            raise e
    for k, want in enumerate(ref):
        got = [out[r][k] for r in range(nr)]
        assert sum(g["count"] for g in got) == want["count"] == NH
        assert sum(g["ncorrect"] for g in got) == want["ncorrect"]
        assert abs(sum(g["cost"] for g in got) - want["cost"]) <= 1e-10 * want["cost"]
    for x in states + held:
        x.close()


def _bare_context(n_sites, maxm):
    """a context without image data (TrainStates always sets some)"""
    from tnml_amd import lib
    L = lib.load()
    h = C.c_void_p()
    cfg = lib.Config(0, 0, 1, n_sites, 10, 10, maxm, lib.DTYPES["f64"], 0, 0, 0)
    assert L.tnml_create(C.byref(h), C.byref(cfg)) == 0
    return h


def test_attach_refusals_and_the_lock():
    from tnml_amd import lib
    from tnml_amd.fixedl import TnmlError, TrainStates
    tr, ho, W = _problem(False)
    Ws = [A.copy() for A in W]
    Ws[N // 2 - 1] = Ws[N // 2 - 1][..., 0]
    trs, hos, _ = _problem(True)

    def fresh_train(data=tr, single=False, maxm=M):
        ts = _states(data, maxm, single)
        ts.set_mps(Ws if single else W)
        ts.init()
        return ts
    ts = fresh_train()

    def refused(other, words):
        with pytest.raises(TnmlError) as e:
            ts.attach_heldout(other)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        other.close()
    phi, lab = ho
    refused(TrainStates(lab, 10, M, phi=phi[:, :10]), ["N differs"])
    refused(_states(hos, M, True), ["mode differs"])
    refused(_states(ho, M, False, dtype="f64_e32"), ["dtype differs"])
    refused(_states(ho, M - 2, False), ["maxm", "smaller"])
    refused(TrainStates(lab, N, M, phi=phi, rank=0, nranks=2), ["nranks = 2"])
    bare = _bare_context(N, M)
    L = lib.load()
    assert L.tnml_heldout_attach(ts._h, bare) != 0
    assert b"no image data" in L.tnml_last_error(ts._h)
    L.tnml_destroy(bare)
    # target_label of the per-label variant
    t3 = fresh_train(trs, True)
    other = TrainStates(hos[1], N, M, phi=hos[0], single_label=5)
    with pytest.raises(TnmlError, match="target_label differs"):
        t3.attach_heldout(other)
    other.close(); t3.close()
    # a bond update in flight, then mid-sweep
    hs = _states(ho, M, False)
    ts.bond_update_begin(1, 1, *SWEEP)
    with pytest.raises(TnmlError, match="in flight"):
        ts.attach_heldout(hs)
    ts.bond_update_end()
    with pytest.raises(TnmlError, match="sweep start"):
        ts.attach_heldout(hs)
    ts.close()
    # read without attach
    ts = fresh_train()
    with pytest.raises(TnmlError, match="no held-out context"):
        ts.heldout_report()
    # the lock: calls that would change the held-out context's W, environments, data or bond
    ts.attach_heldout(hs)
    B = hs.bond_tensor(1)
    for call in (lambda: hs.set_site(1, W[0]), hs.init, lambda: hs.setBond(2), lambda: hs.shiftE(1, True),
                 lambda: hs.bond_update(1, 1, *SWEEP), hs.classify, lambda: hs.forward(B), lambda: hs.quadcost(B, 0.0)):
        with pytest.raises(TnmlError, match="held-out"):
            call()
    with pytest.raises(TnmlError, match="held-out"):             # and the training context keeps its W and environments to bond updates
        ts.init()
    hs.get_site(1); hs.env(3)                                    # read-only calls keep working
    assert ts.heldout_report()["bond"] == 0
    with pytest.raises(TnmlError):                               # attached elsewhere already
        fresh_train().attach_heldout(hs)
    # destroying either context first detaches
    hs.close()
    with pytest.raises(TnmlError, match="no held-out context"):
        ts.heldout_report()
    ts.bond_update(1, 1, *SWEEP)
    ts.close()
    ts, hs = fresh_train(), _states(ho, M, False)
    ts.attach_heldout(hs)
    ts.close()
    hs.init()                                                    # unlocked again
    hs.close()


def _digits(tmp_path, per_label=150):
    """scikit-learn's 8x8 digits as idx files: 150 images per digit for training, the rest as the t10k set (as test_digits_e2e.py)"""
    from sklearn.datasets import load_digits
    from tnml_amd import synth
    d = load_digits()
    px = np.clip(np.rint(d.images.reshape(-1, 64) * (255.0 / 16.0)), 0, 255).astype(np.uint8)
    lab = d.target.astype(np.int32)
    train_idx = np.concatenate([np.flatnonzero(lab == l)[:per_label] for l in range(10)])
    test_idx = np.setdiff1d(np.arange(len(lab)), train_idx)
    data = str(tmp_path / "data")
    synth.write_idx(data, px[np.sort(train_idx)], lab[np.sort(train_idx)], side=8)
    synth.write_idx(data, px[test_idx], lab[test_idx], train=False, side=8)
    return data, px[test_idx], lab[test_idx]


HELD_RE = r"^Held-out: Percent correct = ([0-9.]+)%, # incorrect = (\d+)/(\d+), Cost = ([0-9.]+)$"


def test_drivers_report_heldout_lines_on_real_images(tmp_path):
    import re
    import subprocess
    import sys
    from tnml_amd import hostlib
    from tnml_amd.fixedl import TrainStates
    from oracle import pyoracle
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data, tpx, tlab = _digits(tmp_path)
    keys = "datadir = %s\nfeature_scale = 255\n" % data
    body = "Ntrain = 150\nNbatch = 10\nNsweep = 1\ncutoff = 1E-10\nmaxm = 10\nminm = 5\nninitial = 5\nlambda = 1E-3\nNpass = 4\nseed = 3\n"

    def run(name, extra, prog="fixedL"):
        wd = tmp_path / name
        wd.mkdir()
        (wd / "input").write_text("input\n{\n" + keys + body + extra + "}\n")
        cmd = [sys.executable, "-m", "tnml_amd.train"] if prog == "train" else [os.path.join(root, "tnml_amd", prog)]
        r = subprocess.run(cmd + ["input"], capture_output=True, text=True, cwd=wd, timeout=600, env=dict(os.environ, PYTHONPATH=root))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        return r.stdout, wd
    yes, wy = run("yes", "heldout = yes\nbond_log = bonds.csv\n")
    no, _ = run("no", "heldout = no\n")
    plain, _ = run("plain", "")
    assert no == plain                                                   # off: byte-identical output
    held = re.findall(HELD_RE, yes, re.M)
    assert len(held) == 1 + 2 * 63 and all(int(h[2]) == len(tlab) for h in held)
    assert [ln for ln in yes.splitlines() if not ln.startswith("Held-out:")] == plain.splitlines()   # training untouched
    lines = yes.splitlines()
    assert lines[lines.index(next(ln for ln in lines if ln.startswith("Before starting DMRG Cost"))) + 1].startswith("Held-out:")
    after = [i for i, ln in enumerate(lines) if ln.startswith("--> After SVD, Cost")]
    assert len(after) == 2 * 63 and all(lines[i + 1].startswith("Held-out:") for i in after)
    csv = (wy / "bonds.csv").read_text().splitlines()
    assert csv[0].endswith(",heldout_cost,heldout_ncorrect,nheldout") and len(csv) == 1 + 2 * 63
    last = csv[-1].split(",")
    assert int(last[-1]) == len(tlab) and int(last[-2]) == len(tlab) - int(held[-1][1])
    # fulltest on the W this run wrote counts what the last held-out line says
    (wy / "input_test").write_text("input\n{\n%s}\n" % keys)
    ev = subprocess.run([os.path.join(root, "tnml_amd", "fulltest"), "input_test"], capture_output=True, text=True, cwd=wy, timeout=600)
    assert ev.returncode == 0, ev.stdout[-1500:] + ev.stderr[-1500:]
    m = re.search(r"(\d+)/(\d+) correct", ev.stdout)
    assert m and int(m.group(2)) == len(tlab) and int(m.group(1)) == len(tlab) - int(held[-1][1])
    # the Python driver (one process): the same counts, costs within 1e-10
    py, _ = run("py", "heldout = yes\n", prog="train")
    held_py = re.findall(HELD_RE, py, re.M)
    assert [h[1:3] for h in held_py] == [h[1:3] for h in held]
    assert all(abs(float(a[3]) - float(b[3])) <= 1.0001e-10 for a, b in zip(held_py, held))
    # the per-label driver: its last held-out line is a tnml_classify of the W<label> it wrote
    sg, ws = run("single", "label = 3\nheldout = yes\n", prog="single")
    held_s = re.findall(HELD_RE, sg, re.M)
    assert len(held_s) == 1 + 2 * 63
    W3 = hostlib.read_mps(str(ws / "W3"))
    hs = TrainStates(tlab, 64, 10, phi=pyoracle.features_single(tpx, True), single_label=3)
    hs.set_mps(W3)
    w, pred, cnt, ninc = hs.classify()
    y = (tlab == 3).astype(float)
    assert int(held_s[-1][1]) == int(ninc.sum()) == int(((w[:, 0] > 0.5) != (tlab == 3)).sum())
    assert abs(float(held_s[-1][3]) - ((w[:, 0] - y) ** 2).sum() / len(tlab)) <= 1e-9
    hs.close()
