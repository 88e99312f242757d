"""GPU tests of the linear classifier (linear.cc): the batched CG of kernels_linear.hip against a numpy restatement of
linear.cc:27-90 and :169-187, its determinism, and the `linear` driver end to end including the hand-off of its W%d files to
fixedL's W0..W9 branch (fixedL.cc:682-701)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tnml_amd import hostlib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEAR = os.path.join(ROOT, "tnml_amd", "linear")
FIXEDL = os.path.join(ROOT, "tnml_amd", "fixedL")
if not (os.path.exists(LINEAR) and os.path.exists(os.path.join(ROOT, "tnml_amd", "libtnml.so"))):
    import __graft_entry__
    __graft_entry__.build()

from tnml_amd.linear import LinearCG  # noqa: E402  (after the build)


# ---- numpy restatement of linear.cc (literal order of operations) ---------------------------------------------------------------
def features_of(pixels):
    """v_n = [1, x/4...], x = byte/255. (linear.cc:118-121,133-139, mllib/mnist.h:495)"""
    x = (np.asarray(pixels, dtype=np.float64) / 255.0) / 4.0
    return np.concatenate([np.ones((x.shape[0], 1)), x], axis=1)


def np_cgrad(Xv, y, W, lam, npass, rr=None, Ws=None):
    """cgrad, linear.cc:27-90, one label column: returns (W, costs); rr (a list) receives r.r, the initial one first, Ws the W of
    every pass"""
    NT = Xv.shape[0]
    W = W.copy()
    r = np.zeros_like(W)
    for n in range(NT):                                  # :37-42 (per image, as written)
        Wt = W @ Xv[n]
        r += (y[n] - Wt) * Xv[n]
    r /= NT
    if lam != 0.0:
        r = r - lam * W
    p = r.copy()
    costs = []
    if rr is not None:
        rr.append(r @ r)
    for _ in range(npass):
        pv = Xv @ p                                      # :52-57
        pAp = (pv * pv).sum()
        pAp /= NT
        pAp += lam * (W @ W)                             # :58 W.W, not p.p
        a = (r @ r) / pAp
        W = W + a * p
        dW = y - Xv @ W                                  # :64-69
        nr = Xv.T @ dW
        C = (dW * dW).sum()
        nr /= NT
        C /= NT
        if lam != 0.0:
            nr = nr - lam * W
        beta = (nr @ nr) / (r @ r)
        r = nr
        if rr is not None:
            rr.append(r @ r)
        C += lam * (W @ W)
        costs.append(C)
        if Ws is not None:
            Ws.append(W.copy())
        p = r + beta * p
    return W, np.array(costs)


def stable_passes(Xv, y, W, lam, npass, c_scale):
    """How many leading passes of the restatement are insensitive to the order of its sums: it runs a second time over the images in
    reverse order, and a pass counts while both runs agree to 1e-11 on the cost (relative to max(|C|, c_scale)) and to 1e-10 on W
    (relative to max|W|) -- ten times inside the tolerances the kernels are held to (1e-10, 1e-9).  At lambda = 0 the CG amplifies
    round-off -- on an ill-conditioned system, and on any system once it has converged (its steps are then round-off over round-off,
    0/0 once r is exactly 0) -- so two summation orders part after some passes; those passes say nothing about the kernels and are not
    compared.  A pass that starts from a residual at round-off (r.r below 1e-24 of its start) ends the count as well."""
    Ws1, Ws2, rr = [], [], []
    with np.errstate(all="ignore"):
        _, c1 = np_cgrad(Xv, y, W, lam, npass, rr=rr, Ws=Ws1)
        _, c2 = np_cgrad(np.ascontiguousarray(Xv[::-1]), np.ascontiguousarray(y[::-1]), W, lam, npass, Ws=Ws2)
        rr = np.array(rr)
        ok = (np.abs(c1 - c2) <= 1e-11 * np.maximum(np.abs(c1), c_scale)) & (rr[:-1] > 1e-24 * rr[0])
        ok &= np.array([np.abs(a - b).max() <= 1e-10 * np.abs(a).max() for a, b in zip(Ws1, Ws2)])
    return npass if ok.all() else int(np.argmin(ok))


def np_evaluate(Xv, labels, L, V):
    """linear.cc:169-187: (#correct, Cnl)"""
    y = np.where(labels == L, 1.0, -1.0)
    f = Xv @ V
    return int((f * y > 0).sum()), float(((f - y) ** 2).sum() / len(y))


def _problem(kind, NT, N, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 10, size=NT).astype(np.int32)
    if kind == "u8":
        pixels = synth.synthetic_images(N, labels, seed=seed)
        return dict(pixels=pixels), features_of(pixels), labels
    feats = rng.normal(0.0, 0.25, size=(NT, N))          # a general (well-conditioned) design matrix
    return dict(features=feats), np.concatenate([np.ones((NT, 1)), feats], axis=1), labels


def _start(K, N, seed):
    V = np.random.default_rng(seed + 100).uniform(0.0, 1.0, size=(K, N + 1))
    return V / np.linalg.norm(V, axis=1, keepdims=True)


# ---- per-pass parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 196, 784])
@pytest.mark.parametrize("NT", [1, 37, 257, 6007])
@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("K", [1, 10])
@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_per_pass_parity(kind, K, lam, NT, N):
    """the first 30 passes against the restatement: costs to 1e-10 relative on every pass, W to 1e-9 after the last one -- over the
    passes on which the restatement itself is insensitive to the order of its sums (stable_passes; all 30 at lambda = 1e-3)"""
    data, Xv, labels = _problem(kind, NT, N, seed=NT + N)
    cols = list(range(K)) if K == 10 else [NT % 10]
    V0 = _start(K, N, NT)
    ys = [np.where(labels == L, 1.0, -1.0) for L in cols]
    c_scale = [1e-6 * float(((y - Xv @ V0[k]) ** 2).mean()) for k, y in enumerate(ys)]
    npass = min(stable_passes(Xv, y, V0[k], lam, 30, c_scale[k]) for k, y in enumerate(ys))
    assert npass == 30 if lam > 0 else npass >= (1 if NT == 1 else 3), npass
    cg = LinearCG(labels, cols, device=0, **data)
    cg.start(V0, lam)
    got = cg.run(npass)
    Vg = cg.V
    for k, y in enumerate(ys):
        Wr, cr = np_cgrad(Xv, y, V0[k], lam, npass)
        tol = 1e-10 * np.maximum(np.abs(cr), c_scale[k])
        bad = np.nonzero(~(np.abs(got[:, k] - cr) <= tol))[0]
        assert len(bad) == 0, (k, npass, bad, got[bad, k], cr[bad])
        dv = np.abs(Vg[k] - Wr)
        assert dv.max() <= 1e-9 * np.abs(Wr).max(), (k, npass, int(dv.argmax()), dv.max())


def test_convergence_to_least_squares():
    """lambda = 0, well-conditioned f64 problem: the CG reaches numpy.linalg.lstsq's solution"""
    N, NT = 16, 400
    data, Xv, labels = _problem("f64", NT, N, seed=11)
    cols = [0, 4, 9]
    cg = LinearCG(labels, cols, device=0, **data)
    cg.start(_start(3, N, 11), 0.0)
    cg.run(50)
    V = cg.V
    for k, L in enumerate(cols):
        y = np.where(labels == L, 1.0, -1.0)
        ls = np.linalg.lstsq(Xv, y, rcond=None)[0]
        assert np.abs(V[k] - ls).max() <= 1e-8 * np.abs(ls).max(), (L, np.abs(V[k] - ls).max())


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_column_independence_bitwise(kind):
    """column L of a K = 10 run is the K = 1 run of label L, bit for bit"""
    N, NT = 196, 3001
    data, _, labels = _problem(kind, NT, N, seed=5)
    V0 = _start(10, N, 5)
    cg = LinearCG(labels, list(range(10)), device=0, **data)
    cg.start(V0, 1e-3)
    c10 = cg.run(25)
    V10 = cg.V
    for L in (0, 3, 9):
        one = LinearCG(labels, [L], device=0, **data)
        one.start(V0[L:L + 1], 1e-3)
        c1 = one.run(25)
        np.testing.assert_array_equal(c1[:, 0], c10[:, L])
        np.testing.assert_array_equal(one.V[0], V10[L])
        one.close()


def test_chunked_runs_and_repeatability_bitwise():
    N, NT = 784, 2500
    data, _, labels = _problem("u8", NT, N, seed=9)
    V0 = _start(10, N, 9)
    runs = []
    for chunks in ([30], [10, 20], [30]):
        cg = LinearCG(labels, list(range(10)), device=0, **data)
        cg.start(V0, 1e-3)
        costs = np.concatenate([cg.run(c) for c in chunks])
        runs.append((costs, cg.V))
        cg.close()
    for costs, V in runs[1:]:
        np.testing.assert_array_equal(costs, runs[0][0])
        np.testing.assert_array_equal(V, runs[0][1])


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_evaluate(kind):
    N, NT = 196, 1234
    data, Xv, labels = _problem(kind, NT, N, seed=21)
    cols = [1, 2, 7]
    cg = LinearCG(labels, cols, device=0, **data)
    V = np.random.default_rng(3).normal(scale=0.2, size=(3, N + 1))
    nc, cnl = cg.evaluate(V)
    for k, L in enumerate(cols):
        want_nc, want_cnl = np_evaluate(Xv, labels, L, V[k])
        assert nc[k] == want_nc
        assert abs(cnl[k] - want_cnl) <= 1e-12 * want_cnl
    # evaluation leaves the CG alone, and a new data set (the test set) can be loaded into the same context
    cg.start(V, 0.0)
    a = cg.run(3)
    cg.evaluate(V)
    b = cg.run(3)
    ref = LinearCG(labels, cols, device=0, **data)
    ref.start(V, 0.0)
    np.testing.assert_array_equal(np.concatenate([a, b]), ref.run(6))
    data2, Xv2, labels2 = _problem(kind, 300, N, seed=22)
    cg.set_data(labels2, **data2)
    nc2, cnl2 = cg.evaluate(V)
    for k, L in enumerate(cols):
        want_nc, want_cnl = np_evaluate(Xv2, labels2, L, V[k])
        assert nc2[k] == want_nc and abs(cnl2[k] - want_cnl) <= 1e-12 * want_cnl


# ---- the driver ---------------------------------------------------------------------------------------------------------------
N_DRV, PER_LABEL, NTEST = 16, 20, 57


def _dataset(tmp_path):
    labels = synth.synthetic_labels(10 * PER_LABEL, seed=31, per_label=PER_LABEL)
    pixels = synth.synthetic_images(N_DRV, labels, seed=31)
    tl = np.random.default_rng(32).integers(0, 10, size=NTEST).astype(np.int32)
    tp = synth.synthetic_images(N_DRV, tl, seed=33)
    d = str(tmp_path / "data")
    synth.write_idx(d, pixels, labels)
    synth.write_idx(d, tp, tl, train=False)
    return d, pixels, labels, tp, tl


def _run(exe, wd, body, timeout=300):
    os.makedirs(wd, exist_ok=True)
    inp = os.path.join(wd, "input")
    with open(inp, "w") as f:
        f.write("input\n{\n" + body + "\n}\n")
    out = subprocess.run(["timeout", "-k", "10", str(timeout), exe, inp], capture_output=True, text=True, cwd=wd)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


def test_driver_end_to_end(tmp_path):
    d, pixels, labels, tp, tl = _dataset(tmp_path)
    Xv, Xt = features_of(pixels), features_of(tp)
    npass = 40
    common = "datadir = %s\nNlinear_iter = %d\nlambda = 0\ncg_block = 16\n" % (d, npass)

    # labels = all and label = 3 from the seeded random start: the same V3
    wa, wb = str(tmp_path / "all"), str(tmp_path / "three")
    out_a = _run(LINEAR, wa, common + "labels = all\nfeature_scale = 255")
    _run(LINEAR, wb, common + "label = 3\nfeature_scale = 255")
    v_all, v_3 = hostlib.read_vec(os.path.join(wa, "V3")), hostlib.read_vec(os.path.join(wb, "V3"))
    assert np.abs(v_all - v_3).max() <= 1e-12 * np.abs(v_3).max()
    assert "Found file STOP" not in out_a
    for L in range(10):
        assert os.path.exists(os.path.join(wa, "W%d" % L)) and os.path.exists(os.path.join(wa, "V%d" % L))
    assert hostlib.read_sites(os.path.join(wa, "sites")) == (N_DRV, 2)

    # log lines against numpy from a known start (V%d files present: "Reading parameters from disk", :155), at lambda = 1e-3, where
    # every one of the 40 passes is insensitive to the order of the sums (stable_passes), so each printed cost is held to 1e-10
    wc = str(tmp_path / "logs")
    os.makedirs(wc)
    V0 = _start(10, N_DRV, 77)
    for L in range(10):
        hostlib.write_vec(os.path.join(wc, "V%d" % L), V0[L])
    lam = 1e-3
    out = _run(LINEAR, wc, common + "labels = all\nlambda = %g" % lam)
    assert out.count("Reading parameters from disk") == 10
    lines = re.findall(r"^L(\d)  (\d+) C = ([0-9.eE+-]+)$", out, flags=re.M)
    assert len(lines) == 10 * npass
    ev = re.findall(r"^Percent correct = ([0-9.]+)%, #correct = (\d+)/(\d+), #incorrect = (\d+)/(\d+)\nC \(= ([0-9.]+) \+ ([0-9.]+)\) = ([0-9.]+)$",
                    out, flags=re.M)
    assert len(ev) == 20                                 # train then test, ten labels each
    for L in range(10):
        y = np.where(labels == L, 1.0, -1.0)
        assert stable_passes(Xv, y, V0[L], lam, npass, 0.0) == npass
        Wr, cr = np_cgrad(Xv, y, V0[L], lam, npass)
        got = np.array([float(c) for l, p, c in lines if int(l) == L])
        assert [int(p) for l, p, c in lines if int(l) == L] == list(range(1, npass + 1))
        bad = np.nonzero(~(np.abs(got - cr) <= 1e-10 * cr + 5.1e-11))[0]                    # (+ the %.10f of the log line)
        assert len(bad) == 0, (L, bad, got[bad], cr[bad])
        Vf = hostlib.read_vec(os.path.join(wc, "V%d" % L))
        assert np.abs(Vf - Wr).max() <= 1e-9 * np.abs(Wr).max()
        for (Xs, ls, e) in ((Xv, labels, ev[L]), (Xt, tl, ev[10 + L])):
            nc, cnl = np_evaluate(Xs, ls, L, Vf)
            cl = lam * (Vf @ Vf)                                                              # :185 Cl = lambda V.V
            assert int(e[1]) == nc and int(e[2]) == len(ls) and int(e[3]) == len(ls) - nc
            assert abs(float(e[0]) - nc * 100.0 / len(ls)) <= 5.1e-5
            assert abs(float(e[5]) - cnl) <= 1e-10 * cnl + 5.1e-11
            assert abs(float(e[6]) - cl) <= 1e-10 * cl + 5.1e-11
            assert abs(float(e[7]) - (cnl + cl)) <= 1e-10 * (cnl + cl) + 5.1e-11
    assert "W entries are the reference's V(j)" in out

    # STOP at the first block boundary, file removed (:80-85)
    ws = str(tmp_path / "stop")
    os.makedirs(ws)
    open(os.path.join(ws, "STOP"), "w").close()
    out = _run(LINEAR, ws, common + "label = 5\ncg_block = 7")
    assert re.findall(r"^  (\d+) C = ", out, flags=re.M) == [str(i) for i in range(1, 8)]
    assert "Found file STOP, exiting" in out and not os.path.exists(os.path.join(ws, "STOP"))
    assert os.path.exists(os.path.join(ws, "W5"))

    # fixedL's W0..W9 branch in the labels = all directory, at the matching feature_scale
    out = _run(FIXEDL, wa, "datadir = %s\nNtrain = %d\nNbatch = 10\nNsweep = 1\nlambda = 0\nmaxm = 10\nfeature_scale = 255" % (d, PER_LABEL))
    assert "Found separate W0,W1,...,W9 MPS: summing" in out
    V = np.stack([hostlib.read_vec(os.path.join(wa, "V%d" % L)) for L in range(10)])
    P = Xv @ V.T                                          # [NT, 10]
    delta = (labels[:, None] == np.arange(10)[None, :]).astype(np.float64)
    cost = ((delta - P) ** 2).sum() / len(labels)
    m = re.search(r"Before starting DMRG Cost = ([0-9.]+)", out)
    assert m and abs(float(m.group(1)) - cost) <= 1e-7, (m and m.group(1), cost)
    pred = np.argmax(np.abs(P), axis=1)                   # first max of |P_l|
    ncor = int((pred == labels).sum())
    m = re.search(r"Percent correct = ([0-9.]+)%, # incorrect = (\d+)/(\d+)", out)
    assert m and int(m.group(2)) == len(labels) - ncor and int(m.group(3)) == len(labels)
