"""Streamed inference (tnml_predict_u8 / tnml_predict_phi, kernels_chain.hip): images a context does not hold, contracted with its W by
one launch of the chain kernel per chunk.  Truth is the oracle's per-image full contraction (toverlap); contexts are data-less unless
the test is about a training context."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TOL = 1e-11                        # the "costs" column of the fp64 row of test_gpu_parity.TOL

DIMS = [[1, 2, 3, 5, 9, 17, 33, 65, 120, 2, 1],
        [1, 2, 120, 97, 64, 60, 61, 128, 33, 2, 1],
        [1, 2, 4, 150, 129, 200, 300, 257, 16, 2, 1],
        [1, 2, 16, 512, 511, 130, 64, 2, 1]]          # the upper bound: the Label site (N = 8, site 4) carries 512 x 2 x 511 x 10


def _relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _mps_with_dims(dims, seed):
    """random weight MPS with the given bond dimensions d_0 = 1, d_1, ..., d_N = 1 (Label index on site N/2), any shapes"""
    rng = np.random.default_rng(seed)
    N = len(dims) - 1
    W = []
    for j in range(1, N + 1):
        ml, mr = dims[j - 1], dims[j]
        shape = (ml, 2, mr, 10) if j == N // 2 else (ml, 2, mr)
        A = rng.standard_normal(shape) / np.sqrt(2. * max(ml, mr) * (10 if j == N // 2 else 1))
        A[:, 0] += (np.eye(ml, mr) if A.ndim == 3 else np.eye(ml, mr)[:, :, None] / np.sqrt(10.))
        W.append(A)
    return W


def _dataless(N, maxm, W, single_label=None):
    """a context that holds no images: sized by W alone"""
    from tnml_amd.fixedl import TrainStates
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, maxm, no_data=True, single_label=single_label)
    ts.set_mps(W)
    return ts


def _toverlap(phi, labels, W):
    from oracle import pyoracle
    o = pyoracle.Oracle(phi, labels, W)
    return np.stack([o.toverlap(i) for i in range(len(labels))])


@functools.lru_cache(maxsize=None)
def _small(N, m):
    """70 images: (pixels, boosted features, W, truth on the boosted features, the byte feature map, truth on it)"""
    from oracle import pyoracle
    pixels, labels, phi, W = make_problem(N, 70, m, 3, pixel_boost=200.0)
    phi8 = pyoracle.features_series(pixels)
    return pixels, phi, W, _toverlap(phi, labels, W), phi8, _toverlap(phi8, labels, W)


@functools.lru_cache(maxsize=None)
def _odd(k):
    """40 images on the k-th list of bond dimensions: (pixels, boosted features, W, truth on them, truth on the byte feature map)"""
    from oracle import pyoracle
    dims = DIMS[k]
    N = len(dims) - 1
    pixels, labels, phi, _ = make_problem(N, 40, 2, 5, pixel_boost=200.0)
    W = _mps_with_dims(dims, 11)
    return pixels, phi, W, _toverlap(phi, labels, W), _toverlap(pyoracle.features_series(pixels), labels, W)


def _gap(truth):
    s = np.sort(np.abs(truth), axis=1)
    return ((s[:, -1] - s[:, -2]) / np.abs(truth).max()).min()


@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("N,m", [(12, 4), (4, 2), (17, 6)])
def test_predict_matches_toverlap(N, m, form):
    """both input forms on a data-less context against the oracle, every image's prediction included"""
    pixels, phi, W, t_phi, _, t_u8 = _small(N, m)
    ts = _dataless(N, m, W)
    w, pred = ts.predict(phi=phi) if form == "phi" else ts.predict(pixels=pixels)
    truth = t_phi if form == "phi" else t_u8
    print("relmax", _relmax(w, truth), "smallest top-two gap", _gap(truth))
    assert w.shape == (70, 10) and pred.shape == (70,)
    assert _relmax(w, truth) < 1e-12
    np.testing.assert_array_equal(pred, np.abs(truth).argmax(axis=1))
    w0, p0 = ts.predict(phi=phi[:0])                            # n = 0 succeeds and does nothing
    assert w0.shape == (0, 10) and p0.shape == (0,)
    ts.close()


@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("k", range(len(DIMS)))
def test_predict_every_tile_class_and_odd_shape(k, form):
    """bond dimensions 1, odd, ml != mr, up to 512: the three tile widths, masked rows and columns, the parked right-chain vector in
    LDS and in the global scratch.  Boosted features given, and the reference's own feature map from bytes."""
    pixels, phi, W, t_phi, t_u8 = _odd(k)
    ts = _dataless(len(W), max(DIMS[k]), W)
    w, pred = ts.predict(phi=phi) if form == "phi" else ts.predict(pixels=pixels)
    truth = t_phi if form == "phi" else t_u8
    print("relmax", _relmax(w, truth), "smallest top-two gap", _gap(truth))
    assert _relmax(w, truth) < 1e-11
    np.testing.assert_array_equal(pred, np.abs(truth).argmax(axis=1))
    ts.close()


def test_predict_refuses_a_bond_above_512():
    from tnml_amd.fixedl import TnmlError
    dims = [1, 2, 16, 513, 16, 2, 1]
    W = _mps_with_dims(dims, 11)
    ts = _dataless(len(W), 513, W)
    with pytest.raises(TnmlError, match="tnml_classify"):
        ts.predict(pixels=np.zeros((3, len(W)), dtype=np.uint8))
    ts.close()


def test_predict_is_independent_of_batch_chunk_and_tile():
    """an image's weights are the same bits wherever it lands: permuted batch, cut batch, five chunks, every tile width"""
    pixels, phi, W, truth, _, _ = _small(12, 4)
    ts = _dataless(12, 4, W)
    full = ts.predict(phi=phi)[0]
    assert _relmax(full, truth) < 1e-12
    perm = np.random.default_rng(5).permutation(70)
    wp = ts.predict(phi=phi[perm])[0]
    back = np.empty_like(wp)
    back[perm] = wp
    assert np.array_equal(back, full)
    cut = np.concatenate([ts.predict(phi=phi[a:b])[0] for a, b in ((0, 1), (1, 18), (18, 70))])
    assert np.array_equal(cut, full)
    ts.set_option("predict_chunk", 16)
    assert np.array_equal(ts.predict(phi=phi)[0], full)
    fresh = _dataless(12, 4, W)                                 # bytes in: chunks of 16 against one chunk on a fresh context
    assert np.array_equal(ts.predict(pixels=pixels)[0], fresh.predict(pixels=pixels)[0])
    fresh.close()
    ts.close()
    # bonds up to 120: a 40-image call and a 1-image call, chunks of 16, and the tile widths 64 / 32 / 16 forced
    pixels, phi, W, truth, _ = _odd(0)
    ts = _dataless(len(W), 120, W)
    full = ts.predict(phi=phi)[0]
    assert _relmax(full, truth) < 1e-11
    for i in (0, 39):
        assert np.array_equal(ts.predict(phi=phi[i:i + 1])[0], full[i:i + 1])
    for tile in (64, 32, 16):
        ts.set_option("predict_tile", tile)
        assert np.array_equal(ts.predict(phi=phi)[0], full), tile
        assert np.array_equal(ts.predict(phi=phi[39:])[0], full[39:]), tile
    ts.set_option("predict_tile", 0)
    ts.set_option("predict_chunk", 16)
    assert np.array_equal(ts.predict(phi=phi)[0], full)
    ts.close()


def test_predict_runs_the_chain_kernel_once_per_chunk():
    pixels, phi, W, truth, _, _ = _small(12, 4)
    ts = _dataless(12, 4, W)
    ts.set_option("predict_chunk", 16)
    ts.profile(True)
    ts.profile_reset()
    w = ts.predict(phi=phi)[0]
    prof = ts.profile_read()
    ts.profile(False)
    assert _relmax(w, truth) < 1e-12
    assert prof["chain"][0] == 5, prof
    assert prof["fgemm_shift"][0] == 0 and prof["fgemm_fwd"][0] == 0 and prof["labeldot"][0] == 0, prof
    ts.close()


def test_predict_workspace_does_not_grow_with_the_image_count():
    pixels, phi, W, _, _, t_u8 = _small(12, 4)
    ts = _dataless(12, 4, W)
    before = ts.device_bytes()
    assert before == ts.device_bytes()
    ts.predict(pixels=pixels[:64])
    small = ts.device_bytes()
    big_px = np.tile(pixels, (92, 1))[:6400]
    w = ts.predict(pixels=big_px)[0]
    assert ts.device_bytes() == small > before                  # allocated by the first call, not by tnml_create
    assert np.array_equal(w[:70], w[70:140]) and _relmax(w[:70], t_u8) < 1e-12
    ts.close()


def _train_pair():
    from oracle import pyoracle
    from tnml_amd.fixedl import TrainStates
    pixels, labels, phi, W = make_problem(12, 60, 4, 3, pixel_boost=200.0)
    ts = TrainStates(labels, 12, 4, phi=phi)
    o = pyoracle.Oracle(phi, labels, W)
    ts.set_mps(W)
    o.init()
    ts.init()
    return ts, o


def _same_report(a, b):
    for key in a:
        if key == "cg":
            assert a["cg"] == b["cg"]
        else:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


def test_predict_leaves_a_training_context_alone():
    from tnml_amd.fixedl import TnmlError, TrainStates
    sweep = (4, 2, 1e-10, 3, 1e-3, 1e-10)
    others = make_problem(12, 33, 4, 11, pixel_boost=200.0)
    ts, o = _train_pair()
    t_others = _toverlap(others[2], others[1], ts.get_mps())
    ts.setBond(1)
    o.set_bond(1)
    B0 = o.bond_tensor(1)
    P0 = ts.forward(B0)
    w, pred = ts.predict(phi=others[2])
    assert _relmax(w, t_others) < 1e-12
    np.testing.assert_array_equal(pred, np.abs(t_others).argmax(axis=1))
    assert np.array_equal(ts.forward(B0), P0)
    rep = ts.bond_update(1, 1, *sweep)
    ro = o.mldmrg(1, *sweep, max_bonds=1)[0]
    print("bond update cost", rep["cost"], "oracle", ro["cost"], "rel", abs(rep["cost"] - ro["cost"]) / abs(ro["cost"]))
    assert rep["newm"] == ro["newm"]
    assert abs(rep["cost"] - ro["cost"]) <= C_TOL * abs(ro["cost"])
    ts.close()
    # refused while a bond update is in flight; the report is that of a run without the attempt
    reports = []
    for attempt in (False, True):
        ts, _ = _train_pair()
        ts.bond_update_begin(1, 1, *sweep)
        if attempt:
            with pytest.raises(TnmlError, match="bond update is in flight"):
                ts.predict(phi=others[2])
        reports.append(ts.bond_update_end())
        ts.close()
    _same_report(reports[0], reports[1])
    # allowed while a held-out context is attached
    ts, _ = _train_pair()
    held = make_problem(12, 40, 4, 17, pixel_boost=200.0)
    hs = TrainStates(held[1], 12, 4, phi=held[2])
    ts.attach_heldout(hs)
    w = ts.predict(phi=others[2])[0]
    assert _relmax(w, t_others) < 1e-12
    with pytest.raises(TnmlError):                              # (the held-out lock itself is in place)
        ts.set_site(1, ts.get_site(1))
    with pytest.raises(TnmlError, match="attached as a held-out set"):   # the held-out context itself refuses, as it refuses classify:
        hs.predict(phi=others[2])                                         # train's bond updates rewrite its W from another stream
    ts.close()
    hs.close()


def test_predict_per_label_variant():
    """TNML_MODE_SINGLE: label extent 1, site 1 plays the centre, pred = [f > 1/2]"""
    from oracle import pyoracle
    from tnml_amd import synth
    N, NT, m = 12, 60, 4
    labels = synth.synthetic_labels(NT, seed=3, per_label=NT // 10)
    pixels = synth.synthetic_images(N, labels, seed=3)
    phi = pyoracle.features_single(pixels, True).copy()
    phi[..., 1] *= 300.0
    W = synth.random_mps(N, m, seed=10)
    W[N // 2 - 1] = W[N // 2 - 1][..., 0] * 3.0            # plain MPS: no Label index
    f = np.ones((NT, 1))
    for j, A in enumerate(W):
        f = np.einsum("na,nab->nb", f, np.einsum("ns,asb->nab", phi[:, j, :], A))
    ts = _dataless(N, m, W, single_label=3)
    w, pred = ts.predict(phi=phi)
    print("relmax", _relmax(w[:, 0], f[:, 0]), "closest to 1/2", np.abs(f[:, 0] - 0.5).min())
    assert w.shape == (NT, 1)
    assert _relmax(w[:, 0], f[:, 0]) < 1e-12
    np.testing.assert_array_equal(pred, (f[:, 0] > 0.5).astype(np.int32))
    ts.close()


def _table(out):
    """the result table of fullTest as the evaluators print it"""
    lines = [l for l in out.splitlines() if re.search(r"\d+/\d+ correct", l) or l.startswith("Total # test images")]
    assert len(lines) >= 3, out[-1500:]
    return lines


def _run(exe, inp, cwd):
    run = subprocess.run([os.path.join(ROOT, "tnml_amd", exe), str(inp)], capture_output=True, text=True, cwd=cwd, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    return run.stdout


def test_fulltest_driver_with_predict(tmp_path):
    """`fulltest` on the idx sets of test_fixedl_cli_driver_end_to_end with the W that run starts from (no training here: the start W
    already spreads its predictions over eight labels): predict = yes prints the table of predict = no, which is the oracle's, plus the
    line that names the device path; bytes in (series) and features in (normal); chunks of 48, so the 130 images take three launches"""
    from oracle import pyoracle
    from tnml_amd import hostlib, synth
    N, per_label = 16, 20
    labels = synth.synthetic_labels(10 * per_label, seed=9, per_label=per_label)
    pixels = np.clip(synth.synthetic_images(N, labels, seed=9).astype(np.int32) * 3, 0, 255).astype(np.uint8)
    data = str(tmp_path / "data")
    synth.write_idx(data, pixels, labels)
    tl = synth.synthetic_labels(130, seed=21)
    tp = np.clip(synth.synthetic_images(N, tl, seed=21).astype(np.int32) * 3, 0, 255).astype(np.uint8)
    synth.write_idx(data, tp, tl, train=False)
    hostlib.build_initial_w(data, per_label, 3, 5, str(tmp_path / "W"))
    hostlib.write_sites(str(tmp_path / "sites"), N)
    Wf = hostlib.read_mps(str(tmp_path / "W"))
    for feat, entry, phi_t in (("series", "tnml_predict_u8", pyoracle.features_series(tp)),
                               ("normal", "tnml_predict_phi", np.stack([np.cos(np.pi / 2 * tp / 65025.), np.sin(np.pi / 2 * tp / 65025.)], axis=-1))):
        pred = np.abs(_toverlap(phi_t, tl, Wf)).argmax(axis=1)
        assert len(set(pred.tolist())) >= 5                     # not a constant prediction: a misplaced chunk would change the table
        outs = {}
        for mode in ("no", "yes"):
            tin = tmp_path / ("input_%s_%s" % (feat, mode))
            tin.write_text("input\n{\ndatadir = %s\nfname = W\nfeature = %s\nprecision = f64\npredict = %s\npredict_chunk = 48\n}\n" % (data, feat, mode))
            outs[mode] = _run("fulltest", tin, tmp_path)
        assert _table(outs["yes"]) == _table(outs["no"])
        digits = re.findall(r"Digit (\d) (\d+)/(\d+) correct", outs["yes"])
        assert [(int(a), int(b), int(c)) for a, b, c in digits] == \
            [(l, int(((pred == tl) & (tl == l)).sum()), int((tl == l).sum())) for l in range(10) if (tl == l).any()]
        assert "Total # test images = 130" in outs["yes"]
        assert "Device path: streamed chain kernel (%s), 48 images per chunk" % entry in outs["yes"]
        assert "Device path" not in outs["no"]
        assert outs["yes"].index("Device path") < outs["yes"].index(_table(outs["yes"])[0])


def test_separate_fulltest_driver_with_predict(tmp_path):
    """`separate_fulltest` on the idx sets and the input file of test_single_and_separate_fulltest_cli with the ten W<n> those trainings
    start from; chunks of 50, so the 120 images take three launches per W<n>; the table is also the oracle's"""
    from oracle import pyoracle
    from tnml_amd import hostlib, synth
    N, per_label = 16, 16
    labels = synth.synthetic_labels(10 * per_label, seed=6, per_label=per_label)
    tl = synth.synthetic_labels(120, seed=23)
    allpx = np.clip(synth.synthetic_images(N, np.concatenate([labels, tl]), seed=6).astype(np.int32) * 3, 0, 255).astype(np.uint8)
    data = str(tmp_path / "data")
    synth.write_idx(data, allpx[:len(labels)], labels)
    synth.write_idx(data, allpx[len(labels):], tl, train=False)
    for L in range(10):
        (tmp_path / ("L%d" % L)).mkdir()
        hostlib.build_initial_single(data, per_label, L, 3, 4, True, str(tmp_path / ("L%d" % L) / ("W%d" % L)))
    hostlib.write_sites(str(tmp_path / "sites"), N)
    outs = {}
    for mode in ("no", "yes"):
        tin = tmp_path / ("input_" + mode)
        tin.write_text("input\n{\ndatadir = %s\nfeature_scale = 1\nimglen = 4\npredict = %s\npredict_chunk = 50\n}\n" % (data, mode))
        outs[mode] = _run("separate_fulltest", tin, tmp_path)
    assert _table(outs["yes"]) == _table(outs["no"])
    assert "Total # test images = 120" in outs["yes"]
    assert "Device path: streamed chain kernel (tnml_predict_phi), 50 images per chunk" in outs["yes"] and "Device path" not in outs["no"]
    assert outs["yes"].index("Device path") < outs["yes"].index(_table(outs["yes"])[0])
    tp = allpx[len(labels):]
    phit = pyoracle.features_single(tp, True)
    O = np.zeros((10, len(tl)))
    for L in range(10):
        oo = pyoracle.SingleOracle(phit, tl, L, hostlib.read_mps(str(tmp_path / ("L%d" % L) / ("W%d" % L))))
        O[L] = [oo.output(i) for i in range(len(tl))]
    pred = np.abs(O).argmax(axis=0)
    print("predicted labels", np.bincount(pred, minlength=10))
    assert len(set(pred.tolist())) >= 3                         # not a constant prediction
    digits = re.findall(r"Digit (\d) (\d+)/(\d+) correct", outs["yes"])
    assert [(int(a), int(b), int(c)) for a, b, c in digits] == \
        [(l, int(((pred == tl) & (tl == l)).sum()), int((tl == l).sum())) for l in range(10) if (tl == l).any()]
    costs = {k: [float(x) for x in re.findall(r"Digit \d C = ([0-9.eE+-]+)", v)] for k, v in outs.items()}
    assert len(costs["yes"]) == 10
    np.testing.assert_allclose(costs["yes"], costs["no"], rtol=1e-10)
