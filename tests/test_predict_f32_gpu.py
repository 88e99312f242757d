"""Streamed inference in fp32 (option predict_dtype = 1, k_chain<float> in kernels_chain.hip) against the bit-exact model of its arithmetic
(chain32_model.py, proved on the host by test_chain32_model_host.py): np.array_equal on the weights and on pred, never a tolerance.
Contexts are data-less unless the test is about a training context."""
import os
import re
import subprocess

import numpy as np
import pytest

import chain32_cases as cases
import chain32_model as cm
from conftest import make_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dataless(N, maxm, W, single_label=None):
    from tnml_amd.fixedl import TrainStates
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, maxm, no_data=True, single_label=single_label)
    ts.set_mps(W)
    return ts


def _predict(ts, kind, key, form, sl=slice(None), dtype="f32"):
    pixels, f, _ = cases.inputs(kind, key)
    return ts.predict(phi=f["phi"][sl], dtype=dtype) if form == "phi" else ts.predict(pixels=pixels[sl], dtype=dtype)


@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("N,m", cases.SMALL)
def test_f32_small_problems_are_the_model_bit_for_bit(N, m, form):
    _, _, W = cases.inputs("small", (N, m))
    wm, pm = cases.model("small", (N, m), form)
    truth = cases.oracle("small", (N, m), form)
    ts = _dataless(N, m, W)
    w, pred = _predict(ts, "small", (N, m), form)
    print("relmax against the oracle", np.abs(w - truth).max() / np.abs(truth).max(), "bits differ in", int((w != wm).sum()), "weights")
    assert w.shape == (70, 10) and pred.shape == (70,) and w.dtype == np.float64
    assert np.array_equal(w, wm)
    assert np.array_equal(w, w.astype(np.float32).astype(np.float64))         # fp32 results widened
    assert np.array_equal(pred, pm)
    assert np.array_equal(pred, np.abs(truth).argmax(axis=1))                 # the oracle's argmax on every image
    w0, p0 = _predict(ts, "small", (N, m), form, slice(0, 0))                 # n = 0 succeeds and does nothing
    assert w0.shape == (0, 10) and p0.shape == (0,)
    ts.close()


@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("k", range(len(cases.DIMS)))
def test_f32_every_tile_class_and_odd_shape(k, form):
    """bond dimensions 1, odd, ml != mr, up to 1 024: masked rows and columns, R parked in LDS and in the global scratch, and every tile
    width the fp32 cap allows at the list's largest bond (64 up to 256, 32 up to 512, 16 up to 1 024), forced through predict_tile"""
    _, _, W = cases.inputs("dims", k)
    wm, pm = cases.model("dims", k, form)
    truth = cases.oracle("dims", k, form)
    top = max(cases.DIMS[k])
    ts = _dataless(len(W), top, W)
    cap = 64 if top <= 256 else (32 if top <= 512 else 16)
    for tile in [0] + [t for t in (64, 32, 16) if t <= cap]:
        ts.set_option("predict_tile", tile)
        w, pred = _predict(ts, "dims", k, form)
        print("tile", tile, "relmax against the oracle", np.abs(w - truth).max() / np.abs(truth).max(), "bits differ in", int((w != wm).sum()), "weights")
        assert np.array_equal(w, wm), tile
        assert np.array_equal(pred, pm), tile
    assert np.array_equal(pm, np.abs(truth).argmax(axis=1))
    ts.close()


def test_f32_is_independent_of_batch_chunk_and_tile():
    """an image's fp32 weights are the same bits wherever it lands"""
    _, f, W = cases.inputs("small", (12, 4))
    phi = f["phi"]
    full = cases.model("small", (12, 4), "phi")[0]
    ts = _dataless(12, 4, W)
    assert np.array_equal(ts.predict(phi=phi, dtype="f32")[0], full)
    perm = np.random.default_rng(5).permutation(70)
    assert np.array_equal(ts.predict(phi=phi[perm])[0], full[perm])
    cut = np.concatenate([ts.predict(phi=phi[a:b])[0] for a, b in ((0, 1), (1, 18), (18, 70))])
    assert np.array_equal(cut, full)
    ts.set_option("predict_chunk", 16)
    assert np.array_equal(ts.predict(phi=phi)[0], full)
    ts.set_option("predict_chunk", 8192)
    for tile in (64, 32, 16):
        ts.set_option("predict_tile", tile)
        assert np.array_equal(ts.predict(phi=phi)[0], full), tile
        assert np.array_equal(ts.predict(phi=phi[69:])[0], full[69:]), tile          # a 1-image call
    ts.close()
    pixels, _, W = cases.inputs("dims", 0)                    # bonds up to 120, bytes in, 40 images
    full, pm = cases.model("dims", 0, "u8")
    ts = _dataless(len(W), 120, W)
    ts.set_option("predict_dtype", 1)
    for tile in (64, 32, 16):
        ts.set_option("predict_tile", tile)
        for i in (0, 39):
            w1, p1 = ts.predict(pixels=pixels[i:i + 1])
            assert np.array_equal(w1, full[i:i + 1]) and np.array_equal(p1, pm[i:i + 1]), (tile, i)
    ts.set_option("predict_tile", 0)
    ts.set_option("predict_chunk", 16)
    assert np.array_equal(ts.predict(pixels=pixels)[0], full)
    ts.close()


def test_f32_per_label_variant():
    """TNML_MODE_SINGLE: label extent 1, site 1 plays the centre, pred = [w > 0.5f] on the fp32 value"""
    phi, W, f = cases.per_label_problem()
    wm, pm = cm.predict32(W, phi, single=True)
    ts = _dataless(12, 4, W, single_label=3)
    w, pred = ts.predict(phi=phi, dtype="f32")
    assert w.shape == (60, 1)
    assert np.array_equal(w, wm)
    assert np.array_equal(pred, pm)
    assert np.array_equal(pred, (f[:, 0] > 0.5).astype(np.int32))
    ts.close()


def test_f32_under_an_input_map():
    """7 x 6 source, 2 x 2 blocks from (1, 0), 3 x 3 sites: row 0 is covered by no block; a random table, so a look-up and not an
    expression.  The model takes fl32(table[codes])."""
    from tnml_amd.input_map import InputMap
    rng = np.random.default_rng(77)
    ncodes = 255 * 4 + 1
    table = np.stack([1. + 0.1 * rng.standard_normal(ncodes), 0.5 * rng.standard_normal(ncodes)], axis=-1)
    m = InputMap(7, 6, 2, 1, 0, 3, 3, table)
    px = rng.integers(0, 256, (150, m.S), dtype=np.uint8)
    px[0] = 0
    px[1] = 255
    W = cases.mps_with_dims([1, 2, 5, 6, 3, 6, 4, 5, 2, 1], 5)
    wm, pm = cm.predict32(W, m.features(px))
    ts = _dataless(m.N, 6, W)
    ts.set_input_map(m)
    ts.set_option("predict_chunk", 64)                         # chunks of 64, 64 and 22
    for tile in (0, 16, 32, 64):
        ts.set_option("predict_tile", tile)
        w, pred = ts.predict(pixels=px, dtype="f32")
        assert np.array_equal(w, wm), tile
        assert np.array_equal(pred, pm), tile
    wf = ts.predict(phi=m.features(px))[0]                     # the same features given: the same bits
    assert np.array_equal(wf, wm)
    ts.close()


def test_switching_the_option_and_the_workspace():
    pixels, f, W = cases.inputs("small", (12, 4))
    wm = cases.model("small", (12, 4), "u8")[0]
    fresh = _dataless(12, 4, W)                                 # never sees the option
    w64, p64 = fresh.predict(pixels=pixels)
    only64 = fresh.device_bytes()
    fresh.close()
    ts = _dataless(12, 4, W)
    before = ts.device_bytes()
    ts.predict(pixels=pixels[:64], dtype="f32")
    small = ts.device_bytes()
    E = sum((A.size + 3) // 4 * 4 for A in W)
    print("device bytes: fp64 only", only64 - before, "fp32 on top", small - only64, "expected", 16 * 12 + 4 + 4 * E)
    assert small - only64 == 16 * 12 + 4 + 4 * E               # site table, range flag, the fp32 copy of W
    big = np.tile(pixels, (90, 1))
    ts.profile(True)
    ts.profile_reset()
    w = ts.predict(pixels=big)[0]
    prof = ts.profile_read()
    ts.profile(False)
    assert ts.device_bytes() == small > before                  # 90 x the images: no growth
    assert np.array_equal(w[:70], wm) and np.array_equal(w[-70:], wm)
    assert prof["chain"][0] == 1 and prof["pack"][0] == 2, prof          # one chunk: one staging kernel + one conversion of W
    w, p = ts.predict(pixels=pixels, dtype="f64")               # back to fp64 on the same context: the bits of the fresh context
    assert np.array_equal(w, w64) and np.array_equal(p, p64)
    assert not np.array_equal(w, wm)
    ts.set_option("predict_dtype", 1)
    assert np.array_equal(ts.predict(pixels=pixels)[0], wm)
    ts.close()


def test_f32_follows_a_W_that_changes_between_calls():
    """the fp32 copy is made per call, and grows with W"""
    _, f, W = cases.inputs("small", (12, 4))
    ts = _dataless(12, 8, W)
    assert np.array_equal(ts.predict(phi=f["phi"], dtype="f32")[0], cases.model("small", (12, 4), "phi")[0])
    b0 = ts.device_bytes()
    W2 = cases.mps_with_dims([1, 2, 4, 8, 7, 8, 5, 8, 8, 6, 4, 2, 1], 3)
    ts.set_mps(W2)
    assert np.array_equal(ts.predict(phi=f["phi"])[0], cm.chain32(W2, f["phi"]))
    assert ts.device_bytes() > b0
    ts.close()


def test_f32_refusals():
    from tnml_amd.fixedl import TnmlError
    W = cases.mps_with_dims([1, 2, 16, 1025, 16, 2, 1], 11)
    ts = _dataless(len(W), 1025, W)
    with pytest.raises(TnmlError, match=r"1025.*up to 1024.*tnml_classify"):
        ts.predict(pixels=np.zeros((3, len(W)), dtype=np.uint8), dtype="f32")
    with pytest.raises(TnmlError, match="predict_dtype"):
        ts.set_option("predict_dtype", 2)
    with pytest.raises(TnmlError, match="predict_dtype"):
        ts.set_option("predict_dtype", -1)
    with pytest.raises(ValueError):
        ts.predict(pixels=np.zeros((3, len(W)), dtype=np.uint8), dtype="bf16")
    ts.close()


def test_f32_leaving_the_range_fails_and_fp64_still_works():
    from tnml_amd.fixedl import TnmlError
    _, f, W = cases.inputs("small", (12, 4))
    phi = f["phi"]
    Wbig = [A * 1e5 for A in W]                                 # the weights reach 1e60: far outside fp32, well inside fp64
    ts = _dataless(12, 4, Wbig)
    with pytest.raises(TnmlError, match=r"predict_dtype.*fp64"):
        ts.predict(phi=phi, dtype="f32")
    w, pred = ts.predict(phi=phi, dtype="f64")
    truth = cases.oracle("small", (12, 4), "phi")
    assert np.isfinite(w).all()
    assert np.abs(w / 1e60 - truth).max() / np.abs(truth).max() < 1e-12
    assert np.array_equal(pred, np.abs(truth).argmax(axis=1))
    ts.set_mps(W)                                               # and fp32 again, in range: the flag does not stick
    assert np.array_equal(ts.predict(phi=phi, dtype="f32")[0], cases.model("small", (12, 4), "phi")[0])
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


def test_f32_leaves_a_training_context_alone():
    from oracle import pyoracle
    from tnml_amd.fixedl import TnmlError
    sweep = (4, 2, 1e-10, 3, 1e-3, 1e-10)
    others = make_problem(12, 33, 4, 11, pixel_boost=200.0)
    ts, o = _train_pair()
    ts.setBond(1)
    o.set_bond(1)
    B0 = o.bond_tensor(1)
    P0 = ts.forward(B0)
    w, pred = ts.predict(phi=others[2], dtype="f32")
    wm, pm = cm.predict32(ts.get_mps(), others[2])
    assert np.array_equal(w, wm) and np.array_equal(pred, pm)
    assert np.array_equal(ts.forward(B0), P0)
    ts.close()
    reports = []
    for attempt in (False, True):
        ts, _ = _train_pair()
        ts.bond_update_begin(1, 1, *sweep)
        if attempt:
            with pytest.raises(TnmlError, match="bond update is in flight"):
                ts.predict(phi=others[2], dtype="f32")
        reports.append(ts.bond_update_end())
        ts.close()
    _same_report(reports[0], reports[1])


def _table(out):
    lines = [l for l in out.splitlines() if re.search(r"\d+/\d+ correct", l) or l.startswith("Total # test images")]
    assert len(lines) >= 3, out[-1500:]
    return lines


def _run(exe, inp, cwd):
    run = subprocess.run([os.path.join(ROOT, "tnml_amd", exe), str(inp)], capture_output=True, text=True, cwd=cwd, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    return run.stdout


def _digit_counts(out):
    return [(int(a), int(b), int(c)) for a, b, c in re.findall(r"Digit (\d) (\d+)/(\d+) correct", out)]


def _expected_counts(pred, tl):
    return [(l, int(((pred == tl) & (tl == l)).sum()), int((tl == l).sum())) for l in range(10) if (tl == l).any()]


def test_fulltest_driver_with_predict_dtype(tmp_path):
    """the inputs of test_fulltest_driver_with_predict; predict_dtype = f32: the table of the model's predictions, the line names fp32;
    predict_dtype = f64: the output of the key left out; predict = no with f32: said once to be ignored"""
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
    for feat, entry, phi_t in (("series", "tnml_predict_u8", cm.features_u8(tp)),
                               ("normal", "tnml_predict_phi", np.stack([np.cos(np.pi / 2 * tp / 65025.), np.sin(np.pi / 2 * tp / 65025.)], axis=-1))):
        pred = cm.predict32(Wf, phi_t)[1]
        assert len(set(pred.tolist())) >= 5
        outs = {}
        for mode, extra in (("none", ""), ("f64", "predict_dtype = f64\n"), ("f32", "predict_dtype = f32\n")):
            tin = tmp_path / ("input_%s_%s" % (feat, mode))
            tin.write_text("input\n{\ndatadir = %s\nfname = W\nfeature = %s\nprecision = f64\npredict = yes\npredict_chunk = 48\n%s}\n" % (data, feat, extra))
            outs[mode] = _run("fulltest", tin, tmp_path)
        assert outs["f64"] == outs["none"]
        assert _digit_counts(outs["f32"]) == _expected_counts(pred, tl)
        assert "Total # test images = 130" in outs["f32"]
        assert "Device path: streamed chain kernel (%s, fp32), 48 images per chunk" % entry in outs["f32"]
        assert "fp32" not in outs["f64"]
    tin = tmp_path / "input_ignored"
    tin.write_text("input\n{\ndatadir = %s\nfname = W\nfeature = series\nprecision = f64\npredict = no\npredict_dtype = f32\n}\n" % data)
    out = _run("fulltest", tin, tmp_path)
    assert out.count("predict_dtype = f32 is ignored") == 1 and "Device path" not in out


def test_separate_fulltest_driver_with_predict_dtype(tmp_path):
    """the inputs of test_separate_fulltest_driver_with_predict; the table is that of the ten per-label models"""
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
    for mode, extra in (("none", ""), ("f64", "predict_dtype = f64\n"), ("f32", "predict_dtype = f32\n")):
        tin = tmp_path / ("input_" + mode)
        tin.write_text("input\n{\ndatadir = %s\nfeature_scale = 1\nimglen = 4\npredict = yes\npredict_chunk = 50\n%s}\n" % (data, extra))
        outs[mode] = _run("separate_fulltest", tin, tmp_path)
    assert outs["f64"] == outs["none"]
    assert "Device path: streamed chain kernel (tnml_predict_phi, fp32), 50 images per chunk" in outs["f32"]
    phit = pyoracle.features_single(allpx[len(labels):], True)
    O = np.stack([cm.chain32(hostlib.read_mps(str(tmp_path / ("L%d" % L) / ("W%d" % L))), phit)[:, 0] for L in range(10)])
    pred = np.abs(O).argmax(axis=0)
    assert len(set(pred.tolist())) >= 3
    assert _digit_counts(outs["f32"]) == _expected_counts(pred, tl)
    assert "Total # test images = 120" in outs["f32"]
