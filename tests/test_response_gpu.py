"""Streamed site responses (tnml_response_u8 / tnml_response_phi, kernels_response.hip): resp[n, j, s], the output of the chosen label
for image n with the feature of site j replaced by e_s.  The yardstick is tests/response_model.py (held to the oracle by
tests/test_response_model_host.py); contexts are data-less unless the test is about a training context."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import make_problem
from response_model import response

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11                         # per site, relative to the site's largest |resp|: the bound of the predict tests on these shapes

DIMS = [[1, 2, 3, 5, 9, 17, 33, 65, 120, 2, 1],
        [1, 2, 120, 97, 64, 60, 61, 128, 33, 2, 1],
        [1, 2, 4, 150, 129, 200, 300, 257, 16, 2, 1],
        [1, 2, 16, 512, 511, 130, 64, 2, 1]]          # the Label site (N = 8, site 4) carries 512 x 2 x 511 x 10


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


def _which(n, seed, nl=10):
    return np.random.default_rng(seed).integers(0, nl, size=n).astype(np.int32)


def _site_err(got, model):
    """per site: max over images and s of |got - model|, over the site's largest |model|"""
    return np.abs(got - model).max(axis=(0, 2)) / np.abs(model).max(axis=(0, 2))


@functools.lru_cache(maxsize=None)
def _odd(k):
    """40 images on the k-th list of bond dimensions: (pixels, boosted features, byte features, W)"""
    from oracle import pyoracle
    dims = DIMS[k]
    N = len(dims) - 1
    pixels, _, phi, _ = make_problem(N, 40, 2, 5, pixel_boost=200.0)
    return pixels, phi, pyoracle.features_series(pixels), _mps_with_dims(dims, 11)


@functools.lru_cache(maxsize=None)
def _small(N, m):
    """70 images: (pixels, boosted features, byte features, W)"""
    from oracle import pyoracle
    pixels, _, phi, W = make_problem(N, 70, m, 3, pixel_boost=200.0)
    return pixels, phi, pyoracle.features_series(pixels), W


@functools.lru_cache(maxsize=None)
def _model(kind, key, form, chosen):
    """the model on _odd(key) / _small(*key), once per case: (resp, weights, label)"""
    pixels, phi, phi8, W = _odd(key) if kind == "odd" else _small(*key)
    which = None if chosen == "own" else _which(len(pixels), 17)
    return response(W, phi if form == "phi" else phi8, which)


def _check_against_model(ts, kind, key, form, chosen):
    pixels, phi, phi8, W = _odd(key) if kind == "odd" else _small(*key)
    n = len(pixels)
    which = None if chosen == "own" else _which(n, 17)
    src = dict(phi=phi) if form == "phi" else dict(pixels=pixels)
    m_resp, m_w, m_label = _model(kind, key, form, chosen)
    resp, (w, pred) = ts.site_response(which=which, want_weights=True, **src)
    err = _site_err(resp, m_resp)
    s = np.sort(np.abs(m_w), axis=1)
    print("per-site error", err.max(), "smallest top-two gap", ((s[:, -1] - s[:, -2]) / np.abs(m_w).max()).min())
    assert resp.shape == (n, len(W), 2)
    assert err.max() < TOL, err
    wp, pp = ts.predict(**src)
    assert np.array_equal(w, wp) and np.array_equal(pred, pp)           # the inward pass is the chain kernel's, bit for bit
    if which is None:
        np.testing.assert_array_equal(pred, m_label)
    # multilinearity on the device alone: the image's own feature at any site gives back the weight of the chosen label
    feats = phi if form == "phi" else phi8
    label = pred if which is None else which
    ident = (feats * resp).sum(axis=2)                                    # [n, N]
    dev = np.abs(ident - w[np.arange(n), label][:, None]).max() / np.abs(w).max()
    print("identity", dev)
    assert dev < TOL
    return resp, w, label


@pytest.mark.parametrize("chosen", ["own", "given"])
@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("k", range(len(DIMS)))
def test_response_matches_the_model_on_every_tile_class_and_odd_shape(k, form, chosen):
    """bonds of 1, odd bonds, ml != mr, masked last blocks, the three tile widths, the Label site at 512 x 2 x 511 x 10"""
    ts = _dataless(len(DIMS[k]) - 1, max(DIMS[k]), _odd(k)[3])
    _check_against_model(ts, "odd", k, form, chosen)
    ts.close()


@pytest.mark.parametrize("chosen", ["own", "given"])
@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("N,m", [(4, 2), (4, 3), (12, 4), (12, 5), (17, 6)])
def test_response_short_chains(N, m, form, chosen):
    ts = _dataless(N, m, _small(N, m)[3])
    _check_against_model(ts, "small", (N, m), form, chosen)
    r0 = ts.site_response(phi=_small(N, m)[1][:0])                       # n = 0 succeeds and does nothing
    assert r0.shape == (0, N, 2)
    ts.close()


@pytest.mark.parametrize("N", [2, 3])
def test_chains_below_four_sites_are_refused_at_creation(N):
    """tnml.h: N = 2 and N = 3 do not reach tnml_response_*, tnml_create refuses them with a message"""
    from tnml_amd.fixedl import TnmlError, TrainStates
    with pytest.raises(TnmlError, match="N >= 4"):
        TrainStates(np.zeros(1, dtype=np.int32), N, 2, no_data=True)


def test_response_predicts_a_changed_byte():
    """first site, Label site, last site: predict() on the image with that byte changed is phi(g') . resp of the unchanged image"""
    from oracle import pyoracle
    N, m = 12, 4
    pixels, _, _, W = _small(N, m)
    ts = _dataless(N, m, W)
    resp, (w, pred) = ts.site_response(pixels=pixels, want_weights=True)
    rng = np.random.default_rng(23)
    rows = np.arange(len(pixels))
    for j in (0, N // 2 - 1, N - 1):
        changed = pixels.copy()
        changed[:, j] = (pixels[:, j].astype(np.int32) + rng.integers(1, 256, size=len(pixels))) % 256     # every byte really changes
        f = pyoracle.features_series(changed)[:, j]                     # phi(g')
        w2 = ts.predict(pixels=changed)[0]
        dev = np.abs((f * resp[:, j]).sum(axis=1) - w2[rows, pred]).max() / np.abs(w2).max()
        print("site", j + 1, "changed byte", dev)
        assert dev < TOL
    # and with given features: any psi at a site
    _, phi, _, _ = _small(N, m)
    resp = ts.site_response(phi=phi, which=_which(70, 3))
    for j in (0, N // 2 - 1, N - 1):
        changed = phi.copy()
        changed[:, j] = rng.standard_normal((70, 2))
        w2 = ts.predict(phi=changed)[0]
        dev = np.abs((changed[:, j] * resp[:, j]).sum(axis=1) - w2[rows, _which(70, 3)]).max() / np.abs(w2).max()
        print("site", j + 1, "changed feature", dev)
        assert dev < TOL
    ts.close()


@pytest.mark.parametrize("kind,key,maxm", [("small", (12, 4), 4), ("odd", 0, 120)])
def test_response_is_independent_of_batch_chunk_and_tile(kind, key, maxm):
    """an image's responses are the same bits wherever it lands"""
    pixels, phi, _, W = _odd(key) if kind == "odd" else _small(*key)
    n = len(pixels)
    which = _which(n, 29)
    ts = _dataless(len(W), maxm, W)
    for src, wh in ((dict(phi=phi), None), (dict(pixels=pixels), which)):
        cut = lambda a, b, perm=None: ts.site_response(which=None if wh is None else (wh[a:b] if perm is None else wh[perm]),
                                                       **{k: (v[a:b] if perm is None else v[perm]) for k, v in src.items()})
        ts.set_option("response_chunk", 1024)
        ts.set_option("predict_tile", 0)
        full = cut(0, n)
        assert np.array_equal(cut(0, n), full)                          # repeats
        perm = np.random.default_rng(5).permutation(n)
        back = np.empty_like(full)
        back[perm] = cut(0, n, perm)
        assert np.array_equal(back, full)
        cuts = ((0, 1), (1, 18), (18, n))
        assert np.array_equal(np.concatenate([cut(a, b) for a, b in cuts]), full)
        for i in (0, n - 1):
            assert np.array_equal(cut(i, i + 1), full[i:i + 1])
        for tile in (64, 32, 16):
            ts.set_option("predict_tile", tile)
            assert np.array_equal(cut(0, n), full), tile
            assert np.array_equal(cut(n - 1, n), full[n - 1:]), tile
        ts.set_option("predict_tile", 0)
        ts.set_option("response_chunk", 16)
        assert np.array_equal(cut(0, n), full)
    ts.close()


def test_response_per_label_variant():
    """TNML_MODE_SINGLE: one output, site 1 plays the centre, no left chain; which must be NULL or all zero"""
    from oracle import pyoracle
    from tnml_amd import synth
    from tnml_amd.fixedl import TnmlError
    N, NT, m = 12, 60, 4
    labels = synth.synthetic_labels(NT, seed=3, per_label=NT // 10)
    pixels = synth.synthetic_images(N, labels, seed=3)
    phi = pyoracle.features_single(pixels, True).copy()
    phi[..., 1] *= 300.0
    W = synth.random_mps(N, m, seed=10)
    W[N // 2 - 1] = W[N // 2 - 1][..., 0] * 3.0            # plain MPS: no Label index
    m_resp, m_w, _ = response(W, phi)
    ts = _dataless(N, m, W, single_label=3)
    resp, (w, pred) = ts.site_response(phi=phi, want_weights=True)
    err = _site_err(resp, m_resp)
    print("per-site error", err.max())
    assert err.max() < TOL, err
    wp, pp = ts.predict(phi=phi)
    assert w.shape == (NT, 1) and np.array_equal(w[:, 0], wp[:, 0]) and np.array_equal(pred, pp)
    assert np.array_equal(ts.site_response(phi=phi, which=np.zeros(NT, dtype=np.int32)), resp)
    bad = np.zeros(NT, dtype=np.int32)
    bad[7] = 1
    with pytest.raises(TnmlError, match="image 7"):
        ts.site_response(phi=phi, which=bad)
    assert np.array_equal(ts.site_response(phi=phi), resp)
    ts.close()


def test_response_under_an_input_map():
    """raw 28 x 28 bytes through the device input map: the bits of the feature path on the features the map defines"""
    from tnml_amd import synth
    from tnml_amd.input_map import InputMap
    m = InputMap.from_imglen(28, 14, "normal")
    raw = np.random.default_rng(8).integers(0, 256, size=(20, m.S)).astype(np.uint8)
    W = synth.random_mps(m.N, 6, seed=4)
    ts = _dataless(m.N, 6, W)
    ref, (w_ref, p_ref) = ts.site_response(phi=m.features(raw), want_weights=True)
    ts.set_input_map(m)
    got, (w, p) = ts.site_response(pixels=raw, want_weights=True)
    assert got.shape == (20, m.N, 2) and np.abs(got).max() > 0
    assert np.array_equal(got, ref) and np.array_equal(w, w_ref) and np.array_equal(p, p_ref)
    wp, pp = ts.predict(pixels=raw)
    assert np.array_equal(w, wp) and np.array_equal(p, pp)
    ts.close()


def test_response_bookkeeping():
    """one launch per chunk and none of the chain kernel; a workspace of its own that does not grow with the image count and leaves
    predict's bytes alone"""
    N, m = 12, 4
    pixels, phi, _, W = _small(N, m)
    ts = _dataless(N, m, W)
    before = ts.device_bytes()
    ts.set_option("response_chunk", 16)
    ts.profile(True)
    ts.profile_reset()
    r16 = ts.site_response(phi=phi)
    prof = ts.profile_read()
    ts.profile(False)
    assert prof["site_resp"][0] == 5 and prof["chain"][0] == 0, prof
    assert prof["fgemm_shift"][0] == 0 and prof["fgemm_fwd"][0] == 0 and prof["labeldot"][0] == 0, prof
    ts.close()
    ts = _dataless(N, m, W)
    assert ts.device_bytes() == before                          # a re-created context starts where the first one did
    ts.predict(pixels=pixels[:64])
    with_predict = ts.device_bytes()
    r = ts.site_response(pixels=pixels[:64])
    small = ts.device_bytes()
    assert small > with_predict > before                        # allocated by the first call
    big = ts.site_response(pixels=np.tile(pixels, (92, 1))[:6400])
    assert ts.device_bytes() == small
    assert np.array_equal(big[:70], big[70:140]) and np.array_equal(big[:64], r)
    ts.predict(pixels=pixels)
    assert ts.device_bytes() == small                           # predict's workspace is what it was
    ts.close()
    ts = _dataless(N, m, W)
    ts.site_response(pixels=pixels[:64])
    assert ts.device_bytes() - before == small - with_predict   # the response workspace counts the same with and without predict's
    assert np.array_equal(ts.site_response(phi=phi), r16)
    assert ts.site_response(pixels=pixels[:0]).shape == (0, N, 2)
    ts.close()


def test_response_refusals_leave_the_context_usable():
    from tnml_amd.fixedl import TnmlError
    W513 = _mps_with_dims([1, 2, 16, 513, 16, 2, 1], 11)
    ts = _dataless(len(W513), 513, W513)
    with pytest.raises(TnmlError, match="tnml_classify"):
        ts.site_response(pixels=np.zeros((3, len(W513)), dtype=np.uint8))
    ts.close()
    N, m = 12, 4
    pixels, phi, _, W = _small(N, m)
    ts = _dataless(N, m, W)
    good = ts.site_response(phi=phi)
    bad = _which(70, 1)
    bad[41] = 10
    with pytest.raises(TnmlError, match="image 41"):
        ts.site_response(phi=phi, which=bad)
    bad[41] = -1
    with pytest.raises(TnmlError, match="image 41"):
        ts.site_response(pixels=pixels, which=bad)
    assert np.array_equal(ts.site_response(phi=phi), good)
    ts.set_option("predict_dtype", 1)
    with pytest.raises(TnmlError, match="predict_dtype"):
        ts.site_response(phi=phi)
    ts.set_option("predict_dtype", 0)
    assert np.array_equal(ts.site_response(phi=phi), good)
    ts.close()


def _train_ctx():
    from tnml_amd.fixedl import TrainStates
    pixels, labels, phi, W = make_problem(12, 60, 4, 3, pixel_boost=200.0)
    ts = TrainStates(labels, 12, 4, phi=phi)
    ts.set_mps(W)
    ts.init()
    return ts, W


def _same_report(a, b):
    for key in a:
        if key == "cg":
            assert a["cg"] == b["cg"]
        else:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


def test_response_leaves_a_training_context_alone():
    from tnml_amd.fixedl import TnmlError
    sweep = (4, 2, 1e-10, 3, 1e-3, 1e-10)
    others = make_problem(12, 33, 4, 11, pixel_boost=200.0)
    reports, resps = [], []
    for call in (False, True):
        ts, W = _train_ctx()
        ts.bond_update_begin(1, 1, *sweep)
        if call:
            with pytest.raises(TnmlError, match="bond update is in flight"):
                ts.site_response(phi=others[2])
        first = ts.bond_update_end()
        if call:                                                # on a context that holds data and environments, between two bond updates
            resps.append(ts.site_response(phi=others[2]))
            resps.append(ts.site_response(phi=others[2]))
            Wnow = ts.get_mps()
        reports.append((first, ts.bond_update(2, 1, *sweep)))
        ts.close()
    _same_report(reports[0][0], reports[1][0])
    _same_report(reports[0][1], reports[1][1])
    assert np.array_equal(resps[0], resps[1])
    err = _site_err(resps[0], response(Wnow, others[2])[0])
    print("per-site error on the trained W", err.max())
    assert err.max() < TOL


def _table(out):
    """the result table of fullTest as the evaluators print it"""
    lines = [l for l in out.splitlines() if re.search(r"\d+/\d+ correct", l) or l.startswith("Total # test images")]
    assert len(lines) >= 3, out[-1500:]
    return lines


def _run(exe, inp, cwd):
    run = subprocess.run([os.path.join(ROOT, "tnml_amd", exe), str(inp)], capture_output=True, text=True, cwd=cwd, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    return run.stdout


def test_fulltest_driver_writes_the_responses(tmp_path):
    """`fulltest` with predict = yes and response = r.npy on a tiny W: the file is the array site_response gives on the same images for
    their predicted label, the table is that of a run without the key"""
    from tnml_amd import hostlib, synth
    N, per_label, nresp = 16, 20, 30
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
    maxm = max(max(A.shape[0], A.shape[2]) for A in Wf)
    outs = {}
    for key in ("", "response = r.npy\nresponse_n = %d\n" % nresp):
        tin = tmp_path / ("input_%d" % len(outs))
        tin.write_text("input\n{\ndatadir = %s\nfname = W\nfeature = series\nprecision = f64\npredict = yes\npredict_chunk = 48\n%s}\n" % (data, key))
        outs[bool(key)] = _run("fulltest", tin, tmp_path)
    assert _table(outs[True]) == _table(outs[False])
    assert "Device path: site responses (tnml_response_u8), 1024 images per chunk" in outs[True]
    assert "site responses" not in outs[False]
    got = np.load(str(tmp_path / "r.npy"))
    assert got.dtype == np.float64 and got.shape == (nresp, N, 2)
    ts = _dataless(N, maxm, Wf)
    want = ts.site_response(pixels=tp[:nresp])
    ts.close()
    assert np.abs(want).max() > 0 and np.array_equal(got, want)
