"""Streamed input gradients (tnml_backward_u8 / tnml_backward_phi, kernels_inputgrad.hip): dphi[n, j, s] = sum_l c_nl dW_l(x_n)/dphi[n, j, s]
for every site of every image, and the torch layer on top of it (tnml_amd/torch_layer.py).  The yardstick is tests/inputgrad_model.py
with its own elementwise bound (proved by tests/test_inputgrad_model_host.py); contexts are data-less.

The dispatch picks the 16-wide tile for the few images of a test (fewer tiles than compute units), so the cases that are about a bond
class run under predict_tile = 64, which gives the widest tile of the class: 64 up to bond 128, 32 up to 256, 16 above."""
import ctypes as C

import numpy as np
import pytest

import inputgrad_model as im
import long_chain_cases as lc
import response_model as rm
import sitegrad_model as sm
from conftest import make_problem

pytestmark = pytest.mark.gpu
U = 2.0 ** -53

# the 16-row tile edges, and at N = 5 the bonds on either side of the tile-width thresholds (the Label site is site 2)
EDGE_DIMS = [1, 2, 15, 16, 17, 15, 2, 1]
THRESHOLD_DIMS = {128: [1, 2, 128, 16, 2, 1], 129: [1, 2, 129, 16, 2, 1], 256: [1, 2, 256, 16, 2, 1], 257: [1, 2, 257, 16, 2, 1], 512: [1, 2, 512, 16, 2, 1]}
_CASES = {}


def _dims_case(dims, n):
    key = (tuple(dims), n)
    if key not in _CASES:
        d = sm._images(len(dims) - 1, n, 5)
        d["W"] = sm.mps_with_dims(dims, 11)
        _CASES[key] = d
    return _CASES[key]


def _dataless(W, single_label=None, tile=0):
    """a context that holds no images: sized by W alone"""
    from tnml_amd.fixedl import TrainStates
    maxm = max(max(A.shape[0], A.shape[2]) for A in W)
    ts = TrainStates(np.zeros(1, dtype=np.int32), len(W), maxm, no_data=True, single_label=single_label)
    ts.set_mps(W)
    if tile:
        ts.set_option("predict_tile", tile)
    return ts


def _plain(W):
    """the per-label variant's W: no Label index"""
    return [A if A.ndim == 3 else A[..., 0] * 3.0 for A in W]


def _src(case, form, rows=slice(None)):
    return dict(phi=case["phi"][rows]) if form == "phi" else dict(pixels=case["pixels"][rows])


def _coefs(case, mode, target=None, rows=slice(None)):
    return dict(labels=case["labels"][rows]) if mode == "labels" else dict(coef=case["coef"][rows, :1 if target is not None else 10])


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_against_model(ts, case, form, mode, target=None):
    """the device's dphi within the model's bound; weights and pred those of predict(), bit for bit"""
    d_m, _, bnd = im.model_of(case, form, mode, target)
    _, dphi, (w, pred) = ts.backward(want_sites=False, want_weights=True, **_coefs(case, mode, target), **_src(case, form))
    assert dphi.shape == d_m.shape
    ratio = im.worst_ratio(dphi, d_m, bnd)
    print("worst error / bound", ratio, "largest |dphi|", np.abs(d_m).max())
    assert ratio <= 1.
    assert np.abs(dphi).max() > 0
    wp, pp = ts.predict(**_src(case, form))
    assert np.array_equal(w, wp) and np.array_equal(pred, pp)
    return dphi, w


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("n", [1, 17, 70])
@pytest.mark.parametrize("k", range(len(sm.DIMS)))
def test_dphi_matches_the_model_on_every_bond_class(k, n, form, mode):
    """bonds of 1, 2, 3, 5, 9, 17, 33, 65, 120, ml != mr, the three tile widths, the Label site at 512 x 2 x 511 x 10; one image, a
    partial tile, more than one tile"""
    case = sm.odd_case(k, n)
    ts = _dataless(case["W"], tile=64)
    _check_against_model(ts, case, form, mode)
    ts.close()


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("n", [1, 17, 70])
def test_dphi_at_the_row_tile_edges(n, mode):
    """bonds of 15, 16 and 17: a row tile that is not full, one that is, one row into the next"""
    case = _dims_case(EDGE_DIMS, n)
    ts = _dataless(case["W"], tile=64)
    _check_against_model(ts, case, "phi", mode)
    ts.close()


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("bond", sorted(THRESHOLD_DIMS))
def test_dphi_at_the_tile_width_thresholds(bond, mode):
    """N = 5 with one large bond: 128 (the last of the 64-wide tile), 129 and 256 (32-wide), 257 and 512 (16-wide)"""
    case = _dims_case(THRESHOLD_DIMS[bond], 70)
    ts = _dataless(case["W"], tile=64)
    _check_against_model(ts, case, "u8" if bond == 257 else "phi", mode)
    ts.close()


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("N,m", [(4, 2), (4, 3), (5, 3), (12, 5)])
def test_dphi_short_chains(N, m, form, mode):
    """N = 4 is the shortest chain served: one site left of the Label site (site N // 2), which is next to the end"""
    case = sm.small_case(N, m)
    ts = _dataless(case["W"])
    _check_against_model(ts, case, form, mode)
    g0, d0 = ts.backward(phi=case["phi"][:0], labels=case["labels"][:0])             # n = 0 succeeds and zeroes grad
    assert d0.shape == (0, N, 2) and not any(g.any() for g in g0)
    ts.close()


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("N", [4, 6, 12])
def test_dphi_per_label_variant(N, mode):
    """TNML_MODE_SINGLE: nl = 1, site 1 plays the centre, no left chain"""
    base = sm.small_case(N, 5 if N > 4 else 3)
    case = _CASES.setdefault(("plain", N), dict(base, W=_plain(base["W"])))
    ts = _dataless(case["W"], single_label=3)
    _, w = _check_against_model(ts, case, "phi", mode, target=3)
    assert w.shape == (70, 1)
    ts.close()


def test_dphi_under_the_softmax_loss():
    """labels mode under option loss = softmax: the coefficients are k_site_backward's (tests/test_loss_gpu.py holds them to their
    model); dphi is the model's on those coefficients, and grad is site_gradient()'s, bit for bit"""
    case = sm.small_case(12, 5)
    ts = _dataless(case["W"])
    ts.set_loss("softmax", 0.7)
    grads, dphi = ts.backward(labels=case["labels"], phi=case["phi"])
    coef = ts.gradient_coef()
    assert coef.shape == (70, 10) and np.abs(coef.sum(axis=1)).max() < 1e-12          # softmax - y sums to zero
    want, _ = im.input_gradient(case["W"], case["phi"], coef=coef)
    ratio = im.worst_ratio(dphi, want, im.bound(case["W"], case["phi"], coef=coef))
    print("worst error / bound", ratio)
    assert ratio <= 1.
    assert _same(grads, ts.site_gradient(labels=case["labels"], phi=case["phi"]))
    ts.set_loss("quadratic")
    quad = ts.backward(labels=case["labels"], phi=case["phi"], want_sites=False)[1]
    assert not np.array_equal(quad, dphi)
    ts.close()


@pytest.mark.parametrize("side,imglen", [(8, 4)])
def test_dphi_under_an_input_map(side, imglen):
    """raw bytes through the device input map: dphi is with respect to the features of the N reduced sites, the bits of the feature
    path on the features the map defines"""
    from tnml_amd import synth
    from tnml_amd.input_map import InputMap
    m = InputMap.from_imglen(side, imglen, "normal")
    rng = np.random.default_rng(8)
    raw = rng.integers(0, 256, size=(20, m.S)).astype(np.uint8)
    labels = rng.integers(0, 10, size=20).astype(np.int32)
    W = synth.random_mps(m.N, 6, seed=4)
    ts = _dataless(W)
    g_ref, d_ref = ts.backward(labels=labels, phi=m.features(raw))
    ts.set_input_map(m)
    g, d = ts.backward(labels=labels, pixels=raw)
    assert d.shape == (20, m.N, 2) and np.abs(d).max() > 0
    assert np.array_equal(d, d_ref) and _same(g, g_ref)
    want, _ = im.input_gradient(W, m.features(raw), labels=labels)
    ratio = im.worst_ratio(d, want, im.bound(W, m.features(raw), labels=labels))
    print("worst error / bound", ratio)
    assert ratio <= 1.
    ts.close()


@pytest.mark.parametrize("k,mode", [(0, "labels"), (1, "coef")])
def test_an_images_bits_do_not_depend_on_tile_chunk_or_position(k, mode):
    """130 images: the tile widths 16 / 32 / 64, chunks of 64 (two full and a ragged one), the images in reverse order, one image alone
    and a repeat all give the same bits for every image"""
    case = sm.odd_case(k, 130)
    kw = dict(phi=case["phi"], want_sites=False, **_coefs(case, mode))
    ts = _dataless(case["W"])
    full = ts.backward(**kw)[1]
    assert np.array_equal(ts.backward(**kw)[1], full)
    for tile in (16, 32, 64):
        ts.set_option("predict_tile", tile)
        assert np.array_equal(ts.backward(**kw)[1], full), tile
    ts.set_option("gradient_chunk", 64)
    for tile in (64, 0):
        ts.set_option("predict_tile", tile)
        assert np.array_equal(ts.backward(**kw)[1], full), ("chunks of 64", tile)
    rev = slice(None, None, -1)
    assert np.array_equal(ts.backward(phi=case["phi"][rev], want_sites=False, **_coefs(case, mode, rows=rev))[1], full[rev])
    for i in (0, 77, 129):
        one = ts.backward(phi=case["phi"][i:i + 1], want_sites=False, **_coefs(case, mode, rows=slice(i, i + 1)))[1]
        assert np.array_equal(one[0], full[i]), i
    ts.set_option("gradient_chunk", 512)
    small = ts.backward(phi=case["phi"][:20], want_sites=False, **_coefs(case, mode, rows=slice(0, 20)))[1]     # after n = 130 on the same context
    assert np.array_equal(small, full[:20])
    ts.close()


@pytest.mark.parametrize("name,mode", [("C", "coef"), ("C", "labels"), ("E196", "labels")])
def test_dphi_on_long_chains(name, mode):
    """case C of tests/long_chain_cases.py (784 sites, bonds up to 130: the 32-wide tile, a tape of 50 000 rows) and E196 (196 sites, raw
    bytes through the input map), inside the bound"""
    d = lc.case(name)
    p = lc.CASES[name]
    f = lc.feats(name, "map" if "imap" in d else "phi")
    ts = _dataless(d["W"], tile=p["tile"])
    if "imap" in d:
        ts.set_input_map(d["imap"])
        src = dict(pixels=d["raw"])
    else:
        src = dict(phi=d["phi"])
    dphi = ts.backward(want_sites=False, **lc.coefs(name, mode), **src)[1]
    want, _ = im.input_gradient(d["W"], f, **lc.coefs(name, mode))
    bnd = im.bound(d["W"], f, **lc.coefs(name, mode))
    ratio = im.worst_ratio(dphi, want, bnd)
    teeth = float((bnd / np.abs(want)).min())
    print(name, mode, "worst error / bound", ratio, "smallest bound / |dphi|", teeth)
    assert ratio <= 1.
    assert np.isfinite(bnd).all() and teeth < 1e-6                                    # the bound sees something at this length
    ts.close()


def test_dphi_is_the_sum_of_the_site_responses():
    """against merged device code: dphi = sum_l c_nl site_response(which = l), inside the sum of the two models' bounds and the
    roundings of the sum itself (nl products and additions)"""
    case = sm.small_case(12, 5)
    W, phi, coef = case["W"], case["phi"], case["coef"]
    n = len(phi)
    ts = _dataless(W)
    dphi = ts.backward(coef=coef, phi=phi, want_sites=False)[1]
    total, allowed, mag = np.zeros_like(dphi), im.bound(W, phi, coef=coef), np.zeros_like(dphi)
    for l in range(10):
        which = np.full(n, l, dtype=np.int32)
        resp = ts.site_response(phi=phi, which=which)
        total += coef[:, l, None, None] * resp
        mag += np.abs(coef[:, l, None, None] * resp)
        allowed = allowed + np.abs(coef[:, l, None, None]) * rm.bound(W, phi, which)
    allowed = allowed + 2 * 10 * U * mag
    print("worst difference / allowed", float((np.abs(dphi - total) / allowed).max()))
    assert (np.abs(dphi - total) <= allowed).all()
    assert (allowed < 1e-8 * np.abs(dphi).max()).all()
    ts.close()


@pytest.mark.parametrize("mode", ["labels", "coef"])
def test_euler_tie_on_the_devices_own_weights(mode):
    """sum_s phi[n, j, s] dphi[n, j, s] = sum_l c_nl W_l(x_n) at every site, against the call's own weights"""
    case = sm.odd_case(0, 70)
    W, phi = case["W"], case["phi"]
    ts = _dataless(W, tile=64)
    _, dphi, (w, _) = ts.backward(phi=phi, want_sites=False, want_weights=True, **_coefs(case, mode))
    coef = case["coef"] if mode == "coef" else 2. * (w - sm.targets(case["labels"], 10))
    _, _, bnd = im.model_of(case, "phi", mode)
    _, w_abs, c_abs = im.abs_input_gradient(W, phi, **_coefs(case, mode))
    K = im.rounding_count(len(W), 120, 10)
    allowed = (np.abs(phi) * bnd).sum(axis=2) + K * U * (c_abs * w_abs).sum(axis=1)[:, None]
    got, want = (phi * dphi).sum(axis=2), (coef * w).sum(axis=1)[:, None]
    assert (np.abs(got - want) <= allowed).all()
    assert (allowed < 1e-6 * (c_abs * w_abs).sum(axis=1)[:, None]).all()
    ts.close()


def test_grad_weights_and_pred_are_those_of_the_existing_calls_and_the_launches_follow_the_outputs():
    case = sm.small_case(12, 5)
    ts = _dataless(case["W"])
    ts.set_option("gradient_chunk", 16)                                               # 70 images: five chunks
    for form in ("phi", "u8"):
        for mode in ("labels", "coef"):
            kw = dict(_coefs(case, mode), **_src(case, form))
            ref, (w_ref, p_ref) = ts.site_gradient(want_weights=True, **kw)
            grads, dphi, (w, p) = ts.backward(want_weights=True, **kw)
            assert _same(grads, ref) and np.array_equal(w, w_ref) and np.array_equal(p, p_ref)
            wp, pp = ts.predict(**_src(case, form))
            assert np.array_equal(w, wp) and np.array_equal(p, pp)
            g2, d2 = ts.backward(want_inputs=False, **kw)
            assert d2 is None and _same(g2, ref)
            g3, d3 = ts.backward(want_sites=False, **kw)
            assert g3 is None and np.array_equal(d3, dphi)
            assert _same(ts.site_gradient(**kw), ref)                                 # and the gradient call after it is what it was
    kw = dict(labels=case["labels"], phi=case["phi"])
    launches = {}
    for sites, inputs in ((True, True), (False, True), (True, False)):
        ts.profile(True)
        ts.profile_reset()
        ts.backward(want_sites=sites, want_inputs=inputs, **kw)
        prof = ts.profile_read()
        ts.profile(False)
        launches[(sites, inputs)] = (prof["site_bwd"][0], prof["site_grad"][0], prof["input_grad"][0])
        assert prof["site_resp"][0] == 0 and prof["chain"][0] == 0, prof
    assert launches == {(True, True): (5, 5, 5), (False, True): (5, 0, 5), (True, False): (5, 5, 0)}, launches
    with pytest.raises(Exception, match="both NULL"):
        ts.backward(want_sites=False, want_inputs=False, **kw)
    ts.close()


def _ru16(m):
    return (m + 15) // 16 * 16


def _staging(N, C, forms):
    per = {"u8": 2 * N * C, "phi": 32 * N * C}
    return sum(per[f] for f in ([forms] if isinstance(forms, str) else forms))


def _formula_gradient(W, chunk, staging, nl=10):
    """the workspace of tnml_site_gradient_* as include/tnml.h states it"""
    N = len(W)
    C_ = (chunk + 63) // 64 * 64
    B = 32 + sum(_ru16(A.shape[2]) for A in W[:-1])
    E = sum(A.size for A in W)
    return 16 * N + 16 * nl * C_ + 8 * C_ + 4 * (N + 2) + 8 * (N + 1) + 4 * (N + nl) + 8 * E + 16 * B * C_ + _staging(N, C_, staging)


def _formula_dphi(W, chunk):
    """what tnml_backward_* adds from the first call that asks for dphi on, as include/tnml.h states it"""
    return 32 * len(W) * ((chunk + 63) // 64 * 64)


def _formula_response(W, chunk, staging, nl=10):
    N = len(W)
    C_ = (chunk + 63) // 64 * 64
    label_site = next(A for A in W if A.ndim == 4)
    B = 32 + sum(_ru16(A.shape[2]) for A in W[:-1]) + _ru16(label_site.shape[0]) + _ru16(label_site.shape[2])
    return 16 * N + 8 * nl * C_ + 8 * C_ + 4 * (N + 4) + 32 * N * C_ + 8 * B * C_ + _staging(N, C_, staging)


def _formula_predict(W, chunk, staging, nl=10):
    N = len(W)
    C_ = (chunk + 63) // 64 * 64
    M = _ru16(min(max(max(A.shape[0], A.shape[2]) for A in W), 512))
    return 16 * N + 8 * nl * C_ + 4 * C_ + 8 * M * C_ + _staging(N, C_, staging)


def test_backward_bookkeeping():
    """the gradient workspace keeps its formula; the dphi buffers are 32 N C bytes of their own, made by the first call that asks for
    dphi, re-made with gradient_chunk and released with the input map; predict and response keep their bytes"""
    case = sm.small_case(12, 5)
    W = case["W"]
    kw = dict(labels=case["labels"], phi=case["phi"])
    ts = _dataless(W)
    before = ts.device_bytes()
    ts.site_gradient(**kw)
    assert ts.device_bytes() - before == _formula_gradient(W, 512, "phi")
    ts.backward(want_inputs=False, **kw)                                              # grad alone: nothing is added
    assert ts.device_bytes() - before == _formula_gradient(W, 512, "phi")
    ts.backward(**kw)
    assert ts.device_bytes() - before == _formula_gradient(W, 512, "phi") + _formula_dphi(W, 512)
    ts.site_gradient(**kw)
    ts.backward(want_sites=False, **kw)
    assert ts.device_bytes() - before == _formula_gradient(W, 512, "phi") + _formula_dphi(W, 512)
    ts.set_option("gradient_chunk", 100)                                              # re-made: the dphi buffers come back with the next call that asks
    ts.site_gradient(**kw)
    assert ts.device_bytes() - before == _formula_gradient(W, 100, "phi")
    ts.backward(want_sites=False, labels=case["labels"], pixels=case["pixels"])
    assert ts.device_bytes() - before == _formula_gradient(W, 100, ["phi", "u8"]) + _formula_dphi(W, 100)
    ts.set_option("predict_chunk", 1024)
    ts.set_option("response_chunk", 1024)
    ts.predict(phi=case["phi"])
    ts.site_response(phi=case["phi"])
    others = _formula_predict(W, 1024, "phi") + _formula_response(W, 1024, "phi")
    assert ts.device_bytes() - before == _formula_gradient(W, 100, ["phi", "u8"]) + _formula_dphi(W, 100) + others
    ts.backward(**kw)
    assert ts.device_bytes() - before == _formula_gradient(W, 100, ["phi", "u8"]) + _formula_dphi(W, 100) + others
    ts.set_input_map(None)                                                            # releases the gradient and response workspaces whole
    assert ts.device_bytes() - before == _formula_predict(W, 1024, "phi")
    ts.backward(want_sites=False, **kw)
    assert ts.device_bytes() - before == _formula_predict(W, 1024, "phi") + _formula_gradient(W, 100, "phi") + _formula_dphi(W, 100)
    ts.close()


def _call(ts, n, x, labels, coef, grad, dphi):
    from tnml_amd import lib as _lib
    lp = None if labels is None else labels.ctypes.data_as(C.POINTER(C.c_int32))
    cp = None if coef is None else _lib.dptr(coef)
    gp = None if grad is None else _lib.dptr(grad)
    dp = None if dphi is None else _lib.dptr(dphi)
    rc = ts._L.tnml_backward_phi(ts._h, n, _lib.dptr(x), lp, cp, gp, dp, None, None)
    return rc, ts._L.tnml_last_error(ts._h).decode()


def test_backward_refusals_leave_the_context_usable_and_the_outputs_untouched():
    from tnml_amd.fixedl import TnmlError
    W513 = sm.mps_with_dims([1, 2, 16, 513, 16, 2, 1], 11)
    ts = _dataless(W513)
    with pytest.raises(TnmlError, match="tnml_classify"):
        ts.backward(labels=np.zeros(3, dtype=np.int32), pixels=np.zeros((3, len(W513)), dtype=np.uint8))
    ts.close()
    case = sm.small_case(12, 5)
    W, phi, labels, coef = case["W"], np.ascontiguousarray(case["phi"]), case["labels"], np.ascontiguousarray(case["coef"])
    ts = _dataless(W)
    good_g, good_d = ts.backward(labels=labels, phi=phi)
    elems = sum(g.size for g in good_g)

    def refused(match, lab, cf, outputs=(True, True)):
        grad = np.full(elems, 7.5) if outputs[0] else None
        dphi = np.full((70, 12, 2), 7.5) if outputs[1] else None
        rc, msg = _call(ts, 70, phi, lab, cf, grad, dphi)
        assert rc != 0 and match in msg, msg
        assert all((a == 7.5).all() for a in (grad, dphi) if a is not None)           # untouched

    refused("both NULL", labels, None, outputs=(False, False))
    refused("exactly one of labels and coef", labels, coef)
    refused("exactly one of labels and coef", None, None)
    bad = labels.copy()
    bad[41] = 10
    refused("image 41", bad, None)
    bad[41] = -1
    refused("image 41", bad, None, outputs=(False, True))
    for v in (np.nan, np.inf):
        cf = coef.copy()
        cf[57, 3] = v
        refused("image 57 is not finite", None, cf)
    ts.set_option("predict_dtype", 1)
    refused("predict_dtype", labels, None)
    ts.set_option("predict_dtype", 0)
    g, d = ts.backward(labels=labels, phi=phi)
    assert _same(g, good_g) and np.array_equal(d, good_d)
    # n = 0 zeroes grad and touches nothing else
    grad, dphi = np.full(elems, 7.5), np.full((70, 12, 2), 7.5)
    rc, _ = _call(ts, 0, phi, labels, None, grad, dphi)
    assert rc == 0 and not grad.any() and (dphi == 7.5).all()
    ts.close()


# ---- the torch layer ----
def _torch_problem(N=5, m=3, n=3):
    from tnml_amd import synth
    _, labels, phi, _ = make_problem(N, 10, 2, 7, pixel_boost=200.0)
    return synth.random_mps(N, m, seed=10), np.ascontiguousarray(phi[:n]), np.asarray(labels[:n], dtype=np.int64)


def test_gradcheck_of_the_mps_function_for_phi_and_every_site():
    """torch.autograd.gradcheck in fp64 at its default tolerances, N = 5, m = 3, n = 3.  gradcheck perturbs its inputs in place, so
    the function under test uploads every site before it applies MPSFunction"""
    import torch
    from tnml_amd.torch_layer import MPSFunction
    W, phi, _ = _torch_problem()
    ts = _dataless(W)

    def fn(x, *sites):
        for j, A in enumerate(sites, start=1):
            ts.set_site(j, A.detach().numpy())
        return MPSFunction.apply(ts, x, *sites)

    x = torch.tensor(phi, dtype=torch.float64, requires_grad=True)
    sites = [torch.tensor(np.ascontiguousarray(A), dtype=torch.float64, requires_grad=True) for A in W]
    assert torch.autograd.gradcheck(fn, (x, *sites))
    ts.close()


def test_one_sgd_step_of_the_layer_lowers_a_cross_entropy_computed_in_torch():
    import torch
    from tnml_amd.torch_layer import MPSLayer
    W, phi, labels = _torch_problem(N=6, m=4, n=10)
    ts = _dataless(W)
    layer = MPSLayer(ts, train_sites=True)
    assert [tuple(p.shape) for p in layer.sites] == [A.shape for A in W]
    opt = torch.optim.SGD(layer.parameters(), lr=1e-2)
    x, y = torch.tensor(phi), torch.tensor(labels)
    loss = torch.nn.functional.cross_entropy(layer(x), y)
    opt.zero_grad()
    loss.backward()
    assert all(p.grad is not None and p.grad.abs().max() > 0 for p in layer.sites)
    opt.step()
    with torch.no_grad():
        after = torch.nn.functional.cross_entropy(layer(x), y)
    print("cross-entropy", float(loss.detach()), "->", float(after))
    assert float(after) < float(loss.detach())
    for j, p in enumerate(layer.sites, start=1):                                      # the context holds the stepped sites
        assert np.array_equal(ts.get_site(j), p.detach().numpy())
    ts.close()


def test_a_linear_feature_map_in_front_of_the_layer_gets_dphi_chained_by_hand():
    import torch
    from tnml_amd.torch_layer import MPSLayer
    W, _, _ = _torch_problem(N=6, m=4, n=10)
    rng = np.random.default_rng(3)
    xs = rng.random((10, 6))
    go = rng.standard_normal((10, 10))
    ts = _dataless(W)
    layer = MPSLayer(ts)
    feat = torch.nn.Linear(1, 2).double()
    phi = feat(torch.tensor(xs).unsqueeze(-1))                                        # [n, N, 2]
    (layer(phi) * torch.tensor(go)).sum().backward()
    dphi = ts.backward(coef=go, phi=phi.detach().numpy(), want_sites=False)[1]
    want_w, want_b = np.einsum("njs,nj->s", dphi, xs), dphi.sum(axis=(0, 1))
    tol_w = 4 * xs.size * U * np.einsum("njs,nj->s", np.abs(dphi), xs)                # the two sums of 60 terms, in any order
    tol_b = 4 * xs.size * U * np.abs(dphi).sum(axis=(0, 1))
    gw, gb = feat.weight.grad.numpy()[:, 0], feat.bias.grad.numpy()
    assert np.abs(gw).min() > 0 and np.abs(gb).min() > 0
    assert (np.abs(gw - want_w) <= tol_w).all() and (np.abs(gb - want_b) <= tol_b).all()
    assert all(p.grad is None for p in layer.sites)
    ts.close()
