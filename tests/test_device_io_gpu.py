"""Device-resident arguments (the tnml_*_dev calls of include/tnml.h and the torch-tensor paths of TrainStates on top of them).

The yardstick throughout is the host-pointer call on the same values, compared bit for bit (np.array_equal / torch.equal): those
calls are held to their models by the suites of their own, so no tolerance enters here.  Contexts are data-less; the shapes are the
smallest at which the new code can go wrong: bonds that cross a 16-row tile, chunks of 64 with a ragged tail, arguments that are
views into the middle of an allocation.

One reading of the wording, written down here because test_refusals asserts it: a value refusal (a label of 10, a NaN coefficient, a
which of -1) is found BY the one k_check_batch launch, so for those cases "nothing is launched" means that io_check gained exactly its
one launch and no other class gained any; for the pointer refusals no class gains a launch, io_check included."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import inputgrad_model as im
import sitegrad_model as sm

pytestmark = pytest.mark.gpu

EDGE_DIMS = [1, 2, 15, 16, 17, 15, 2, 1]
SMALL_DIMS = [1, 2, 3, 5, 3, 2, 1]
DIMS = {"odd0": sm.DIMS[0], "edge": EDGE_DIMS, "small": SMALL_DIMS}     # odd0: bonds of 17 and 33 (and 65, 120)
NS = [1, 17, 70, 130]
_CASES = {}


def _case(name, n):
    if (name, n) not in _CASES:
        dims = DIMS[name]
        d = sm._images(len(dims) - 1, n, 5)
        d["W"] = sm.mps_with_dims(dims, 11)
        d["which"] = (np.arange(n) % 10).astype(np.int32)
        d["phi32"] = d["phi"].astype(np.float32)
        _CASES[(name, n)] = d
    return _CASES[(name, n)]


def _dataless(W, single_label=None, chunk=64):
    from tnml_amd.fixedl import TrainStates
    maxm = max(max(A.shape[0], A.shape[2]) for A in W)
    ts = TrainStates(np.zeros(1, dtype=np.int32), len(W), maxm, no_data=True, single_label=single_label)
    ts.set_mps(W)
    if chunk:
        for opt in ("predict_chunk", "response_chunk", "gradient_chunk"):
            ts.set_option(opt, chunk)
        ts._gchunk = chunk
    return ts


def _dev(a, view=False):
    """a numpy array as a device tensor; view: a slice big[3:] of a larger tensor, so that the pointer is no allocation start"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not view:
        return t.cuda()
    big = torch.empty((t.shape[0] + 3,) + tuple(t.shape[1:]), dtype=t.dtype, device="cuda")
    big[3:] = t.cuda()
    return big[3:]


def _np(t):
    return t.cpu().numpy()


def _same_list(dev_list, host_list):
    return len(dev_list) == len(host_list) and all(np.array_equal(_np(a), b) for a, b in zip(dev_list, host_list))


def _src(case, form, rows=slice(None)):
    """(host keywords, device keywords factory) of an input form: pixels, phi, phi32 (host yardstick: phi32 widened to fp64)"""
    if form == "pixels":
        return dict(pixels=case["pixels"][rows]), lambda view=False: dict(pixels=_dev(case["pixels"][rows], view))
    if form == "phi":
        return dict(phi=case["phi"][rows]), lambda view=False: dict(phi=_dev(case["phi"][rows], view))
    return dict(phi=case["phi32"][rows].astype(np.float64)), lambda view=False: dict(phi=_dev(case["phi32"][rows], view))


def _compare_all(ts, case, form, view=False, nl=10):
    """predict, evaluate, site_response with and without which, backward in its three output combinations under labels and coef:
    every output of the device call equals the host call's"""
    host, devf = _src(case, form)
    labels, coef, which = case["labels"], np.ascontiguousarray(case["coef"][:, :nl]), case["which"] % nl
    w, p = ts.predict(**host)
    wd, pd = ts.predict(**devf(view))
    assert wd.is_cuda and wd.dtype == torch.float64 and pd.dtype == torch.int32
    assert np.array_equal(_np(wd), w) and np.array_equal(_np(pd), p)
    rep, (w2, p2) = ts.evaluate(labels, want_weights=True, **host)
    repd, (w2d, p2d) = ts.evaluate(_dev(labels, view), want_weights=True, **devf(view))
    for f in rep.FIELDS:
        assert np.array_equal(getattr(rep, f), getattr(repd, f)), f
    assert np.array_equal(_np(w2d), w2) and np.array_equal(_np(p2d), p2)
    assert ts.evaluate(_dev(labels, view), **devf(view)) == rep                        # without weights and pred
    for wh in (None, which):
        r, (w3, p3) = ts.site_response(which=wh, want_weights=True, **host)
        rd, (w3d, p3d) = ts.site_response(which=None if wh is None else _dev(wh, view), want_weights=True, **devf(view))
        assert np.array_equal(_np(rd), r) and np.array_equal(_np(w3d), w3) and np.array_equal(_np(p3d), p3)
    for mode in ("labels", "coef"):
        hk = dict(labels=labels) if mode == "labels" else dict(coef=coef)
        for sites, inputs in ((True, False), (False, True), (True, True)):
            dk = dict(labels=_dev(labels, view)) if mode == "labels" else dict(coef=_dev(coef, view))
            g, d, (w4, p4) = ts.backward(want_sites=sites, want_inputs=inputs, want_weights=True, **hk, **host)
            gd, dd, (w4d, p4d) = ts.backward(want_sites=sites, want_inputs=inputs, want_weights=True, **dk, **devf(view))
            assert np.array_equal(_np(w4d), w4) and np.array_equal(_np(p4d), p4)
            if sites:
                assert _same_list(gd, g), (mode, sites, inputs)
                assert all(x.shape == y.shape for x, y in zip(gd, g))
            else:
                assert gd is None
            if inputs and form == "phi32":
                assert dd.dtype == torch.float32 and np.array_equal(_np(dd), d.astype(np.float32))      # rounded once
            elif inputs:
                assert dd.dtype == torch.float64 and np.array_equal(_np(dd), d)
            else:
                assert dd is None
        gs = ts.site_gradient(**hk, **host)
        gsd = ts.site_gradient(**(dict(labels=_dev(labels, view)) if mode == "labels" else dict(coef=_dev(coef, view))), **devf(view))
        assert _same_list(gsd, gs)
        # tnml_site_gradient_coef keeps working and reads what the host call leaves
        host_coef = (ts.site_gradient(**hk, **host), ts.gradient_coef())[1]
        dev_coef = (ts.site_gradient(**(dict(labels=_dev(labels)) if mode == "labels" else dict(coef=_dev(coef))), **devf()), ts.gradient_coef())[1]
        assert np.array_equal(dev_coef, host_coef)


@pytest.mark.parametrize("form", ["pixels", "phi", "phi32"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", sorted(DIMS))
def test_chunk_offsets(name, n, form):
    """chunks of 64: one chunk, one image, two chunks with a ragged tail, three chunks; bonds of 15 / 16 / 17 / 33 and a small class"""
    case = _case(name, n)
    ts = _dataless(case["W"])
    _compare_all(ts, case, form)
    ts.close()


@pytest.mark.parametrize("form", ["pixels", "phi", "phi32"])
def test_pointers_that_are_not_allocation_starts(form):
    """every argument a view big[3:] of a larger device tensor"""
    case = _case("edge", 70)
    ts = _dataless(case["W"])
    _compare_all(ts, case, form, view=True)
    ts.close()


def test_n_zero():
    case = _case("small", 17)
    ts = _dataless(case["W"])
    z = slice(0, 0)
    w, p = ts.predict(phi=_dev(case["phi"][z]))
    assert tuple(w.shape) == (0, 10) and tuple(p.shape) == (0,)
    g, d = ts.backward(labels=_dev(case["labels"][z]), phi=_dev(case["phi"][z]))
    assert tuple(d.shape) == (0, len(case["W"]), 2) and not any(bool(x.any()) for x in g)
    assert ts.evaluate(_dev(case["labels"][z]), phi=_dev(case["phi"][z])).n == 0
    ts.close()


def test_wrong_dtype_and_non_contiguous_tensors_are_put_right_on_the_device():
    """int64 labels, float32 coefficients, int16 pixels, a phi that is a transposed view: cast or made contiguous on the device"""
    case = _case("small", 70)
    ts = _dataless(case["W"])
    phi_t = _dev(np.ascontiguousarray(case["phi"].transpose(1, 0, 2))).transpose(0, 1)
    assert not phi_t.is_contiguous()
    coef32 = case["coef"].astype(np.float32)
    g, d = ts.backward(coef=coef32.astype(np.float64), phi=case["phi"])
    gd, dd = ts.backward(coef=_dev(coef32), phi=phi_t)
    assert _same_list(gd, g) and np.array_equal(_np(dd), d)
    rep = ts.evaluate(case["labels"], pixels=case["pixels"])
    assert ts.evaluate(_dev(case["labels"].astype(np.int64)), pixels=_dev(case["pixels"].astype(np.int16))) == rep
    ts.close()


def test_variant_input_map():
    """raw bytes [n][784] through the device input map onto 196 sites, small bonds"""
    from tnml_amd import synth
    from tnml_amd.input_map import InputMap
    m = InputMap.from_imglen(28, 14, "normal")
    rng = np.random.default_rng(8)
    n = 70
    raw = rng.integers(0, 256, size=(n, m.S)).astype(np.uint8)
    labels = rng.integers(0, 10, size=n).astype(np.int32)
    W = synth.random_mps(m.N, 4, seed=4)
    ts = _dataless(W)
    ts.set_input_map(m)
    w, p = ts.predict(pixels=raw)
    wd, pd = ts.predict(pixels=_dev(raw, True))
    assert np.array_equal(_np(wd), w) and np.array_equal(_np(pd), p)
    assert ts.evaluate(_dev(labels), pixels=_dev(raw)) == ts.evaluate(labels, pixels=raw)
    assert np.array_equal(_np(ts.site_response(pixels=_dev(raw))), ts.site_response(pixels=raw))
    g, d = ts.backward(labels=labels, pixels=raw)
    gd, dd = ts.backward(labels=_dev(labels), pixels=_dev(raw))
    assert _same_list(gd, g) and np.array_equal(_np(dd), d) and np.abs(d).max() > 0
    ts.close()


def test_variant_per_label():
    """TNML_MODE_SINGLE: nl = 1, coef[n, 1]"""
    base = _case("small", 70)
    W = [A if A.ndim == 3 else A[..., 0] * 3.0 for A in base["W"]]
    ts = _dataless(W, single_label=3)
    _compare_all(ts, dict(base, W=W), "phi", nl=1)
    ts.close()


def test_variant_softmax_loss():
    case = _case("small", 70)
    ts = _dataless(case["W"])
    ts.set_loss("softmax", 0.7)
    labels, phi = case["labels"], case["phi"]
    g, d = ts.backward(labels=labels, phi=phi)
    gd, dd = ts.backward(labels=_dev(labels), phi=_dev(phi))
    assert _same_list(gd, g) and np.array_equal(_np(dd), d)
    assert ts.evaluate(_dev(labels), phi=_dev(phi)) == ts.evaluate(labels, phi=phi)
    ts.set_loss("quadratic")
    assert not np.array_equal(_np(ts.backward(labels=_dev(labels), phi=_dev(phi), want_sites=False)[1]), d)
    ts.close()


@pytest.mark.parametrize("form", ["pixels", "phi", "phi32"])
def test_variant_predict_dtype_f32(form):
    case = _case("edge", 70)
    ts = _dataless(case["W"])
    host, devf = _src(case, form)
    w, p = ts.predict(dtype="f32", **host)
    wd, pd = ts.predict(dtype="f32", **devf(True))
    assert np.array_equal(_np(wd), w) and np.array_equal(_np(pd), p)
    rep, (w2, p2) = ts.evaluate(case["labels"], want_weights=True, **host)
    repd, (w2d, p2d) = ts.evaluate(_dev(case["labels"]), want_weights=True, **devf())
    assert rep == repd and np.array_equal(_np(w2d), w2) and np.array_equal(_np(p2d), p2)
    w64, _ = ts.predict(dtype="f64", **host)
    assert not np.array_equal(w64, w)
    ts.close()


@pytest.mark.parametrize("method,kw", [("sgd", dict(lr=1e-3, momentum=0.9)), ("adam", dict(lr=1e-3))])
@pytest.mark.parametrize("mode", ["labels", "coef"])
def test_steps(method, kw, mode):
    """two contexts from one W: three steps with host arguments against three with device arguments"""
    case = _case("edge", 130)
    a, b = _dataless(case["W"]), _dataless(case["W"])
    for k in range(3):
        rows = slice(20 * k, 20 * k + 90)
        hk = dict(labels=case["labels"][rows]) if mode == "labels" else dict(coef=np.ascontiguousarray(case["coef"][rows]) * 1e-3)
        dk = {key: _dev(v, True) for key, v in hk.items()}
        ra = a.gradient_step(pixels=case["pixels"][rows], method=method, scale=1. / 90, **hk, **kw)
        rb = b.gradient_step(pixels=_dev(case["pixels"][rows], True), method=method, scale=1. / 90, **dk, **kw)
        assert (ra.t, ra.grad_norm, ra.factor, ra.clipped) == (rb.t, rb.grad_norm, rb.factor, rb.clipped) and ra.eval == rb.eval
        assert ra.t == k + 1 and ra.grad_norm > 0
    assert all(np.array_equal(x, y) for x, y in zip(a.get_mps(), b.get_mps()))
    assert not np.array_equal(a.get_mps()[3], case["W"][3])
    for which in (("m", "v") if method == "adam" else ("v",)):
        assert all(np.array_equal(x, y) for x, y in zip(a.step_state(which), b.step_state(which)))
    a.close(); b.close()


def test_sites_round_trip():
    case = _case("edge", 17)
    W = case["W"]
    ts = _dataless(W)
    for j in range(1, len(W) + 1):
        A = ts.get_site(j, device=True)
        assert A.is_cuda and tuple(A.shape) == W[j - 1].shape and A.stride() == ts._fstrides(A.shape)
        assert np.array_equal(_np(A), ts.get_site(j))
        B = (A * 1.5 + 0.25)
        assert B.stride() == A.stride()
        ts.set_site(j, B)                                                              # the library's layout: the pointer goes down as it is
        assert np.array_equal(ts.get_site(j), _np(B))
        Cc = torch.from_numpy(np.ascontiguousarray(W[j - 1])).cuda()                    # last-index-fastest: brought into the layout on the device
        ts.set_site(j, Cc)
        assert np.array_equal(ts.get_site(j), W[j - 1])
    assert all(np.array_equal(_np(x), y) for x, y in zip(ts.get_mps(device=True), W))
    from tnml_amd.fixedl import TnmlError
    with pytest.raises(TnmlError, match="Label Index not on site"):
        ts.set_site(1, ts.get_site(len(W) // 2, device=True)[:1, :, :2].contiguous())
    ts.close()


def test_stream():
    """the inputs are written by work queued on a non-default stream directly behind a large matmul; the call is made under that stream"""
    case = _case("edge", 70)
    ts = _dataless(case["W"])
    g, d, (w, p) = ts.backward(labels=case["labels"], phi=case["phi"], want_weights=True)
    src, lab = _dev(case["phi"]), _dev(case["labels"])
    s = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device="cuda")
    phi = torch.zeros_like(src)
    labels = torch.zeros_like(lab)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            big = big @ big * 1e-3
        phi.copy_(src * 1.0)
        labels.copy_(lab + 0)
        gd, dd, (wd, pd) = ts.backward(labels=labels, phi=phi, want_weights=True)
    assert _same_list(gd, g) and np.array_equal(_np(dd), d) and np.array_equal(_np(wd), w) and np.array_equal(_np(pd), p)
    ts.close()


# ---- refusals, through the raw entry points ----
def _hip_runtime():
    """the HIP runtime this process has already mapped (torch's), by its path in /proc/self/maps"""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("no HIP runtime is mapped")


def _raw_backward(ts, n, phi=0, labels=0, coef=0, grad=0, dphi=0, dphi32=0, weights=0):
    from tnml_amd import lib as _lib
    b = _lib.DevBatch(n=n, phi=phi or None, labels=labels or None, coef=coef or None, stream=torch.cuda.current_stream().cuda_stream)
    o = _lib.DevOut(grad=grad or None, dphi=dphi or None, dphi32=dphi32 or None, weights=weights or None)
    rc = ts._L.tnml_backward_dev(ts._h, C.byref(b), C.byref(o))
    return rc, ts._L.tnml_last_error(ts._h).decode()


def _launches(ts):
    return {k: v[0] for k, v in ts.profile_read().items()}


def test_refusals():
    from tnml_amd import lib as _lib
    case = _case("small", 17)
    W, n, N = case["W"], 17, len(case["W"])
    ts = _dataless(W)
    phi, labels, coef = _dev(case["phi"]), _dev(case["labels"]), _dev(case["coef"])
    good_g, good_d = ts.backward(labels=labels, phi=phi)                               # (the workspace and the check block exist from here on)
    dphi = torch.full((n, N, 2), 7.0, dtype=torch.float64, device="cuda")
    dphi32 = torch.full((n, N, 2), 7.0, dtype=torch.float32, device="cuda")
    elems = sum(A.size for A in W)
    grad = torch.full((elems,), 7.0, dtype=torch.float64, device="cuda")
    host_phi = np.ascontiguousarray(case["phi"])
    # memory from hipMalloc through the runtime that is already mapped: the range the runtime reports for it, and more than that
    hip = _hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    raw = C.c_void_p()
    assert hip.hipMalloc(C.byref(raw), 256) == 0
    base, size = C.c_void_p(), C.c_size_t()
    assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), raw) == 0 and base.value == raw.value and size.value >= 256
    n_long = size.value // (N * 16) + 1                                                # images whose features no longer fit what the runtime reports
    bad_label = labels.clone(); bad_label[11] = 10; bad_label[13] = -1
    bad_coef = coef.clone(); bad_coef[5, 3] = float("nan"); bad_coef[9, 0] = float("inf")
    bad_which = torch.zeros(n, dtype=torch.int32, device="cuda"); bad_which[4] = -1
    torch.cuda.synchronize()
    P = lambda t: t.data_ptr()
    pointer_cases = [
        ("a NumPy array's address as phi", dict(phi=host_phi.ctypes.data, labels=P(labels), dphi=P(dphi)), "phi.*not device memory"),
        ("a device double array offset by 4 bytes", dict(phi=P(phi) + 4, labels=P(labels), dphi=P(dphi)), "phi.*not aligned to 8"),
        ("an allocation that is too short", dict(n=n_long, phi=raw.value, labels=P(labels), dphi=P(dphi)), "phi.*needs %d bytes, its allocation ends %d bytes" % (n_long * N * 16, size.value)),
        ("an output overlapping an input", dict(phi=P(phi), labels=P(labels), dphi=P(phi) + 16 * N), "dphi overlaps phi"),
        ("two outputs overlapping", dict(phi=P(phi), labels=P(labels), dphi=P(dphi), weights=P(dphi)), "weights overlaps dphi|dphi overlaps weights"),
        ("both dphi and dphi32", dict(phi=P(phi), labels=P(labels), dphi=P(dphi), dphi32=P(dphi32)), "dphi and dphi32"),
    ]
    value_cases = [
        ("a label of 10", dict(phi=P(phi), labels=P(bad_label), dphi=P(dphi), grad=P(grad)), "tnml_backward_dev: label 10 of image 11 out of range"),
        ("a NaN coefficient", dict(phi=P(phi), coef=P(bad_coef), dphi=P(dphi), grad=P(grad)), "tnml_backward_dev: coefficient 3 of image 5 is not finite"),
    ]
    ts.profile(True)
    for cases, may_check in ((pointer_cases, 0), (value_cases, 1)):
        for what, kw, msg in cases:
            ts.profile_reset()
            bytes_before = ts.device_bytes()
            rc, err = _raw_backward(ts, kw.pop("n", n), **kw)
            assert rc != 0 and re.search(msg, err), (what, err)
            after = _launches(ts)
            assert after.pop("io_check") == may_check, (what, after)
            assert not any(after.values()), (what, after)
            assert ts.device_bytes() == bytes_before, what
            torch.cuda.synchronize()
            assert bool((dphi == 7.0).all()) and bool((dphi32 == 7.0).all()) and bool((grad == 7.0).all()), what
            g, d = ts.backward(labels=labels, phi=phi)                                 # the context serves a correct call right afterwards
            assert all(torch.equal(x, y) for x, y in zip(g, good_g)) and torch.equal(d, good_d), what
    # a which of -1: tnml_response_dev
    ts.profile_reset()
    resp = torch.full((n, N, 2), 7.0, dtype=torch.float64, device="cuda")
    good_r = ts.site_response(phi=phi)
    ts.profile_reset()
    bytes_before = ts.device_bytes()
    b = _lib.DevBatch(n=n, phi=P(phi), which=P(bad_which), stream=torch.cuda.current_stream().cuda_stream)
    o = _lib.DevOut(resp=P(resp))
    assert ts._L.tnml_response_dev(ts._h, C.byref(b), C.byref(o)) != 0
    assert "tnml_response_dev: which = -1 of image 4 out of range 0..9" in ts._L.tnml_last_error(ts._h).decode()
    after = _launches(ts)
    assert after.pop("io_check") == 1 and not any(after.values()), after
    assert ts.device_bytes() == bytes_before
    torch.cuda.synchronize()
    assert bool((resp == 7.0).all())
    assert torch.equal(ts.site_response(phi=phi), good_r)
    ts.profile(False)
    # the same words as the host path
    from tnml_amd.fixedl import TnmlError
    with pytest.raises(TnmlError, match="label 10 of image 11 out of range"):
        ts.backward(labels=_np(bad_label), phi=case["phi"])
    assert hip.hipFree(raw) == 0
    ts.close()


def test_a_first_call_that_is_refused_allocates_nothing():
    case = _case("small", 17)
    ts = _dataless(case["W"])
    before = ts.device_bytes()
    rc, err = _raw_backward(ts, 17, phi=np.ascontiguousarray(case["phi"]).ctypes.data, labels=_dev(case["labels"]).data_ptr(),
                            dphi=torch.zeros((17, len(case["W"]), 2), dtype=torch.float64, device="cuda").data_ptr())
    assert rc != 0 and "phi" in err and "not device memory" in err
    assert ts.device_bytes() == before
    ts.close()


def test_launch_counts():
    """class by class the launches of a device call are the host call's plus exactly one io_check, whether or not the call carries
    labels, coef or which"""
    case = _case("edge", 130)                                                          # three chunks
    ts = _dataless(case["W"])
    labels, phi, coef, which = case["labels"], case["phi"], case["coef"], case["which"]

    def count(fn):
        ts.profile(True); ts.profile_reset()
        fn()
        out = _launches(ts)
        ts.profile(False)
        return out

    pairs = [
        (lambda: ts.predict(phi=phi), lambda: ts.predict(phi=_dev(phi)), 1),
        (lambda: ts.evaluate(labels, pixels=case["pixels"]), lambda: ts.evaluate(_dev(labels), pixels=_dev(case["pixels"])), 1),
        (lambda: ts.site_response(phi=phi, which=which), lambda: ts.site_response(phi=_dev(phi), which=_dev(which)), 1),
        (lambda: ts.site_response(phi=phi), lambda: ts.site_response(phi=_dev(phi)), 1),
        (lambda: ts.backward(labels=labels, phi=phi), lambda: ts.backward(labels=_dev(labels), phi=_dev(phi)), 1),
        (lambda: ts.backward(coef=coef, phi=phi, want_sites=False), lambda: ts.backward(coef=_dev(coef), phi=_dev(case["phi32"]), want_sites=False), 1),
        (lambda: ts.gradient_step(labels=labels, phi=phi, lr=1e-4), lambda: ts.gradient_step(labels=_dev(labels), phi=_dev(phi), lr=1e-4), 1),
    ]
    for host_fn, dev_fn, checks in pairs:
        h, d = count(host_fn), count(dev_fn)
        assert h.pop("io_check") == 0 and d.pop("io_check") == checks
        assert h == d and sum(h.values()) > 0, (h, d)
    ts.close()


def test_bookkeeping():
    """host-pointer calls allocate what they did; a device call leaves out the buffer the images are copied into and the transposed
    result, adds the 24-byte check block once, and a later host-pointer call of the form adds what was left out"""
    case = _case("small", 70)
    W, N = case["W"], len(case["W"])
    C_ = 64
    ts = _dataless(W)
    before = ts.device_bytes()
    ts.backward(labels=_dev(case["labels"]), phi=_dev(case["phi"]))
    dev_bytes = ts.device_bytes() - before
    ts.backward(labels=_dev(case["labels"]), phi=_dev(case["phi"]))
    assert ts.device_bytes() - before == dev_bytes
    ts.backward(labels=case["labels"], phi=case["phi"])
    host_after_dev = ts.device_bytes() - before
    assert host_after_dev - dev_bytes == 16 * N * C_ + 16 * N * C_                     # rawphi and the transposed dphi
    ts2 = _dataless(W)
    before2 = ts2.device_bytes()
    ts2.backward(labels=case["labels"], phi=case["phi"])
    assert host_after_dev == ts2.device_bytes() - before2 + 24
    # the block and the event go with the last workspace and come back with the next device call
    ts.set_input_map(None)
    assert ts.device_bytes() == before
    ts.backward(labels=_dev(case["labels"]), phi=_dev(case["phi"]))
    assert ts.device_bytes() - before == dev_bytes
    ts.set_option("gradient_chunk", 128)
    g = ts.backward(labels=_dev(case["labels"]), phi=_dev(case["phi"]))[0]
    assert _same_list(g, ts.backward(labels=case["labels"], phi=case["phi"])[0])              # (the release fell inside that call)
    ts.close(); ts2.close()


def test_euler_tie_on_device_tensors():
    """sum_s phi[n, j, s] dphi[n, j, s] = sum_l c_nl W_l(x_n) at every site (tests/inputgrad_model.py), on the device tensors"""
    case = sm.odd_case(0, 70)
    W, phi = case["W"], case["phi"]
    ts = _dataless(W, chunk=0)
    ts.set_option("predict_tile", 64)
    _, dphi, (w, _) = ts.backward(phi=_dev(phi), coef=_dev(case["coef"]), want_sites=False, want_weights=True)
    _, _, bnd = im.model_of(case, "phi", "coef")
    _, w_abs, c_abs = im.abs_input_gradient(W, phi, coef=case["coef"])
    K = im.rounding_count(len(W), 120, 10)
    U = 2.0 ** -53
    allowed = (np.abs(phi) * bnd).sum(axis=2) + K * U * (c_abs * w_abs).sum(axis=1)[:, None]
    assert dphi.is_cuda and w.is_cuda
    got, want = (phi * _np(dphi)).sum(axis=2), (case["coef"] * _np(w)).sum(axis=1)[:, None]
    assert (np.abs(got - want) <= allowed).all()
    assert (allowed < 1e-6 * (c_abs * w_abs).sum(axis=1)[:, None]).all()
    ts.close()
