"""Backward from the forward's tape (tnml_forward_taped_* / tnml_backward_taped*, k_forward_taped and k_site_outward of
kernels_sitegrad.hip) and the batched site upload (tnml_set_sites_dev, k_sites_gather).  Every number the new calls return has a
yardstick in the tree already: weights and pred must equal predict()'s, grad and dphi backward(coef=..)'s, W after set_sites() the W of
single set_site() calls -- bit for bit, so no tolerance appears here but the Jacobian test's, which is tests/inputgrad_model.py's bound.
Contexts are data-less; gradient_chunk = 64 throughout, so n = 64 is exactly the chunk."""
import numpy as np
import pytest
import torch

import inputgrad_model as im
import sitegrad_model as sm

pytestmark = pytest.mark.gpu
CHUNK = 64
DIMS_WIDE32 = [1, 2, 16, 600, 513, 130, 64, 2, 1]        # fp32 only: a bond between 513 and 1 024 at N = 8 (T = 16)


def _dataless(W, single_label=None, chunk=CHUNK):
    from tnml_amd.fixedl import TrainStates
    maxm = max(max(A.shape[0], A.shape[2]) for A in W)
    ts = TrainStates(np.zeros(1, dtype=np.int32), len(W), maxm, no_data=True, single_label=single_label)
    ts.set_mps(W)
    ts.set_option("gradient_chunk", chunk)
    return ts


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x.cpu() if torch.is_tensor(x) else x), np.asarray(y.cpu() if torch.is_tensor(y) else y)) for x, y in zip(a, b))


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _to(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if dev else a


def _map10():
    """a 2 x 2 block-sum map from 4 x 10 raw bytes onto the 10 sites of sm.odd_case(0, ..)"""
    from tnml_amd.input_map import InputMap
    return InputMap(4, 10, 2, 0, 0, 2, 5, InputMap.from_imglen(8, 4, "normal").table)


def _source(case, form, n, dev):
    """the images of a case in one input form -> the keyword of the streamed calls"""
    if form == "phi":
        return dict(phi=_to(case["phi"][:n], dev))
    if form == "u8":
        return dict(pixels=_to(case["pixels"][:n], dev))
    raw = np.random.default_rng(8).integers(0, 256, size=(n, _map10().S)).astype(np.uint8)
    return dict(pixels=_to(raw, dev))


def _parity(ts, src, coef, dtype="f64", want_sites=True, want_inputs=True, dev_back=None):
    """forward_taped + backward_taped against predict + backward(coef=..) on the same context, every array bit for bit; the taped pair
    runs first (the reference backward takes the tape).  -> the ticket"""
    dev = torch.is_tensor(next(iter(src.values())))
    dev_back = dev if dev_back is None else dev_back
    w, pred, t = ts.forward_taped(dtype=dtype, **src)
    assert t > 0 and ts.tape_ticket() == (t, len(coef))
    g, d = ts.backward_taped(t, _to(coef, dev_back), want_sites=want_sites, want_inputs=want_inputs)
    assert ts.tape_ticket() == (t, len(coef))                                       # a backward leaves the ticket alive
    got_c = ts.gradient_coef(len(coef))
    wr, pr = ts.predict(dtype=dtype, **src)
    ts.set_option("predict_dtype", 0)                                               # (the gradient calls are refused under predict_dtype = 1)
    gr, dr = ts.backward(coef=_to(coef, dev), want_sites=want_sites, want_inputs=want_inputs, dtype=dtype, **src)
    assert np.array_equal(got_c, coef) and np.array_equal(got_c, ts.gradient_coef(len(coef)))                       # the coefficients given, as backward(coef=..) leaves them under either dtype
    assert np.array_equal(_np(w), _np(wr)) and np.array_equal(_np(pred), _np(pr)) and np.abs(_np(w)).max() > 0
    if want_sites:
        assert _same(g, gr) and max(np.abs(_np(x)).max() for x in g) > 0
    else:
        assert g is None
    if want_inputs:
        assert np.array_equal(_np(d), _np(dr)) and np.abs(_np(d)).max() > 0
    else:
        assert d is None
    return t


# every value of every axis on sm.odd_case(0, ..): n, input form, predict_tile, gradient_dtype, memory space
AXES0 = [(1, "phi", 0, "f64", False), (37, "phi", 16, "f64", False), (64, "phi", 32, "f64", True), (37, "phi", 64, "f32", False),
         (37, "u8", 0, "f64", True), (64, "u8", 64, "f32", False), (1, "map", 0, "f32", True), (37, "map", 32, "f64", False),
         (64, "map", 16, "f64", False), (37, "phi", 0, "f32", True), (1, "u8", 16, "f32", False)]


@pytest.mark.parametrize("n,form,tile,dtype,dev", AXES0)
def test_parity_on_the_odd_bonds(n, form, tile, dtype, dev):
    case = sm.odd_case(0, 37 if n <= 37 else 64)
    ts = _dataless(case["W"])
    if form == "map":
        ts.set_input_map(_map10())
    ts.set_option("predict_tile", tile)
    _parity(ts, _source(case, form, n, dev), case["coef"][:n], dtype)
    ts.close()


@pytest.mark.parametrize("k,n,tile,dtype,dev", [(1, 37, 0, "f64", False), (1, 37, 64, "f32", True), (2, 37, 64, "f64", False), (2, 37, 32, "f32", False),
                                               (3, 17, 0, "f64", True), (3, 17, 64, "f32", False)])
def test_parity_on_the_other_tile_classes(k, n, tile, dtype, dev):
    """bonds to 128 (T = 64), to 300 (T = 32 in fp64) and the Label site at 512 x 2 x 511 x 10 (T = 16 in fp64, 32 in fp32)"""
    case = sm.odd_case(k, n)
    ts = _dataless(case["W"])
    ts.set_option("predict_tile", tile)
    _parity(ts, _source(case, "phi", n, dev), case["coef"], dtype)
    ts.close()


@pytest.mark.parametrize("n,dtype,dev,ws,wi", [(17, "f64", False, True, True), (1, "f32", True, True, False), (64, "f64", True, False, True)])
def test_parity_on_a_small_chain_and_with_one_output_only(n, dtype, dev, ws, wi):
    case = sm.small_case(12, 5, 17 if n <= 17 else 64)
    ts = _dataless(case["W"])
    _parity(ts, _source(case, "phi", n, dev), case["coef"][:n], dtype, want_sites=ws, want_inputs=wi)
    ts.close()


def test_parity_in_fp32_on_a_bond_above_512():
    imgs = sm._images(len(DIMS_WIDE32) - 1, 17, 5)
    W = sm.mps_with_dims(DIMS_WIDE32, 11)
    ts = _dataless(W)
    ts.set_option("predict_tile", 64)
    _parity(ts, dict(phi=imgs["phi"]), imgs["coef"], "f32")
    ts.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_chain_ends(dtype):
    """N = 4, Label site 2: the X side seeds bond 1 and carries nothing.  The per-label variant (cs = 1): the X workgroups return at once"""
    case = sm.small_case(4, 3, 17)
    ts = _dataless(case["W"])
    _parity(ts, dict(phi=case["phi"]), case["coef"], dtype)
    ts.close()
    base = sm.small_case(12, 5, 17)
    W1 = [A if A.ndim == 3 else A[..., 0] * 3.0 for A in base["W"]]
    ts = _dataless(W1, single_label=3)
    _parity(ts, dict(phi=base["phi"]), base["coef"][:, :1], dtype)
    _parity(ts, dict(phi=_to(base["phi"], True)), base["coef"][:, :1], dtype)
    ts.close()


def test_one_tape_serves_many_backwards_and_either_memory_space():
    case = sm.odd_case(0, 37)
    phi, c1 = case["phi"], case["coef"]
    c2 = np.random.default_rng(77).standard_normal(c1.shape)
    ts, ref = _dataless(case["W"]), _dataless(case["W"])
    _, _, t = ts.forward_taped(phi=phi)
    for c, dev in ((c1, False), (c2, True), (c1, True), (c2, False)):               # host and device backwards of a host forward
        g, d = ts.backward_taped(t, _to(c, dev))
        gr, dr = ref.backward(coef=c, phi=phi)
        assert _same(g, gr) and np.array_equal(_np(d), dr)
    _, _, t2 = ts.forward_taped(phi=_to(phi, True))                                 # a host backward of a device forward
    assert t2 > t
    g, d = ts.backward_taped(t2, c2)
    gr, dr = ref.backward(coef=c2, phi=phi)
    assert _same(g, gr) and np.array_equal(d, dr)
    ts.close(); ref.close()


def test_ten_unit_rows_give_the_jacobian_of_one_forward():
    """sum_s phi[n, j, s] dphi_l[n, j, s] = W_l(x_n) at every site j, for the ten unit coefficient rows on ONE ticket: the identity and the
    bound of tests/inputgrad_model.py (test_euler_tie_on_the_device_layers_tensors), with c = e_l"""
    case = sm.odd_case(0, 17)
    W, phi = case["W"], case["phi"]
    ts = _dataless(W)
    w, _, t = ts.forward_taped(phi=phi)
    K, U = im.rounding_count(len(W), 120, 10), 2.0 ** -53
    for l in range(10):
        coef = np.zeros((len(phi), 10)); coef[:, l] = 1.
        _, dphi = ts.backward_taped(t, coef, want_sites=False)
        _, w_abs, c_abs = im.abs_input_gradient(W, phi, coef=coef)
        bnd = im.bound(W, phi, coef=coef)
        allowed = (np.abs(phi) * bnd).sum(axis=2) + K * U * (c_abs * w_abs).sum(axis=1)[:, None]
        got = (phi * dphi).sum(axis=2)
        assert (np.abs(got - w[:, l:l + 1]) <= allowed).all(), l
        assert (allowed < 1e-6 * (c_abs * w_abs).sum(axis=1)[:, None]).all()
    assert ts.tape_ticket() == (t, len(phi))
    ts.close()


def _refused(ts, t, coef, killer):
    """backward_taped on a dead ticket: refused with the ticket and the killer's name, outputs untouched, context usable"""
    from tnml_amd import lib as _lib
    from tnml_amd.fixedl import TnmlError
    assert ts.tape_ticket() == (0, 0)
    with pytest.raises(TnmlError) as e:
        ts.backward_taped(t, coef)
    assert ("ticket %d" % t) in str(e.value) and killer in str(e.value), str(e.value)
    grad, dphi = np.full(ts._gradient_buffer().shape, 7.0), np.full((len(coef), ts.N, 2), 7.0)
    cf = np.ascontiguousarray(coef)
    assert ts._L.tnml_backward_taped(ts._h, t, _lib.dptr(cf), _lib.dptr(grad), _lib.dptr(dphi)) != 0
    assert (grad == 7.0).all() and (dphi == 7.0).all()
    gd, dd = torch.full(grad.shape, 7.0, dtype=torch.float64, device="cuda"), torch.full(dphi.shape, 7.0, dtype=torch.float64, device="cuda")
    o = _lib.DevOut(); o.grad, o.dphi = gd.data_ptr(), dd.data_ptr()
    cd = torch.from_numpy(cf).cuda()
    import ctypes as C
    assert ts._L.tnml_backward_taped_dev(ts._h, t, cd.data_ptr(), C.byref(o), torch.cuda.current_stream().cuda_stream) != 0
    torch.cuda.synchronize()
    assert bool((gd == 7.0).all()) and bool((dd == 7.0).all())


def test_ticket_life_cycle():
    case = sm.small_case(12, 5, 17)
    W, phi, coef, labels = case["W"], case["phi"], case["coef"], case["labels"]
    ts = _dataless(W)
    A3 = ts.get_site(3)
    A3d = ts.get_site(3, device=True)
    killers = [
        ("tnml_site_gradient_phi", lambda: ts.site_gradient(coef=coef, phi=phi)),
        ("tnml_backward_phi", lambda: ts.backward(coef=coef, phi=phi)),
        ("tnml_backward_dev", lambda: ts.backward(coef=_to(coef, True), phi=_to(phi, True))),
        ("tnml_site_step_phi", lambda: ts.gradient_step(labels=labels, phi=phi, lr=2.0 ** -30)),
        ("tnml_forward_taped", lambda: ts.forward_taped(phi=phi)),
        ("tnml_set_site", lambda: ts.set_site(3, A3)),
        ("tnml_set_site_dev", lambda: ts.set_site(3, A3d)),
        ("tnml_set_sites_dev", lambda: ts.set_sites([3], [A3d])),
        ("tnml_mps_place", lambda: ts.place(3, A3.shape[0], A3.shape[2], 0, 0, A3)),
        ("tnml_mps_compress", lambda: ts.compress(0.0)),
        ("a bond update", lambda: ts.svd_split(ts.bond_tensor(3), 3, 1, 0.0, 5, 5)),      # the split of a bond update, on bond 3 as it is
        ("gradient_chunk", lambda: ts.set_option("gradient_chunk", 128)),
        ("gradient_chunk", lambda: ts.set_option("gradient_chunk", 60)),                   # another value that rounds to the same capacity
        ("gradient_dtype", lambda: ts.set_option("gradient_dtype", 1)),
        ("tnml_set_input_map", lambda: ts.set_input_map(None)),
    ]
    for killer, kill in killers:
        _, _, t = ts.forward_taped(phi=phi)
        assert ts.tape_ticket() == (t, len(phi))
        kill()
        if killer == "tnml_forward_taped":
            assert ts.tape_ticket()[0] > t
            ts.set_site(3, A3)                                                      # (so that no ticket is live below)
            ts.tape_ticket()
        _refused(ts, t, coef, killer)
        ts.set_option("gradient_chunk", CHUNK); ts.set_option("gradient_dtype", 0)
        if killer == "tnml_site_step_phi":
            ts.set_mps(W); ts.step_reset()
        if killer in ("tnml_mps_place", "tnml_mps_compress", "a bond update"):
            ts.set_mps(W)
        _parity(ts, dict(phi=phi), coef)                                            # the context serves the next pair
    ts.close()


def test_what_does_not_take_the_tape_and_the_refusals_of_the_forward():
    from tnml_amd.fixedl import TnmlError
    case = sm.small_case(12, 5, 17)
    W, phi, coef, labels = case["W"], case["phi"], case["coef"], case["labels"]
    big = sm.small_case(12, 5, 70)
    ts, ref = _dataless(W), _dataless(W)
    _, _, t = ts.forward_taped(phi=phi)
    ts.predict(phi=phi); ts.evaluate(labels, phi=phi); ts.site_response(phi=phi)
    ts.predict(phi=phi, dtype="f32"); ts.set_option("predict_dtype", 0)
    ts.set_option("predict_tile", 64); ts.set_loss("softmax"); ts.set_loss("quadratic")
    assert ts.tape_ticket() == (t, len(phi))
    g, d = ts.backward_taped(t, coef)                                               # under predict_tile = 64, with the forward's tile
    gr, dr = ref.backward(coef=coef, phi=phi)
    assert _same(g, gr) and np.array_equal(d, dr)
    ts.set_option("predict_tile", 0)
    with pytest.raises(TnmlError, match=r"gradient_chunk = 64") as e:
        ts.forward_taped(phi=big["phi"])
    assert "70" in str(e.value)
    assert ts.tape_ticket() == (t, len(phi))                                        # a refused forward has touched nothing
    w0, p0, t0 = ts.forward_taped(phi=phi[:0])
    assert t0 == 0 and w0.shape == (0, 10) and ts.tape_ticket() == (t, len(phi))
    with pytest.raises(TnmlError, match="ticket 0"):
        ts.backward_taped(0, coef)
    with pytest.raises(TnmlError, match="not finite"):
        ts.backward_taped(t, np.where(np.arange(coef.size).reshape(coef.shape) == 13, np.inf, coef))
    with pytest.raises(TnmlError, match="not finite"):
        ts.backward_taped(t, _to(np.where(np.arange(coef.size).reshape(coef.shape) == 13, np.nan, coef), True))
    with pytest.raises(TnmlError, match="both NULL"):
        ts.backward_taped(t, coef, want_sites=False, want_inputs=False)
    for rows in (coef[:5], np.concatenate([coef, coef]), _to(coef[:5], True)):        # the live ticket's forward had 17 images
        with pytest.raises(ValueError, match="the forward of ticket %d had 17 images" % t):
            ts.backward_taped(t, rows)
    assert ts.tape_ticket() == (t, len(phi))
    # fp32: W scaled so that a weight leaves the fp32 range
    ts.set_mps([A * 1e8 for A in W])
    with pytest.raises(TnmlError, match="gradient_dtype"):
        ts.forward_taped(phi=phi, dtype="f32")
    assert ts.tape_ticket() == (0, 0)
    ts.close(); ref.close()


def _launches(ts, fn):
    ts.profile(True); ts.profile_reset()
    fn()
    got = {k: v[0] for k, v in ts.profile_read().items() if v[0]}
    ts.profile(False)
    return got


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_launches_by_class(dtype):
    case = sm.small_case(12, 5, 17)
    phi, coef = case["phi"], case["coef"]
    ts = _dataless(case["W"])
    ts.forward_taped(phi=phi, dtype=dtype)                                          # (the workspace is made)
    box = {}
    fwd = _launches(ts, lambda: box.update(t=ts.forward_taped(phi=phi)[2]))
    assert fwd.pop("fwd_taped") == 1 and "chain" not in fwd and "site_bwd" not in fwd and "site_out" not in fwd
    assert set(fwd) <= {"pack"}                                                     # staging, and under fp32 the copy of W
    for ws, wi in ((True, True), (True, False), (False, True)):
        bwd = _launches(ts, lambda: ts.backward_taped(box["t"], coef, want_sites=ws, want_inputs=wi))
        assert bwd.pop("site_out") == 1 and bwd.pop("site_grad", 0) == int(ws) and bwd.pop("input_grad", 0) == int(wi)
        assert bwd.pop("pack", 0) == int(wi)                                        # the transposition of dphi alone: no fp32 copy of W, no staging
        assert not bwd, bwd
    dev = _launches(ts, lambda: ts.backward_taped(box["t"], _to(coef, True)))
    assert dev == {"site_out": 1, "site_grad": 1, "input_grad": 1, "pack": 1, "io_check": 1}
    ts.close()


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("form,dtype", [("phi", "f64"), ("u8", "f64"), ("phi", "f32")])
def test_device_bytes_are_those_of_backward(form, dtype, dev):
    case = sm.small_case(12, 5, 17)
    src, coef = _source(case, form, 17, dev), case["coef"]
    a, b = _dataless(case["W"]), _dataless(case["W"])
    base = a.device_bytes()
    assert b.device_bytes() == base
    _, _, t = a.forward_taped(dtype=dtype, **src)
    a.backward_taped(t, _to(coef, dev))
    b.backward(coef=_to(coef, dev), dtype=dtype, **src)
    assert a.device_bytes() == b.device_bytes() > base
    a.close(); b.close()


def test_set_sites():
    from tnml_amd.fixedl import TnmlError
    case = sm.odd_case(1, 37)
    W = case["W"]
    N = len(W)
    rng = np.random.default_rng(4)
    new = [A + 0.01 * rng.standard_normal(A.shape) for A in W]
    a, b = _dataless(W), _dataless(W)
    for j, A in enumerate(new, start=1):
        a.set_site(j, A)
    tensors = [torch.from_numpy(np.ascontiguousarray(A)).cuda() for A in new]       # C-contiguous: brought into the library's layout first
    tensors[2] = b.get_site(3, device=True).copy_(torch.from_numpy(new[2]).cuda())  # and one that already is
    tensors[4] = tensors[4].float()                                                 # and one that is not fp64 (its values round)
    a.set_site(5, new[4].astype(np.float32))
    base = b.device_bytes()
    order = list(rng.permutation(N) + 1)
    got = _launches(b, lambda: b.set_sites(order, [tensors[j - 1] for j in order]))
    assert got == {"sites_copy": 1}
    assert b.device_bytes() == base + 32 * N
    assert all(np.array_equal(a.get_site(j), b.get_site(j)) for j in range(1, N + 1))
    assert not np.array_equal(b.get_site(2), W[1])
    b.set_sites([], [])                                                             # count = 0: nothing
    assert b.device_bytes() == base + 32 * N
    part = _launches(b, lambda: b.set_sites([N, 1], [torch.from_numpy(W[N - 1].copy()).cuda(), torch.from_numpy(W[0].copy()).cuda()]))
    assert part == {"sites_copy": 1} and np.array_equal(b.get_site(N), W[N - 1]) and np.array_equal(b.get_site(1), W[0])
    # refusals: W as it was, nothing launched
    import ctypes as C
    before = b.get_mps()
    good = [b.get_site(j, device=True) for j in (1, 2, 3)]
    host = np.ascontiguousarray(new[1]).ravel(order="F").copy()
    # memory from hipMalloc through the runtime that is already mapped: shorter than site 3 (torch's allocator would hand out a piece of a large block)
    from test_device_io_gpu import _hip_runtime
    hip = _hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    short, rbase, rsize = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(short), 256) == 0
    assert hip.hipMemGetAddressRange(C.byref(rbase), C.byref(rsize), short) == 0 and rsize.value < W[2].size * 8

    def raw(sites, ptrs):
        s = (C.c_int32 * len(sites))(*sites)
        p = (C.c_void_p * len(sites))(*ptrs)
        return b._L.tnml_set_sites_dev(b._h, len(sites), s, p, torch.cuda.current_stream().cuda_stream)

    for what, sites, ptrs in (("site 2 named twice", [1, 2, 2], [g.data_ptr() for g in good]), ("site 0 out of range", [1, 0, 3], [g.data_ptr() for g in good]),
                              ("site %d out of range" % (N + 1), [N + 1], [good[0].data_ptr()]), ("A_dev of site 2", [1, 2, 3], [good[0].data_ptr(), host.ctypes.data, good[2].data_ptr()]),
                              ("A_dev of site 3", [1, 2, 3], [good[0].data_ptr(), good[1].data_ptr(), short.value])):
        b.profile(True); b.profile_reset()
        assert raw(sites, ptrs) != 0
        msg = b._L.tnml_last_error(b._h).decode()
        assert what in msg, (what, msg)
        assert not any(v[0] for v in b.profile_read().values())
        b.profile(False)
    with pytest.raises(TnmlError, match="needs .* bytes"):
        b._ck(raw([3], [short.value]))
    assert hip.hipFree(short) == 0
    with pytest.raises(ValueError, match="site 2"):
        b.set_sites([2], [good[2]])
    assert _same(b.get_mps(), before)
    a.close(); b.close()


def _layer_step(W, phi, go, taped, device, compute_dtype, two_forwards=False):
    """one SGD step of an MPSLayer -> (out, phi.grad, site grads, parameters after, next forward, launches of the step by class)"""
    from tnml_amd.torch_layer import MPSLayer
    ts = _dataless(W)
    layer = MPSLayer(ts, train_sites=True, device=device, compute_dtype=compute_dtype, taped=taped)
    x = torch.tensor(phi, device=device or "cpu", requires_grad=True)
    g = torch.tensor(go, device=device or "cpu")
    ts.profile(True); ts.profile_reset()
    out = layer(x)
    if two_forwards:                                                                # the second forward takes the tape of the first
        assert torch.equal(layer(x), out)
    (out * g).sum().backward()
    counts = {k: v[0] for k, v in ts.profile_read().items() if v[0]}
    ts.profile(False)
    grads = [p.grad.detach().cpu().clone() for p in layer.sites]
    lr = 2.0 ** np.floor(np.log2(1e-3 / max(float(p.abs().max()) for p in grads)))   # a power of two: lr * grad is exact
    torch.optim.SGD(layer.parameters(), lr=lr).step()
    up = {}
    with torch.no_grad():
        ts.profile(True); ts.profile_reset()
        nxt = layer(x)
        up = {k: v[0] for k, v in ts.profile_read().items() if v[0]}
        ts.profile(False)
    res = (out.detach().cpu(), x.grad.detach().cpu(), grads, [p.detach().cpu().clone() for p in layer.sites], nxt.cpu(), counts, up)
    ts.close()
    return res


@pytest.mark.parametrize("compute_dtype", ["f64", "f32"])
@pytest.mark.parametrize("device", [None, "cuda"])
def test_layer_step_taped_equals_untaped(device, compute_dtype):
    case = sm.small_case(12, 5, 17)
    W, phi = case["W"], np.ascontiguousarray(case["phi"])
    go = np.random.default_rng(2).standard_normal((17, 10))
    plain = _layer_step(W, phi, go, False, device, compute_dtype)
    taped = _layer_step(W, phi, go, True, device, compute_dtype)
    stale = _layer_step(W, phi, go, True, device, compute_dtype, two_forwards=True)
    for got in (taped, stale):
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and torch.equal(got[4], plain[4])
        assert all(torch.equal(a, b) for a, b in zip(got[2], plain[2])) and all(torch.equal(a, b) for a, b in zip(got[3], plain[3]))
    assert plain[1].abs().max() > 0 and not torch.equal(plain[4], plain[0])
    assert plain[5].get("site_bwd") == 1 and plain[5].get("chain") == 1 and "fwd_taped" not in plain[5]
    assert "site_bwd" not in taped[5] and "chain" not in taped[5] and taped[5]["fwd_taped"] == 1 and taped[5]["site_out"] == 1
    assert stale[5].get("site_bwd") == 1 and stale[5]["fwd_taped"] == 2 and "site_out" not in stale[5]   # the stale ticket fell back
    if device:
        assert taped[6].get("sites_copy") == 1 and plain[6].get("sites_copy") == 1  # all 12 changed sites in one launch
    else:
        assert "sites_copy" not in taped[6]
    assert taped[6].get("chain") == 1 and "fwd_taped" not in taped[6]               # under no_grad nothing changes


def test_layer_batch_above_the_chunk_takes_the_old_path():
    case = sm.small_case(12, 5, 70)
    W, phi = case["W"], np.ascontiguousarray(case["phi"])
    go = np.random.default_rng(2).standard_normal((70, 10))
    plain = _layer_step(W, phi, go, False, "cuda", "f64")
    taped = _layer_step(W, phi, go, True, "cuda", "f64")
    assert torch.equal(taped[0], plain[0]) and torch.equal(taped[1], plain[1]) and all(torch.equal(a, b) for a, b in zip(taped[2], plain[2]))
    assert "fwd_taped" not in taped[5] and "site_out" not in taped[5] and taped[5]["site_bwd"] == 2 and taped[5]["chain"] >= 1
