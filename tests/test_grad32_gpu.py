"""Streamed gradients in fp32 (option gradient_dtype = 1: the float instantiations of k_site_backward, k_site_grad and k_input_grad)
against the restatement of their arithmetic (grad32_model.py, proved on the host by test_grad32_model_host.py): np.array_equal on
weights, pred, grad and dphi, never a tolerance.  Contexts are data-less."""
import ctypes as C

import numpy as np
import pytest

import chain32_cases as cases
import chain32_model as cm
import grad32_model as gm
import sitestep_model as st

pytestmark = pytest.mark.gpu


def _dataless(W, single_label=None):
    from tnml_amd.fixedl import TrainStates
    maxm = max(max(A.shape[0], A.shape[2]) for A in W)
    ts = TrainStates(np.zeros(1, dtype=np.int32), len(W), maxm, no_data=True, single_label=single_label)
    ts.set_mps(W)
    return ts


def _src(d, form, rows=slice(None)):
    return dict(phi=d["forms"]["phi"][rows]) if form == "phi" else dict(pixels=d["pixels"][rows])


def _coefs(d, mode, rows=slice(None)):
    return dict(labels=d["labels"][rows]) if mode == "labels" else dict(coef=d["coef"][rows])


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _check(ts, d, form, mode, want, tag=""):
    """one backward call under gradient_dtype = 1 against the model's dict"""
    grads, dphi, (w, pred) = ts.backward(**_coefs(d, mode), **_src(d, form), want_weights=True, dtype="f32")
    diff = sum(int((a != b).sum()) for a, b in zip(grads, want["grads"]))
    print(tag, form, mode, "bits differ in", diff, "gradient values,", int((dphi != want["dphi"]).sum()), "dphi values,", int((w != want["weights"]).sum()), "weights")
    assert np.array_equal(w, want["weights"]) and np.array_equal(pred, want["pred"]), tag
    assert _same(grads, want["grads"]), tag
    assert np.array_equal(dphi, want["dphi"]), tag
    assert np.array_equal(dphi, dphi.astype(np.float32).astype(np.float64)), tag      # every dphi value is an fp32 widened
    return grads, dphi, w, pred


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("N,m", cases.SMALL)
def test_small_problems_are_the_model_bit_for_bit(N, m, form, mode):
    """70 images in chunks of 64 and 6"""
    d = gm.case("small", (N, m))
    ts = _dataless(d["W"])
    ts.set_option("gradient_chunk", 64)
    want = gm.model("small", (N, m), form, mode, 64)
    _, _, w, pred = _check(ts, d, form, mode, want)
    wp, pp = ts.predict(dtype="f32", **_src(d, form))                                 # phase A is the fp32 chain kernel's
    assert np.array_equal(w, wp) and np.array_equal(pred, pp)
    ts.set_option("predict_dtype", 0)                                                 # (the gradient calls refuse predict_dtype = 1)
    if mode == "labels":
        assert np.array_equal(ts.gradient_coef(6), want["coef"][64:])                 # the rounded coefficients, widened
    grads = ts.site_gradient(**_coefs(d, mode), **_src(d, form))                      # (the option holds: fp32 still)
    assert _same(grads, want["grads"])
    ts.close()


LISTS = [("dims", 0, "phi", "labels"), ("dims", 1, "u8", "coef"), ("dims", 2, "u8", "labels"), ("dims", 3, "phi", "coef"), ("1024", 0, "phi", "labels")]


@pytest.mark.parametrize("kind,key,form,mode", LISTS)
def test_every_tile_class_and_odd_shape(kind, key, form, mode):
    """bond dimensions 1, odd, ml != mr, up to 1 024, under predict_tile 0 and every width the fp32 cap allows at the list's largest bond"""
    from tnml_amd.fixedl import TnmlError
    d = gm.case(kind, key)
    top = max(max(A.shape[0], A.shape[2]) for A in d["W"])
    ts = _dataless(d["W"])
    if top > 512:                                                                     # fp64 stops at 512, in the words it has always used
        with pytest.raises(TnmlError, match=r"1024.*chain kernel serves bond dimensions up to 512.*tnml_classify"):
            ts.backward(**_coefs(d, mode), **_src(d, form), dtype="f64")
    want = gm.model(kind, key, form, mode)
    cap = 64 if top <= 256 else (32 if top <= 512 else 16)
    for tile in [0] + [t for t in (64, 32, 16) if t <= cap]:
        ts.set_option("predict_tile", tile)
        _check(ts, d, form, mode, want, "tile %d" % tile)
    ts.close()


def test_independence_of_repeats_tiles_and_batches():
    d = gm.case("small", (12, 4))
    phi, coef = d["forms"]["phi"], d["coef"]
    want = gm.model("small", (12, 4), "phi", "coef", 64)
    ts = _dataless(d["W"])
    ts.set_option("gradient_chunk", 64)
    ts.set_option("gradient_dtype", 1)
    for tile in (0, 64, 32, 16, 0):
        ts.set_option("predict_tile", tile)
        grads, dphi = ts.backward(coef=coef, phi=phi)
        assert _same(grads, want["grads"]) and np.array_equal(dphi, want["dphi"]), tile
        assert np.array_equal(ts.backward(coef=coef[69:], phi=phi[69:], want_sites=False)[1], want["dphi"][69:]), tile     # a 1-image call
    perm = np.random.default_rng(5).permutation(70)
    assert np.array_equal(ts.backward(coef=coef[perm], phi=phi[perm], want_sites=False)[1], want["dphi"][perm])
    cut = np.concatenate([ts.backward(coef=coef[a:b], phi=phi[a:b], want_sites=False)[1] for a, b in ((0, 1), (1, 18), (18, 70))])
    assert np.array_equal(cut, want["dphi"])
    ts.close()


def test_per_label_variant_under_an_input_map():
    """the map of test_f32_under_an_input_map (7 x 6 source, 2 x 2 blocks from (1, 0), 3 x 3 sites, a random table), site 1 plays the
    Label site"""
    from tnml_amd.input_map import InputMap
    rng = np.random.default_rng(77)
    ncodes = 255 * 4 + 1
    table = np.stack([1. + 0.1 * rng.standard_normal(ncodes), 0.5 * rng.standard_normal(ncodes)], axis=-1)
    m = InputMap(7, 6, 2, 1, 0, 3, 3, table)
    px = rng.integers(0, 256, (150, m.S), dtype=np.uint8)
    px[0] = 0
    px[1] = 255
    labels = rng.integers(0, 10, 150).astype(np.int32)
    W = [A if A.ndim == 3 else A[..., 0] * 3.0 for A in cases.mps_with_dims([1, 2, 5, 6, 3, 6, 4, 5, 2, 1], 5)]
    want = gm.backward32(W, m.features(px), labels=labels, target_label=3, chunk=64)
    ts = _dataless(W, single_label=3)
    ts.set_input_map(m)
    ts.set_option("gradient_chunk", 64)                                               # chunks of 64, 64 and 22
    for tile in (0, 16):
        ts.set_option("predict_tile", tile)
        grads, dphi, (w, pred) = ts.backward(labels=labels, pixels=px, want_weights=True, dtype="f32")
        assert np.array_equal(w, want["weights"]) and np.array_equal(pred, want["pred"]), tile
        assert _same(grads, want["grads"]) and np.array_equal(dphi, want["dphi"]), tile
    gf, df = ts.backward(labels=labels, phi=m.features(px))                           # the same features given: the same bits
    assert _same(gf, want["grads"]) and np.array_equal(df, want["dphi"])
    ts.close()


def test_softmax_loss():
    d = gm.case("small", (12, 4))
    phi = d["forms"]["phi"]
    want = gm.backward32(d["W"], phi, labels=d["labels"], chunk=64, loss="softmax", beta=2.5)
    ts = _dataless(d["W"])
    ts.set_option("gradient_chunk", 64)
    ts.set_loss("softmax", 2.5)
    grads, dphi, (w, pred) = ts.backward(labels=d["labels"], phi=phi, want_weights=True, dtype="f32")
    assert np.array_equal(w, want["weights"]) and np.array_equal(pred, want["pred"])
    assert np.array_equal(ts.gradient_coef(6), want["coef"][64:])
    assert _same(grads, want["grads"]) and np.array_equal(dphi, want["dphi"])
    ts.close()


@pytest.mark.parametrize("method,par", [("sgd", dict(lr=1e-3, momentum=0.9)), ("adam", dict(lr=1e-3))])
def test_the_step_is_the_model_on_the_fp32_gradient(method, par):
    """two steps under gradient_dtype = 1, a third under 0 on the same state: W after each is sitestep_model's on the gradient that
    site_gradient() returns at the W before it under the same option, bit for bit"""
    d = gm.case("small", (12, 4))
    batch = dict(labels=d["labels"], phi=d["forms"]["phi"])
    W = d["W"]
    ts = _dataless(W)
    ts.set_option("gradient_chunk", 64)
    state = None
    for t, dtype in enumerate(("f32", "f32", "f64")):
        grads = ts.site_gradient(dtype=dtype, **batch)
        if t == 0:
            assert _same(grads, gm.model("small", (12, 4), "phi", "labels", 64)["grads"])
            state = st.new_state(method, sum(g.size for g in grads))
        rep = ts.gradient_step(method=method, dtype=dtype, **batch, **par)
        W, state, mrep = st.step(W, st.flat(grads), state, method=method, **par)
        assert mrep["applied"] and rep.t == t + 1 == mrep["t"]
        assert _same(ts.get_mps(), W), (t, dtype)
        assert rep.grad_norm == mrep["grad_norm"]
    like = ts.get_mps()
    for which in (("m", "v") if method == "adam" else ("v",)):
        assert _same(ts.step_state(which), st.unflat(state[which], like)), which
    ts.close()


def test_device_tensors_and_the_torch_layer():
    import torch
    from tnml_amd.torch_layer import MPSLayer
    d = gm.case("small", (12, 4))
    W, phi, coef = d["W"], d["forms"]["phi"], d["coef"]
    dev = torch.device("cuda", 0)
    ts = _dataless(W)
    ts.set_option("gradient_chunk", 64)
    want = gm.model("small", (12, 4), "phi", "coef", 64)
    gh, dh, (wh, ph) = ts.backward(coef=coef, phi=phi, want_weights=True, dtype="f32")
    assert _same(gh, want["grads"]) and np.array_equal(dh, want["dphi"])
    gd, dd, (wd, pd) = ts.backward(coef=torch.from_numpy(coef).to(dev), phi=torch.from_numpy(phi).to(dev), want_weights=True)
    assert dd.dtype == torch.float64
    assert _same([g.cpu().numpy() for g in gd], gh) and np.array_equal(dd.cpu().numpy(), dh)
    assert np.array_equal(wd.cpu().numpy(), wh) and np.array_equal(pd.cpu().numpy(), ph)
    # fp32 features: they widen exactly, so the host call on the widened features is the yardstick, and the model on them
    phi32 = phi.astype(np.float32)
    want32 = gm.backward32(W, phi32.astype(np.float64), coef=coef, chunk=64)
    g32h, d32h = ts.backward(coef=coef, phi=phi32.astype(np.float64))
    assert _same(g32h, want32["grads"]) and np.array_equal(d32h, want32["dphi"])
    g32, d32 = ts.backward(coef=torch.from_numpy(coef).to(dev), phi=torch.from_numpy(phi32).to(dev))
    assert d32.dtype == torch.float32
    assert _same([g.cpu().numpy() for g in g32], g32h)
    assert np.array_equal(d32.cpu().numpy(), d32h.astype(np.float32)) and np.array_equal(d32.cpu().numpy().astype(np.float64), d32h)
    # the layer: forward under predict_dtype = 1, backward under gradient_dtype = 1, both options put back
    ts.set_option("gradient_dtype", 0)
    layer = MPSLayer(ts, train_sites=True, device=dev, compute_dtype="f32")
    x = torch.from_numpy(phi).to(dev).requires_grad_(True)
    out = layer(x)
    assert np.array_equal(out.detach().cpu().numpy(), wh)
    got = torch.autograd.grad(out, [x] + list(layer.sites), grad_outputs=torch.from_numpy(coef).to(dev))
    assert np.array_equal(got[0].cpu().numpy(), dh)
    assert _same([g.cpu().numpy() for g in got[1:]], gh)
    assert ts.get_dtype_option("predict_dtype") == 0 and ts.get_dtype_option("gradient_dtype") == 0
    w64 = ts.predict(phi=phi)[0]
    assert not np.array_equal(w64, wh) and np.abs(w64 - wh).max() < 1e-4 * np.abs(w64).max()
    g64 = ts.site_gradient(coef=coef, phi=phi)
    assert not _same(g64, gh)
    default = MPSLayer(ts, device=dev)                                                # the default is the fp64 layer
    assert default.compute_dtype == "f64" and np.array_equal(default(torch.from_numpy(phi).to(dev)).cpu().numpy(), w64)
    with pytest.raises(ValueError):
        MPSLayer(ts, compute_dtype="bf16")
    ts.close()


def test_refusals():
    from tnml_amd.fixedl import TnmlError
    d = gm.case("small", (12, 4))
    phi, coef = d["forms"]["phi"], d["coef"]
    ts = _dataless(d["W"])
    with pytest.raises(TnmlError, match="gradient_dtype"):
        ts.set_option("gradient_dtype", 2)
    with pytest.raises(TnmlError, match="gradient_dtype"):
        ts.set_option("gradient_dtype", -1)
    with pytest.raises(ValueError):
        ts.site_gradient(coef=coef, phi=phi, dtype="bf16")
    ts.set_option("predict_dtype", 1)
    for v in (0, 1):                                                                  # predict_dtype = 1 stays refused, whatever gradient_dtype says
        ts.set_option("gradient_dtype", v)
        with pytest.raises(TnmlError, match=r"predict_dtype = 1 \(fp32\): site gradients are computed in fp64 only \(set predict_dtype = 0\)"):
            ts.site_gradient(coef=coef, phi=phi)
        with pytest.raises(TnmlError, match=r"predict_dtype = 1 \(fp32\): site gradients are computed in fp64 only"):
            ts.backward(coef=coef, phi=phi)
        with pytest.raises(TnmlError, match=r"predict_dtype = 1 \(fp32\): site gradients are computed in fp64 only"):
            ts.gradient_step(coef=coef, phi=phi, lr=1e-3)
    ts.close()
    W = cases.mps_with_dims([1, 2, 16, 1025, 16, 2, 1], 11)
    ts = _dataless(W)
    with pytest.raises(TnmlError, match=r"1025.*fp32 chain kernel serves bond dimensions up to 1024.*tnml_classify"):
        ts.site_gradient(labels=np.zeros(3, dtype=np.int32), pixels=np.zeros((3, len(W)), dtype=np.uint8), dtype="f32")
    ts.close()


def test_leaving_the_fp32_range_fails_and_changes_nothing():
    from tnml_amd import lib as _lib
    from tnml_amd.fixedl import TnmlError
    d = gm.case("small", (12, 4))
    phi, coef = np.ascontiguousarray(d["forms"]["phi"]), np.ascontiguousarray(d["coef"])
    Wbig = [A * 1e5 for A in d["W"]]                                                  # the weights reach 1e60: far outside fp32, well inside fp64
    ts = _dataless(Wbig)
    ts.set_option("gradient_dtype", 1)
    grad = np.full(sum(A.size for A in Wbig), 7.0)
    dphi = np.full(phi.shape, 7.0)
    rc = ts._L.tnml_backward_phi(ts._h, len(phi), _lib.dptr(phi), None, _lib.dptr(coef), _lib.dptr(grad), _lib.dptr(dphi), None, None)
    assert rc != 0
    assert (grad == 7.0).all() and (dphi == 7.0).all()                                # untouched
    with pytest.raises(TnmlError, match=r"gradient_dtype = 1.*not finite.*gradient_dtype = 0"):
        ts.site_gradient(coef=coef, phi=phi)
    with pytest.raises(TnmlError, match="gradient_dtype"):
        ts.gradient_step(coef=coef, phi=phi, lr=1e-3)
    assert _same(ts.get_mps(), Wbig)                                                  # the step applied nothing
    g64, d64 = ts.backward(coef=coef, phi=phi, dtype="f64")                           # the context is usable, fp64 is in range
    assert all(np.isfinite(g).all() for g in g64) and np.isfinite(d64).all()
    ts.set_mps(d["W"])                                                                # and fp32 again, in range: the flag does not stick
    assert _same(ts.site_gradient(coef=coef, phi=phi, dtype="f32"), gm.model("small", (12, 4), "phi", "coef")["grads"])
    ts.close()


def _formula(W, chunk, f32, nl=10):
    """the gradient workspace with dphi for features given from the host, as include/tnml.h states it"""
    N = len(W)
    Cc = (chunk + 63) // 64 * 64
    B = 32 + sum((A.shape[2] + 15) // 16 * 16 for A in W[:-1])
    E = sum(A.size for A in W)
    W32 = sum((A.size + 3) // 4 * 4 for A in W)
    shared = 16 * N + 16 * nl * Cc + 8 * Cc + 4 * (N + 2) + 8 * (N + 1) + 4 * (N + nl) + 8 * E + 32 * N * Cc
    if not f32:
        return shared + 16 * B * Cc + 32 * N * Cc
    return shared + 8 * B * Cc + 4 * W32 + 16 * N + 4 + 16 * N * Cc + 8 * N * Cc


def _equal(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def test_workspace_life_cycle_across_predict_and_gradient():
    """One context through fp32 and fp64 calls of the predict and the gradient workspace, two tnml_set_input_map calls and a changed
    gradient_chunk: N = 8, bond dimension 12, 70 images in chunks of 64 and 6.  Every result is bit for bit what a fresh context
    returns for that single call (the values themselves are held by the model tests above): the fp32 sides of the two workspaces share
    nothing and a release leaves nothing stale.  After every step device_bytes() is the sum of what a context that only ever made
    the predict calls and one that only ever made the gradient calls report at that point, and a context created after this one was
    destroyed starts at the first one's figure.
    The map is that of test_f32_under_an_input_map (2 x 2 blocks from (1, 0), row 0 covered by no block, the same random table) on a
    9 x 4 source, so that it has 4 x 2 = 8 sites: that test's 7 x 6 source makes 9 sites, which a context of N = 8 refuses."""
    from tnml_amd.input_map import InputMap
    rng = np.random.default_rng(77)
    ncodes = 255 * 4 + 1
    table = np.stack([1. + 0.1 * rng.standard_normal(ncodes), 0.5 * rng.standard_normal(ncodes)], axis=-1)
    m = InputMap(9, 4, 2, 1, 0, 4, 2, table)
    assert m.N == 8
    px = rng.integers(0, 256, (70, m.S), dtype=np.uint8)
    px[0] = 0
    px[1] = 255
    phi = m.features(px)
    labels = rng.integers(0, 10, 70).astype(np.int32)
    W = cases.mps_with_dims([1] + [12] * 7 + [1], 5)

    def new():
        ts = _dataless(W)
        ts.set_option("predict_chunk", 64)
        ts.set_option("gradient_chunk", 64)
        return ts

    def predict32(ts, **images):
        got = ts.predict(dtype="f32", **images)
        ts.set_option("predict_dtype", 0)                                             # (the gradient calls refuse predict_dtype = 1)
        return got

    predict_phi = lambda ts: predict32(ts, phi=phi)
    predict_map = lambda ts: predict32(ts, pixels=px)
    back32_phi = lambda ts: ts.backward(labels=labels, phi=phi, want_weights=True, dtype="f32")
    back64_phi = lambda ts: ts.backward(labels=labels, phi=phi, want_weights=True, dtype="f64")
    back32_map = lambda ts: ts.backward(labels=labels, pixels=px, want_weights=True, dtype="f32")
    set_map = lambda ts: ts.set_input_map(m)
    chunk16 = lambda ts: ts.set_option("gradient_chunk", 16)
    # the steps: (what is done, the set-up a fresh context needs before that single call, which workspace's history it belongs to)
    steps = [(predict_phi, [], "pk"), (back32_phi, [], "sg"), (back64_phi, [], "sg"), (set_map, None, "both"), (predict_map, [set_map], "pk"),
             (set_map, None, "both"), (back32_map, [set_map], "sg"), (chunk16, None, "sg"), (back32_map, [set_map, chunk16], "sg"),
             (predict_map, [set_map], "pk")]
    # the predict workspace in closed form, as include/tnml.h states it (C = 64, maxm = 12 -> 16 parked rows): the shared part and the
    # parked vectors, fp32 features given from the host, the fp32 copy of W with its table and flag; under the map the bytes as given,
    # the block sums and the table in fp64 and fp32
    W32 = sum((A.size + 3) // 4 * 4 for A in W)
    pk_phi = (16 * 8 + 8 * 10 * 64 + 4 * 64 + 8 * 16 * 64) + (16 * 8 * 64 + 8 * 8 * 64) + (4 * W32 + 16 * 8 + 4)
    pk_map = m.S * 64 + 2 * 8 * 64 + 16 * ncodes + 8 * ncodes
    ts, only = new(), {"pk": new(), "sg": new()}
    base = ts.device_bytes()
    start = {k: c.device_bytes() for k, c in only.items()}
    assert start["pk"] == start["sg"] == base
    for i, (op, setup, ws) in enumerate(steps):
        got = op(ts)
        for k, c in only.items():
            if ws in (k, "both"):
                op(c)
        alive = {k: c.device_bytes() - start[k] for k, c in only.items()}
        print("step", i, "device bytes", ts.device_bytes() - base, "predict alone", alive["pk"], "gradient alone", alive["sg"])
        assert ts.device_bytes() - base == alive["pk"] + alive["sg"], i
        assert alive["pk"] == pk_phi + (pk_map if i in (4, 9) else 0), i                 # in closed form: the second tnml_set_input_map takes the map part off again, the last predict re-makes it
        if i == 1:
            assert alive["sg"] == _formula(W, 64, True)
        if i in (3, 5):
            assert alive["sg"] == 0, i                                                # tnml_set_input_map releases the gradient workspace whole
        if setup is not None:
            fresh = new()
            for s in setup:
                s(fresh)
            want = op(fresh)
            fresh.close()
            assert _equal(got, want), i
    for c in only.values():
        c.close()
    ts.close()
    again = new()
    assert again.device_bytes() == base
    again.close()


def test_workspace_launches_and_switching_back():
    d = gm.case("small", (12, 4))
    W, phi, coef = d["W"], d["forms"]["phi"], d["coef"]
    fresh = _dataless(W)                                                              # never sees the option
    fresh.set_option("gradient_chunk", 64)
    before = fresh.device_bytes()
    fresh.profile(True)
    fresh.profile_reset()
    g64, d64, (w64, p64) = fresh.backward(coef=coef, phi=phi, want_weights=True)
    prof64 = fresh.profile_read()
    fresh.profile(False)
    assert fresh.device_bytes() - before == _formula(W, 64, False)
    assert fresh.gradient_step(coef=coef[:0], phi=phi[:0], lr=1e-3).t == 0
    fresh.close()
    ts = _dataless(W)
    ts.set_option("gradient_chunk", 64)
    before = ts.device_bytes()
    g0 = ts.site_gradient(coef=coef[:0], phi=phi[:0], dtype="f32")                    # n = 0 succeeds, zeroes grad and allocates nothing
    assert all((g == 0).all() for g in g0) and ts.device_bytes() == before
    ts.profile(True)
    ts.profile_reset()
    g32, d32 = ts.backward(coef=coef, phi=phi)
    prof32 = ts.profile_read()
    ts.profile(False)
    print("device bytes: fp64", _formula(W, 64, False), "fp32", ts.device_bytes() - before)
    assert ts.device_bytes() - before == _formula(W, 64, True)                        # the tapes halve; the fp32 copy of W, its table and flag on top
    for kc in ("site_bwd", "site_grad", "input_grad"):
        assert prof32[kc][0] == prof64[kc][0] == 2, (kc, prof32[kc], prof64[kc])
    assert prof32["chain"][0] == 0
    assert not _same(g32, g64) and not np.array_equal(d32, d64)
    rel = max(np.abs(a - b).max() for a, b in zip(g32, g64)) / max(np.abs(b).max() for b in g64)
    print("relmax of G, fp32 against fp64:", rel)
    assert rel < 1e-4
    gb, db, (wb, pb) = ts.backward(coef=coef, phi=phi, want_weights=True, dtype="f64")   # back to fp64: the bits of the fresh context
    assert _same(gb, g64) and np.array_equal(db, d64) and np.array_equal(wb, w64) and np.array_equal(pb, p64)
    assert _same(ts.backward(coef=coef, phi=phi, dtype="f32")[0], g32)
    ts.close()
