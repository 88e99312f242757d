"""Streamed site gradients (tnml_site_gradient_u8 / tnml_site_gradient_phi, kernels_sitegrad.hip): G_j = sum_n sum_l c_nl dW_l(x_n)/dA_j
for every site.  The yardstick is tests/sitegrad_model.py with its own elementwise bound (proved by tests/test_sitegrad_model_host.py);
contexts are data-less unless the test is about a training context."""
import numpy as np
import pytest

import sitegrad_model as sm
from conftest import make_problem

pytestmark = pytest.mark.gpu


def _dataless(W, single_label=None):
    """a context that holds no images: sized by W alone"""
    from tnml_amd.fixedl import TrainStates
    maxm = max(max(A.shape[0], A.shape[2]) for A in W)
    ts = TrainStates(np.zeros(1, dtype=np.int32), len(W), maxm, no_data=True, single_label=single_label)
    ts.set_mps(W)
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
    """the device's gradient within the model's bound; weights and pred those of predict(), bit for bit"""
    g_m, _, bnd = sm.model_of(case, form, mode, target)
    grads, (w, pred) = ts.site_gradient(want_weights=True, **_coefs(case, mode, target), **_src(case, form))
    assert [g.shape for g in grads] == [A.shape for A in case["W"]]
    ratio = sm.worst_ratio(grads, g_m, bnd)
    print("worst error / bound", ratio, "largest |G|", max(np.abs(g).max() for g in g_m))
    assert ratio <= 1.
    wp, pp = ts.predict(**_src(case, form))
    assert np.array_equal(w, wp) and np.array_equal(pred, pp)
    return grads, w


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("n", [1, 37, 70, 150])
@pytest.mark.parametrize("k", range(len(sm.DIMS)))
def test_gradient_matches_the_model_on_every_tile_class_and_odd_shape(k, n, form, mode):
    """bonds of 1, odd bonds, ml != mr, output blocks that are not full, the three tile widths, the Label site at 512 x 2 x 511 x 10;
    one image, a partial tile, more than one tile"""
    case = sm.odd_case(k, n)
    ts = _dataless(case["W"])
    _check_against_model(ts, case, form, mode)
    ts.close()


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("N,m", [(4, 2), (4, 3), (12, 5), (17, 6)])
def test_gradient_short_chains(N, m, form, mode):
    case = sm.small_case(N, m)
    ts = _dataless(case["W"])
    _check_against_model(ts, case, form, mode)
    g0 = ts.site_gradient(phi=case["phi"][:0], labels=case["labels"][:0])           # n = 0 succeeds and zeroes grad
    assert [g.shape for g in g0] == [A.shape for A in case["W"]] and not any(g.any() for g in g0)
    ts.close()


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("N", [6, 12])
def test_gradient_per_label_variant(N, mode):
    """TNML_MODE_SINGLE: one output, site 1 plays the Label site, no left chain; y_n = [label_n == target_label]"""
    base = sm.small_case(N, 5)
    case = sm._CACHE.setdefault(("plain", N), dict(base, W=_plain(base["W"])))
    ts = _dataless(case["W"], single_label=3)
    _, w = _check_against_model(ts, case, "phi", mode, target=3)
    assert w.shape == (70, 1)
    ts.close()


@pytest.mark.parametrize("side,imglen", [(8, 4), (28, 14)])
def test_gradient_under_an_input_map(side, imglen):
    """raw bytes through the device input map, a 2 x 2 block mean: the bits of the feature path on the features the map defines, and
    inside the model's bound (which has teeth at 16 sites; on this W the contraction on absolute values is orders above |G| over 196
    sites: tests/test_long_chain_gpu.py holds the call to a bound with teeth at 196 and 784 sites under the map)"""
    from tnml_amd import synth
    from tnml_amd.input_map import InputMap
    m = InputMap.from_imglen(side, imglen, "normal")
    rng = np.random.default_rng(8)
    raw = rng.integers(0, 256, size=(20, m.S)).astype(np.uint8)
    labels = rng.integers(0, 10, size=20).astype(np.int32)
    W = synth.random_mps(m.N, 6, seed=4)
    ts = _dataless(W)
    ref, (w_ref, p_ref) = ts.site_gradient(labels=labels, phi=m.features(raw), want_weights=True)
    ts.set_input_map(m)
    got, (w, p) = ts.site_gradient(labels=labels, pixels=raw, want_weights=True)
    assert max(np.abs(g).max() for g in got) > 0
    assert _same(got, ref) and np.array_equal(w, w_ref) and np.array_equal(p, p_ref)
    g_m, _ = sm.site_gradient(W, m.features(raw), labels=labels)
    ratio = sm.worst_ratio(got, g_m, sm.bound(W, m.features(raw), labels=labels))
    print("worst error / bound", ratio)
    assert ratio <= 1.
    ts.close()


@pytest.mark.parametrize("k", [0, 1])
def test_gradient_over_several_tiles_and_chunks(k):
    """bit-identical across the tile widths and on repeats; chunks of 64 against one of 512 within the bound, weights and pred
    bit-identical; a large call leaves nothing behind for a small one (the tape of the tiles a launch did not write is not read)"""
    case = sm.odd_case(k, 150)
    kw = dict(labels=case["labels"], phi=case["phi"])
    ts = _dataless(case["W"])
    full, (w, p) = ts.site_gradient(want_weights=True, **kw)
    assert _same(ts.site_gradient(**kw), full)
    for tile in (16, 32, 64):
        ts.set_option("predict_tile", tile)
        assert _same(ts.site_gradient(**kw), full), tile
    ts.set_option("predict_tile", 0)
    small = ts.site_gradient(labels=case["labels"][:20], phi=case["phi"][:20])      # after n = 150 on the same context
    fresh = _dataless(case["W"])
    assert _same(small, fresh.site_gradient(labels=case["labels"][:20], phi=case["phi"][:20]))
    fresh.close()
    ts.set_option("gradient_chunk", 64)
    cut, (wc, pc) = ts.site_gradient(want_weights=True, **kw)
    assert np.array_equal(wc, w) and np.array_equal(pc, p)
    ratio = sm.worst_ratio(cut, full, sm.model_of(case, "phi", "labels")[2])
    print("chunks of 64 against 512: worst difference / bound", ratio)
    assert ratio <= 1.
    assert _same(ts.site_gradient(**kw), cut)
    ts.set_option("gradient_chunk", 50)                                             # chunks that are no multiple of the tile or of 4
    ratio = sm.worst_ratio(ts.site_gradient(**kw), full, sm.model_of(case, "phi", "labels")[2])
    assert ratio <= 1.
    ts.close()


def test_grad_is_overwritten_not_added_to():
    case = sm.small_case(12, 5)
    ts = _dataless(case["W"])
    a = ts.site_gradient(coef=case["coef"], phi=case["phi"])
    b = ts.site_gradient(labels=case["labels"][:33], pixels=case["pixels"][:33])
    fresh = _dataless(case["W"])
    assert _same(b, fresh.site_gradient(labels=case["labels"][:33], pixels=case["pixels"][:33]))
    assert not _same(a, b)
    # through the C call: what the caller's array held before does not matter
    import ctypes as C
    from tnml_amd import lib as _lib
    flat = np.full(sum(g.size for g in b), 7.5)
    lab = np.ascontiguousarray(case["labels"][:33], dtype=np.int32)
    x = np.ascontiguousarray(case["pixels"][:33], dtype=np.uint8)
    rc = ts._L.tnml_site_gradient_u8(ts._h, 33, x.ctypes.data_as(C.POINTER(C.c_uint8)), lab.ctypes.data_as(C.POINTER(C.c_int32)), None, _lib.dptr(flat), None, None)
    assert rc == 0 and np.array_equal(flat, np.concatenate([g.ravel(order="F") for g in b]))
    ts.close()
    fresh.close()


def test_identities_on_the_device_alone():
    """Euler: sum A_j G_j = sum_n sum_l c_nl W_l(x_n) at every site, against the call's own weights; and one image with a one-hot
    coefficient gives site_response(): sum_{a, r} A_j G_j [s] = phi_s resp[j][s]"""
    case = sm.odd_case(0, 70)
    W, phi = case["W"], case["phi"]
    ts = _dataless(W)
    K, _ = sm.rounding_counts(len(W), 120, 70, 10)
    for mode in ("labels", "coef"):
        grads, (w, _) = ts.site_gradient(phi=phi, want_weights=True, **_coefs(case, mode))
        coef = case["coef"] if mode == "coef" else 2. * (w - sm.targets(case["labels"], 10))
        _, _, bnd = sm.model_of(case, "phi", mode)
        _, w_abs, c_abs = sm.abs_gradient(W, phi, **_coefs(case, mode))
        want = (coef * w).sum()
        for j, (A, G) in enumerate(zip(W, grads)):
            allowed = (np.abs(A) * bnd[j]).sum() + K * sm.U * (c_abs * w_abs).sum()
            assert abs((A * G).sum() - want) <= allowed, (mode, j, (A * G).sum(), want, allowed)
    for i, label in ((0, 4), (33, 0), (69, 9)):
        coef = np.zeros((1, 10))
        coef[0, label] = 1.
        grads = ts.site_gradient(phi=phi[i:i + 1], coef=coef)
        resp = ts.site_response(phi=phi[i:i + 1], which=np.array([label], dtype=np.int32))
        bnd = sm.bound(W, phi[i:i + 1], coef=coef)
        for j, (A, G) in enumerate(zip(W, grads)):
            axes = (0, 2) if A.ndim == 3 else (0, 2, 3)
            allowed = 2 * (np.abs(A) * bnd[j]).sum(axis=axes)
            assert (np.abs((A * G).sum(axis=axes) - phi[i, j] * resp[0, j]) <= allowed).all(), (i, j)
    ts.close()


def test_finite_differences_through_the_public_calls():
    """perturb one site with set_site, take the cost from evaluate(): the first, the Label and the last site of N = 9, bonds up to 33"""
    dims = [1, 2, 5, 9, 33, 17, 7, 3, 2, 1]
    W = sm.mps_with_dims(dims, 21)
    _, labels, phi, _ = make_problem(9, 40, 2, 7, pixel_boost=200.0)
    labels = np.asarray(labels, dtype=np.int32)
    ts = _dataless(W)
    grads = ts.site_gradient(labels=labels, phi=phi)
    bnd = sm.bound(W, phi, labels=labels)
    rng = np.random.default_rng(9)
    for j in (0, 3, 8):
        D = rng.standard_normal(W[j].shape)
        eps = sm.fd_eps(W[j], D)
        ts.set_site(j + 1, W[j] + eps * D)
        plus = ts.evaluate(labels, phi=phi).cost
        ts.set_site(j + 1, W[j] - eps * D)
        minus = ts.evaluate(labels, phi=phi).cost
        ts.set_site(j + 1, W[j])
        fd = (plus - minus) / (2 * eps)
        allowed = sm.fd_allowed(W, phi, labels, j, D, eps, bnd[j])
        print("site", j + 1, "central difference", fd, "<G, D>", (grads[j] * D).sum(), "allowed", allowed)
        assert abs(fd - (grads[j] * D).sum()) <= allowed
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


def test_gradient_leaves_a_training_context_alone():
    from tnml_amd.fixedl import TnmlError
    sweep = (4, 2, 1e-10, 3, 1e-3, 1e-10)
    others = make_problem(12, 33, 4, 11, pixel_boost=200.0)
    lab = np.asarray(others[1], dtype=np.int32)
    reports, got = [], []
    for call in (False, True):
        ts, W = _train_ctx()
        ts.bond_update_begin(1, 1, *sweep)
        if call:
            with pytest.raises(TnmlError, match="bond update is in flight"):
                ts.site_gradient(labels=lab, phi=others[2])
        first = ts.bond_update_end()
        if call:                                                # on a context that holds data and environments, between two bond updates
            got.append(ts.site_gradient(labels=lab, phi=others[2]))
            got.append(ts.site_gradient(labels=lab, phi=others[2]))
            Wnow = ts.get_mps()
        reports.append((first, ts.bond_update(2, 1, *sweep)))
        ts.close()
    _same_report(reports[0][0], reports[1][0])
    _same_report(reports[0][1], reports[1][1])
    assert _same(got[0], got[1])
    g_m, _ = sm.site_gradient(Wnow, others[2], labels=lab)
    ratio = sm.worst_ratio(got[0], g_m, sm.bound(Wnow, others[2], labels=lab))
    print("worst error / bound on the trained W", ratio)
    assert ratio <= 1.


def _ru16(m):
    return (m + 15) // 16 * 16


def _staging(N, C, forms, imap=None):
    """the staging of the input forms a streamed workspace has served since it was made, as include/tnml.h states it"""
    per = {"u8": 2 * N * C, "phi": 32 * N * C}
    if imap is not None:
        per["map"] = imap.S * C + 2 * N * C + 16 * imap.ncodes
    return sum(per[f] for f in ([forms] if isinstance(forms, str) else forms))


def _formula(W, chunk, staging, nl=10, imap=None):
    """the workspace of tnml_site_gradient_* as include/tnml.h states it"""
    N = len(W)
    C = (chunk + 63) // 64 * 64
    B = 32 + sum(_ru16(A.shape[2]) for A in W[:-1])
    E = sum(A.size for A in W)
    return 16 * N + 16 * nl * C + 8 * C + 4 * (N + 2) + 8 * (N + 1) + 4 * (N + nl) + 8 * E + 16 * B * C + _staging(N, C, staging, imap)


def _formula_response(W, chunk, staging, nl=10, imap=None):
    """the workspace of tnml_response_* as include/tnml.h states it"""
    N = len(W)
    C = (chunk + 63) // 64 * 64
    label_site = next(A for A in W if A.ndim == 4)
    B = 32 + sum(_ru16(A.shape[2]) for A in W[:-1]) + _ru16(label_site.shape[0]) + _ru16(label_site.shape[2])
    return 16 * N + 8 * nl * C + 8 * C + 4 * (N + 4) + 32 * N * C + 8 * B * C + _staging(N, C, staging, imap)


def _formula_predict(W, chunk, staging, nl=10, imap=None):
    """the fp64 workspace of tnml_predict_* as include/tnml.h states it, on a context whose maxm is the largest bond of W"""
    N = len(W)
    C = (chunk + 63) // 64 * 64
    M = _ru16(min(max(max(A.shape[0], A.shape[2]) for A in W), 512))
    return 16 * N + 8 * nl * C + 4 * C + 8 * M * C + _staging(N, C, staging, imap)


def test_gradient_bookkeeping():
    """one launch of each kernel per chunk and none of the response or chain kernels; the workspace is the header's formula, does not
    grow with the image count, follows gradient_chunk and goes with the input map"""
    case = sm.small_case(12, 5)
    W = case["W"]
    ts = _dataless(W)
    before = ts.device_bytes()
    ts.set_option("gradient_chunk", 16)
    ts.profile(True)
    ts.profile_reset()
    g16 = ts.site_gradient(labels=case["labels"], phi=case["phi"])
    prof = ts.profile_read()
    ts.profile(False)
    assert prof["site_bwd"][0] == 5 and prof["site_grad"][0] == 5, prof
    assert prof["site_resp"][0] == 0 and prof["chain"][0] == 0 and prof["eval_tally"][0] == 0, prof
    assert ts.device_bytes() - before == _formula(W, 16, "phi")
    ts.set_option("gradient_chunk", 512)
    g = ts.site_gradient(labels=case["labels"], phi=case["phi"])
    assert ts.device_bytes() - before == _formula(W, 512, "phi")
    ratio = sm.worst_ratio(g16, g, sm.model_of(case, "phi", "labels")[2])
    assert ratio <= 1.
    big = ts.site_gradient(labels=np.tile(case["labels"], 30), phi=np.tile(case["phi"], (30, 1, 1)))     # 2 100 images
    assert ts.device_bytes() - before == _formula(W, 512, "phi")
    assert max(np.abs(x).max() for x in big) > max(np.abs(x).max() for x in g)
    ts.site_gradient(labels=case["labels"], pixels=case["pixels"])
    assert ts.device_bytes() - before == _formula(W, 512, "phi") + 2 * 12 * 512
    ts.set_input_map(None)                                      # released with the map's workspaces
    assert ts.device_bytes() == before
    ts.site_gradient(labels=case["labels"], pixels=case["pixels"])
    assert ts.device_bytes() - before == _formula(W, 512, "u8")
    ts.close()


def _call(ts, n, x, labels, coef, flat):
    import ctypes as C
    from tnml_amd import lib as _lib
    lp = None if labels is None else labels.ctypes.data_as(C.POINTER(C.c_int32))
    cp = None if coef is None else _lib.dptr(coef)
    rc = ts._L.tnml_site_gradient_phi(ts._h, n, _lib.dptr(x), lp, cp, _lib.dptr(flat), None, None)
    return rc, ts._L.tnml_last_error(ts._h).decode()


def test_gradient_refusals_leave_the_context_usable_and_grad_untouched():
    from tnml_amd.fixedl import TnmlError, TrainStates
    W513 = sm.mps_with_dims([1, 2, 16, 513, 16, 2, 1], 11)
    ts = _dataless(W513)
    with pytest.raises(TnmlError, match="tnml_classify"):
        ts.site_gradient(labels=np.zeros(3, dtype=np.int32), pixels=np.zeros((3, len(W513)), dtype=np.uint8))
    ts.close()
    case = sm.small_case(12, 5)
    W, phi, labels, coef = case["W"], np.ascontiguousarray(case["phi"]), case["labels"], np.ascontiguousarray(case["coef"])
    bare = TrainStates(np.zeros(1, dtype=np.int32), 12, 5, no_data=True)             # W incomplete
    with pytest.raises(TnmlError, match="site 1 not set"):
        bare.site_gradient(labels=labels, phi=phi)
    bare.close()
    ts = _dataless(W)
    good = ts.site_gradient(labels=labels, phi=phi)
    elems = sum(g.size for g in good)

    def refused(match, lab, cf):
        flat = np.full(elems, 7.5)
        rc, msg = _call(ts, 70, phi, lab, cf, flat)
        assert rc != 0 and match in msg, msg
        assert (flat == 7.5).all()                                # grad untouched

    refused("exactly one of labels and coef", labels, coef)
    refused("exactly one of labels and coef", None, None)
    bad = labels.copy()
    bad[41] = 10
    refused("image 41", bad, None)
    bad[41] = -1
    refused("image 41", bad, None)
    for v in (np.nan, np.inf):
        cf = coef.copy()
        cf[57, 3] = v
        refused("image 57 is not finite", None, cf)
    assert _same(ts.site_gradient(labels=labels, phi=phi), good)
    ts.set_option("predict_dtype", 1)
    refused("predict_dtype", labels, None)
    ts.set_option("predict_dtype", 0)
    assert _same(ts.site_gradient(labels=labels, phi=phi), good)
    ts.close()
    # a context attached as a held-out set refuses, the training context it is attached to serves
    train, _ = _train_ctx()
    held = make_problem(12, 40, 4, 17, pixel_boost=200.0)
    hs = TrainStates(held[1], 12, 4, phi=held[2])
    train.attach_heldout(hs)
    with pytest.raises(TnmlError, match="attached as a held-out set"):
        hs.site_gradient(labels=labels, phi=phi)
    assert len(train.site_gradient(labels=labels, phi=phi)) == 12
    train.close()
    hs.close()


def test_descent_step_lowers_the_cost():
    """three steps of gradient descent with backtracking on 70 images at N = 12, m = 5"""
    case = sm.small_case(12, 5)
    ts = _dataless(case["W"])
    cost = lambda: ts.evaluate(case["labels"], pixels=case["pixels"]).cost
    costs, steps = [cost()], []
    for _ in range(3):
        grads = ts.site_gradient(labels=case["labels"], pixels=case["pixels"])
        steps.append(ts.descent_step(grads, cost, 1e-2))
        costs.append(cost())
    print("costs", costs, "steps", steps)
    assert all(b < a for a, b in zip(costs, costs[1:])) and all(s > 0 for s in steps)
    ts.close()


def _leaves(x):
    return [x] if isinstance(x, np.ndarray) else [a for part in x for a in _leaves(part)]


def test_the_three_streamed_workspaces_leave_one_another_alone():
    """predict, response and gradient interleaved on one context: N = 12, bonds up to 5, 70 images in chunks of 64 (two chunks, a ragged
    tail of 6).  After every round each result is what a fresh context gives that makes that one call alone, bit for bit, and the
    context holds the sum of the three workspaces of include/tnml.h for the input forms each has served since it was made."""
    from tnml_amd import hostlib
    from tnml_amd.input_map import InputMap
    case = sm.small_case(12, 5)
    W = case["W"]
    imap = InputMap(6, 8, 2, 0, 0, 3, 4, hostlib.feature_table("normal", 1.0, 2), feature="normal")      # 48 bytes -> 3 x 4 sites
    raw = np.random.default_rng(12).integers(0, 256, size=(70, imap.S)).astype(np.uint8)
    sources = {"phi": dict(phi=case["phi"]), "u8": dict(pixels=case["pixels"]), "map": dict(pixels=raw)}
    kinds = ("predict", "response", "gradient")
    chunk = dict.fromkeys(kinds, 64)
    formula = dict(predict=_formula_predict, response=_formula_response, gradient=_formula)

    def call(ctx, kind, form):
        if kind == "predict":
            return ctx.predict(**sources[form])
        if kind == "response":
            return ctx.site_response(want_weights=True, **sources[form])
        return ctx.site_gradient(labels=case["labels"], want_weights=True, **sources[form])

    alone = {}

    def fresh(kind, form):
        """that one call on a context of its own, in the options and the map of the moment; once per (call, form, chunk)"""
        key = (kind, form, chunk[kind])
        if key not in alone:
            ctx = _dataless(W)
            for k in kinds:
                ctx.set_option(k + "_chunk", chunk[k])
            if form == "map":
                ctx.set_input_map(imap)
            alone[key] = _leaves(call(ctx, kind, form))
            ctx.close()
        return alone[key]

    ts = _dataless(W)
    before = ts.device_bytes()
    for k in kinds:
        ts.set_option(k + "_chunk", 64)
    served = {k: [] for k in kinds}                                # the input forms a workspace has staged since it was made

    def round_of(form):
        for k in kinds:
            got = _leaves(call(ts, k, form))
            assert _same(got, fresh(k, form)), (k, form, chunk[k])
            assert all(a.any() for a in got if a.dtype.kind == "f"), (k, form)
            if form not in served[k]:
                served[k].append(form)
        want = sum(formula[k](W, chunk[k], served[k], imap=imap) for k in kinds)
        print(form, chunk, "device bytes", ts.device_bytes() - before, "tnml.h", want)
        assert ts.device_bytes() - before == want, (form, served)

    round_of("phi")
    round_of("u8")
    ts.set_input_map(imap)          # predict keeps its workspace but for the map's part; response and gradient are released whole
    served["response"], served["gradient"] = [], []
    round_of("map")
    ts.set_option("response_chunk", 128)                            # re-makes the response workspace alone
    chunk["response"], served["response"] = 128, []
    round_of("map")
    ts.close()
