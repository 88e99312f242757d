"""Softmax cross-entropy in the streamed gradient, step and evaluate (option loss = 1, tnml_amd/csrc/loss_dev.h).  The yardstick is
tests/loss_model.py (held to mpmath by tests/test_loss_model_host.py), fed the weights the device returns: coefficients, costs and
reports are compared bit for bit, the integers exactly.  The gradient is compared with the coef mode on the device's own coefficients,
the step with tests/sitestep_model.py fed the gradient site_gradient() returns.  Every context is data-less."""
import numpy as np
import pytest

import eval_model as em
import loss_model as lm
import sitegrad_model as sm
import sitestep_model as st

pytestmark = pytest.mark.gpu

SMALL = [(4, 2), (12, 5)]
TILES = [16, 32, 64]


def _dataless(W, single_label=None, **kw):
    from tnml_amd.fixedl import TrainStates
    maxm = max(max(A.shape[0], A.shape[2]) for A in W)
    ts = TrainStates(np.zeros(1, dtype=np.int32), len(W), maxm, no_data=True, single_label=single_label, **kw)
    ts.set_mps(W)
    return ts


def _src(case, form, rows=slice(None)):
    return dict(phi=case["phi"][rows]) if form == "phi" else dict(pixels=case["pixels"][rows])


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _softmax_ctx(case, beta=1.0, tile=None, chunk=None):
    ts = _dataless(case["W"])
    ts.set_loss("softmax", beta)
    assert ts.loss == "softmax"
    if tile is not None:
        ts.set_option("predict_tile", tile)
    if chunk is not None:
        ts.set_option("gradient_chunk", chunk)
        ts.set_option("predict_chunk", chunk)
    return ts


def _beta_for_both_branches(w):
    """a beta from the weights, with s the images' spreads max_l (m - w_l): beta (s_min + s_max) / 2 = 708, so that the image with the
    widest spread has an x_l < -708 and the one with the narrowest has none (the bytes' features give spreads within 1e-3 of each
    other, which is still 1e12 roundings apart; the caller asserts both on the model)"""
    spread = (w.max(axis=1)[:, None] - w).max(axis=1)
    assert spread.min() > 0 and spread.max() > (1 + 1e-9) * spread.min(), (spread.min(), spread.max())
    return 708.0 / (0.5 * (spread.min() + spread.max()))


def _check_coefficients(ts, case, form, rows, betas):
    labels = case["labels"][rows]
    for beta in betas:
        if beta == "both":
            _, (w0, _) = ts.site_gradient(labels=labels, want_weights=True, **_src(case, form, rows))
            beta = _beta_for_both_branches(w0)
        ts.set_loss("softmax", beta)
        _, (w, pred) = ts.site_gradient(labels=labels, want_weights=True, **_src(case, form, rows))
        e = lm.exponentials(w, beta)
        if beta not in (1.0, 8.0):
            zero = (e == 0).any(axis=1)
            print("beta", beta, "images with an e_l == 0:", int(zero.sum()), "of", len(e))
            assert zero.any() and (~zero).any()
        yield beta, w, pred, ts.gradient_coef()


@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("N,m", SMALL)
def test_coefficients_bit_for_bit(N, m, tile, form):
    """70 images: ragged last tiles at every width of the tid < T block; beta 1, 8 and one under which the -708 branch is taken on
    some images and not on others"""
    case = sm.small_case(N, m)
    ts = _softmax_ctx(case, tile=tile)
    for beta, w, pred, c in _check_coefficients(ts, case, form, slice(None), [1.0, 8.0, "both"]):
        assert c.shape == (70, 10)
        assert np.array_equal(c, lm.coefficients(w, case["labels"], beta)), beta
        assert np.array_equal(pred, em.predictions(w))
    ts.close()


@pytest.mark.parametrize("form", ["phi", "u8"])
def test_coefficients_of_the_last_chunk(form):
    """150 images in chunks of 64: gradient_coef() is the last chunk's, 22 images"""
    case = sm.odd_case(1, 150)
    ts = _softmax_ctx(case, chunk=64)
    for beta, w, pred, c in _check_coefficients(ts, case, form, slice(None), [1.0, 8.0, "both"]):
        assert c.shape == (22, 10)
        assert np.array_equal(c, lm.coefficients(w[128:], case["labels"][128:], beta)), beta
    ts.close()


@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("N,m", SMALL)
def test_gradient_is_the_coef_mode_on_the_device_coefficients(N, m, tile, form):
    case = sm.small_case(N, m)
    ts = _softmax_ctx(case, beta=8.0, tile=tile)
    G = ts.site_gradient(labels=case["labels"], **_src(case, form))
    c = ts.gradient_coef()
    assert np.abs(c).max() > 0
    Gc = ts.site_gradient(coef=c, **_src(case, form))
    assert _same(G, Gc)
    assert np.array_equal(ts.gradient_coef(), c)                 # (the coef mode leaves what it was given)
    ts.close()


@pytest.mark.parametrize("form", ["phi", "u8"])
def test_gradient_over_three_chunks(form):
    """the coefficients gathered by three one-chunk calls on the slices, then one 150-image call in each mode"""
    case = sm.odd_case(1, 150)
    ts = _softmax_ctx(case, beta=8.0, chunk=64)
    parts = []
    for rows in (slice(0, 64), slice(64, 128), slice(128, 150)):
        ts.site_gradient(labels=case["labels"][rows], **_src(case, form, rows))
        parts.append(ts.gradient_coef())
    c = np.concatenate(parts)
    assert c.shape == (150, 10)
    G = ts.site_gradient(labels=case["labels"], **_src(case, form))
    Gc = ts.site_gradient(coef=c, **_src(case, form))
    assert _same(G, Gc)
    ts.close()


def _check_evaluate(ts, case, form, beta, chunk):
    labels = case["labels"]
    for dtype in ("f64", "f32"):
        w, pred = ts.predict(dtype=dtype, **_src(case, form))
        rep, (w2, pred2) = ts.evaluate(labels, want_weights=True, **_src(case, form))
        assert np.array_equal(w, w2) and np.array_equal(pred, pred2)
        want = lm.report(w, labels, beta, chunk=chunk)
        print(dtype, "chunk", chunk, "cost", rep.cost, "ncorrect", rep.ncorrect, "of", rep.n)
        lm.same_report(rep, want)
        assert rep.cost > 0 and rep == ts.evaluate(labels, **_src(case, form))
    ts.set_option("predict_dtype", 0)


@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("N,m", SMALL)
def test_evaluate(N, m, tile, form):
    """cost and label_cost in k_eval_tally's order, integers by the signed decision; pred and weights are predict()'s; again under
    predict_chunk = 64 (two chunks) and under predict_dtype = 1 on the widened weights"""
    case = sm.small_case(N, m)
    for beta in (1.0, 8.0):
        ts = _softmax_ctx(case, beta=beta, tile=tile)
        _check_evaluate(ts, case, form, beta, 8192)
        ts.set_option("predict_chunk", 64)
        _check_evaluate(ts, case, form, beta, 64)
        ts.close()


def test_evaluate_three_chunks():
    case = sm.odd_case(1, 150)
    ts = _softmax_ctx(case, beta=8.0, chunk=64)
    _check_evaluate(ts, case, "phi", 8.0, 64)
    ts.close()


def _step(ts, W, state, batch, **par):
    """one step on the device and in the model (fed the gradient site_gradient() returns under the context's loss), compared: W,
    grad_norm, factor, clipped, t; eval is evaluate()'s of the batch before the step -> (the model's W after, its state, the report)"""
    method = par.get("method", "sgd")
    grads = ts.site_gradient(**batch)
    src = {k: v for k, v in batch.items() if k != "labels"}
    want_eval = ts.evaluate(batch["labels"], **src)
    if state is None:
        state = st.new_state(method, sum(g.size for g in grads))
    rep = ts.gradient_step(**batch, **par)
    Wm, state, mrep = st.step(W, st.flat(grads), state, **par)
    assert mrep["applied"]
    got = ts.get_mps()
    moved = max(float(np.abs(a - b).max()) for a, b in zip(W, Wm))
    print(method, "t", rep.t, "grad_norm", rep.grad_norm, "factor", rep.factor, "clipped", rep.clipped, "largest move", moved, "cost", rep.eval.cost)
    assert moved > 0
    assert _same(got, Wm)
    assert (rep.t, rep.grad_norm, rep.factor, rep.clipped) == (mrep["t"], mrep["grad_norm"], mrep["factor"], mrep["clipped"])
    assert rep.eval == want_eval and rep.eval.cost > 0
    return Wm, state, rep


def _state_equal(ts, state):
    like = ts.get_mps()
    for which in (("m", "v") if state["method"] == "adam" else ("v",)):
        assert _same(ts.step_state(which), st.unflat(state[which], like)), which


@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("N,m", SMALL)
def test_plain_sgd_step(N, m, tile, form):
    case = sm.small_case(N, m)
    ts = _softmax_ctx(case, beta=8.0, tile=tile)
    batch = dict(labels=case["labels"], **_src(case, form))
    Wm, state, rep = _step(ts, case["W"], None, batch, method="sgd", lr=1e-3, scale=1. / 70)
    assert rep.t == 1 and not rep.clipped and rep.factor == 1. / 70
    _state_equal(ts, state)
    ts.close()


def test_three_adam_steps_with_clipping():
    """odd_case(1, 150) in chunks of 64: batches of 40, 5 and 105 images (two chunks), a clip between the first two norms"""
    case = sm.odd_case(1, 150)
    ts = _softmax_ctx(case, beta=8.0, chunk=64)
    batches = [dict(labels=case["labels"][r], phi=case["phi"][r]) for r in (slice(0, 40), slice(40, 45), slice(45, 150))]
    norms = [st.factor(st.ordered_sumsq(st.flat(ts.site_gradient(**b))), 1., 0.)[0] for b in batches[:2]]
    assert max(norms) > 1.5 * min(norms), norms
    clip = float(np.sqrt(norms[0] * norms[1]))
    W, state, clipped = case["W"], None, []
    for k, b in enumerate(batches):
        W, state, rep = _step(ts, W, state, b, method="adam", lr=1e-3, clip=clip)
        assert rep.t == k + 1
        clipped.append(rep.clipped)
    assert any(clipped) and not all(clipped), clipped
    _state_equal(ts, state)
    ts.close()


def test_switching_back():
    """after set_loss("quadratic") the gradient and the report are those of a context that never saw loss = 1"""
    case = sm.small_case(12, 5)
    fresh = _dataless(case["W"])
    G0 = fresh.site_gradient(labels=case["labels"], phi=case["phi"])
    c0 = fresh.gradient_coef()
    r0 = fresh.evaluate(case["labels"], phi=case["phi"])
    fresh.close()
    ts = _softmax_ctx(case, beta=8.0)
    G1 = ts.site_gradient(labels=case["labels"], phi=case["phi"])
    r1 = ts.evaluate(case["labels"], phi=case["phi"])
    assert not _same(G0, G1) and r1.cost != r0.cost
    ts.set_loss("quadratic")
    assert ts.loss == "quadratic"
    assert _same(ts.site_gradient(labels=case["labels"], phi=case["phi"]), G0)
    assert np.array_equal(ts.gradient_coef(), c0)
    assert ts.evaluate(case["labels"], phi=case["phi"]) == r0
    ts.close()


def test_the_decision():
    """one label slice of the Label site times -3: its output is large and negative where it was positive.  The report follows the
    signed decision, the pred array the first maximum of |W_l|"""
    case = sm.small_case(12, 5)
    labels, phi = case["labels"], case["phi"]
    l0, W, wm = lm.decision_set(case["W"], phi)
    ndiff = int((lm.decisions(wm) != em.predictions(wm)).sum())
    assert 0 < ndiff < len(labels)
    ts = _dataless(W)
    ts.set_loss("softmax", 8.0)
    rep, (w, pred) = ts.evaluate(labels, phi=phi, want_weights=True)
    d = lm.decisions(w)
    print("label slice", l0, "the model's decisions differ on", ndiff, "images, the device's on", int((d != pred).sum()))
    assert (d != pred).any() and not (d != pred).all()
    assert np.array_equal(pred, em.predictions(w))
    lm.same_report(rep, lm.report(w, labels, 8.0))
    assert rep.ncorrect == int((d == labels).sum())
    conf = np.zeros((10, 10), dtype=np.int64)
    np.add.at(conf, (labels, d), 1)
    assert np.array_equal(rep.confusion, conf)
    conf_abs = np.zeros((10, 10), dtype=np.int64)
    np.add.at(conf_abs, (labels, pred), 1)
    assert not np.array_equal(rep.confusion, conf_abs)
    ts.close()


def test_refusals():
    from tnml_amd.fixedl import TnmlError
    case = sm.small_case(12, 5)
    labels, phi = case["labels"], case["phi"]
    ts = _dataless(case["W"])
    with pytest.raises(TnmlError, match="loss = 2, must be in 0..1"):
        ts.set_option("loss", 2)
    assert ts.loss == "quadratic"
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(TnmlError, match="loss_beta = %s" % ("nan" if bad != bad else "inf" if bad > 1 else "%g" % bad)):
            ts.set_option_real("loss_beta", bad)
        with pytest.raises(TnmlError, match="loss_beta"):
            ts.set_loss("softmax", bad)
        assert ts.loss == "quadratic"
    with pytest.raises(ValueError):
        ts.set_loss("hinge")
    with pytest.raises(TnmlError, match="no gradient or step call"):
        ts.gradient_coef()
    with pytest.raises(TnmlError, match="no gradient or step call"):
        ts.gradient_coef(70)
    ts.set_loss("softmax", 8.0)
    _, (w, _) = ts.site_gradient(labels=labels, phi=phi, want_weights=True)
    with pytest.raises(TnmlError, match="70 x 10 coefficients, count = 690"):
        ts.gradient_coef(69)
    assert np.array_equal(ts.gradient_coef(), lm.coefficients(w, labels, 8.0))      # every refusal above has left the context usable
    # weights that are not finite: the coefficients are NaN, the step refuses as it does under loss = 0, W stays
    big = phi.copy()
    big[:, [1, 5, 9], :] = 1e160
    W0 = ts.get_mps()
    with pytest.raises(TnmlError, match="out of range"):
        ts.gradient_step(labels=labels, phi=big, method="sgd", lr=1e-3)
    assert _same(ts.get_mps(), W0) and _same(W0, case["W"])
    assert np.isnan(ts.gradient_coef()).all()
    rep = ts.gradient_step(labels=labels, phi=phi, method="sgd", lr=1e-3)
    assert rep.t == 1
    ts.close()
    # one output has no softmax
    base = sm.small_case(6, 5)
    plain = [A if A.ndim == 3 else A[..., 0] * 3.0 for A in base["W"]]
    single = _dataless(plain, single_label=3)
    with pytest.raises(TnmlError, match="TNML_MODE_SINGLE"):
        single.set_loss("softmax")
    with pytest.raises(TnmlError, match="TNML_MODE_SINGLE"):
        single.set_option("loss", 1)
    assert single.loss == "quadratic"
    rep = single.evaluate(base["labels"], phi=base["phi"])
    assert rep.n == 70 and rep.cost > 0
    single.close()
