"""The streamed calls at the chain lengths they are used at (N = 784, 197, 196): predict in fp64 and fp32, evaluate, site_response,
site_gradient and gradient_step on the cases of tests/long_chain_cases.py, against the models that tests/test_long_chain_host.py
proves on the CPU.  At these lengths the walk control of chain_walk_taped / k_chain (site_at, the parity of the ping-pong tiles after
N - 1 steps, the parked vector, the tape's region table), the block and workgroup searches of k_site_grad / k_site_step and the
[cnt][N][2] transpose of resp run far beyond the 4 to 17 sites of the other GPU tests, and the bounds of the models still have teeth:
the host file asserts that they are at most 1e-8 of what they bound.

Every check prints `long_chain_ratio <case> <call> <form> <worst error / bound>`; one run's lines are kept in
profiles/long_chain_ratios.txt.  Nothing is asserted on them beyond <= 1.  Contexts are data-less."""
import numpy as np
import pytest

import eval_model
import long_chain_cases as lc
import response_model as rm
import sitegrad_model as sm
import sitestep_model as st

pytestmark = pytest.mark.gpu

CASE_FORMS = pytest.mark.parametrize("name,form", lc.CASE_FORMS)
INT_FIELDS = ("n", "ncorrect", "count", "nincorrect", "confusion")
LR = 1e-6                # a step moves every element of 784 sites the same way: small enough for the weights to stay O(1)


def _ctx(name, form, tile=None):
    """a context that holds no images, sized by the case's W; the case's tile width and, for the form "map", its input map"""
    from tnml_amd.fixedl import TrainStates
    d = lc.case(name)
    ts = TrainStates(np.zeros(1, dtype=np.int32), len(d["W"]), max(d["dims"]), no_data=True, single_label=d["target"])
    ts.set_mps(d["W"])
    ts.set_option("predict_tile", lc.CASES[name]["tile"] if tile is None else tile)
    if form == "map":
        ts.set_input_map(d["imap"])
    return ts


def _src(name, form, rows=slice(None)):
    d = lc.case(name)
    if form == "phi":
        return dict(phi=d["phi"][rows])
    return dict(pixels=(d["raw"] if form == "map" else d["pixels"])[rows])


def _coefs(name, mode, rows=slice(None)):
    return {k: v[rows] for k, v in lc.coefs(name, mode).items()}


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _ratio(name, call, form, ratio):
    print("long_chain_ratio %-5s %-28s %-4s %.2e" % (name, call, form, ratio))
    return ratio


@CASE_FORMS
def test_predict_fp64_within_the_weight_bound(name, form):
    m = lc.model(name, form, "coef")
    ts = _ctx(name, form)
    w, pred = ts.predict(**_src(name, form))
    assert w.shape == m["w"].shape
    assert _ratio(name, "predict_f64", form, lc.worst(w - m["w"], m["w_bound"])) <= 1.
    assert np.array_equal(pred, lc.pred_of(name, m["w"]))       # decided: every gap is 1e4 weight bounds wide (the host file)
    w2, p2 = ts.predict(**_src(name, form))
    assert np.array_equal(w2, w) and np.array_equal(p2, pred)
    ts.close()


@CASE_FORMS
def test_predict_fp32_is_the_model_bit_for_bit(name, form):
    """N - 1 fused steps in a fixed order: an order or prefetch mistake accumulates"""
    wm, pm = lc.f32_model(name, form)
    ts = _ctx(name, form)
    w, pred = ts.predict(dtype="f32", **_src(name, form))
    print(name, form, "fp32 weights that differ from the model:", int((w != wm).sum()), "of", w.size)
    assert np.array_equal(w, wm)
    assert np.array_equal(pred, pm)
    assert _ratio(name, "predict_f32_bits_differ", form, float((w != wm).mean())) == 0.
    ts.close()


@CASE_FORMS
def test_evaluate_reports_its_own_weights(name, form):
    """the report is tests/eval_model.py on the device's own weights, the costs in the order kernels_eval.hip states; weights and pred
    are predict's bit for bit; the integers are also those of the model's weights, the decisions being decided"""
    d, m = lc.case(name), lc.model(name, form, "coef")
    ts = _ctx(name, form)
    wp, pp = ts.predict(**_src(name, form))
    rep, (w, pred) = ts.evaluate(d["labels"], want_weights=True, **_src(name, form))
    assert np.array_equal(w, wp) and np.array_equal(pred, pp)
    own = eval_model.report(w, d["labels"], d["target"])
    truth = eval_model.report(m["w"], d["labels"], d["target"])
    for f in INT_FIELDS:
        assert np.array_equal(getattr(rep, f), own[f]), f
        assert np.array_equal(getattr(rep, f), truth[f]), f
    allowed = eval_model.cost_bound(len(d["labels"]), w.shape[1])
    worst = max(abs(rep.cost - own["cost"]) / own["cost"], float((np.abs(rep.label_cost - own["label_cost"]) / np.maximum(own["label_cost"], 1e-300)).max()))
    assert _ratio(name, "evaluate_cost", form, worst / allowed) <= 1.
    assert np.array_equal(rep.label_cost, eval_model.device_order_label_cost(w, d["labels"], target=d["target"]))
    s = 0.0
    for x in rep.label_cost.tolist():
        s += x
    assert rep.cost == s and rep.cost > 0 and rep.n == len(d["labels"])
    assert ts.evaluate(d["labels"], **_src(name, form)) == rep
    ts.close()


@pytest.mark.parametrize("chosen", ["own", "given"])
@CASE_FORMS
def test_site_response_within_its_bound(name, form, chosen):
    d, r = lc.case(name), lc.response_model(name, form, chosen)
    m = lc.model(name, form, "coef")
    f = lc.feats(name, form)
    n = len(f)
    rows = np.arange(n)
    which = None if chosen == "own" else lc.given_labels(name)
    ts = _ctx(name, form)
    resp, (w, pred) = ts.site_response(which=which, want_weights=True, **_src(name, form))
    assert resp.shape == (n, len(d["W"]), 2)
    assert _ratio(name, "site_response_" + chosen, form, lc.worst(resp - r["resp"], r["bound"])) <= 1.
    wp, pp = ts.predict(**_src(name, form))
    assert np.array_equal(w, wp) and np.array_equal(pred, pp)
    label = r["label"]
    if chosen == "own" and d["target"] is None:
        assert np.array_equal(pred, label)
    # the tie on the device alone: the image's own feature at any site gives back the call's own weight of the chosen label
    tie = (f * resp).sum(axis=2)
    allowed = (np.abs(f) * r["bound"]).sum(axis=2) + 2 * rm.U * np.abs(f * resp).sum(axis=2) + m["w_bound"][rows, label][:, None]
    assert _ratio(name, "site_response_tie_" + chosen, form, lc.worst(tie - w[rows, label][:, None], allowed)) <= 1.
    ts.close()


@pytest.mark.parametrize("mode", lc.MODES)
@CASE_FORMS
def test_site_gradient_within_its_bound(name, form, mode):
    d, m = lc.case(name), lc.model(name, form, mode)
    ts = _ctx(name, form)
    grads, (w, pred) = ts.site_gradient(want_weights=True, **_coefs(name, mode), **_src(name, form))
    assert [g.shape for g in grads] == [A.shape for A in d["W"]]
    print(name, form, mode, "largest |G|", max(np.abs(g).max() for g in m["g"]))
    assert _ratio(name, "site_gradient_" + mode, form, sm.worst_ratio(grads, m["g"], m["bound"])) <= 1.
    wp, pp = ts.predict(**_src(name, form))
    assert np.array_equal(w, wp) and np.array_equal(pred, pp)
    assert _same(ts.site_gradient(**_coefs(name, mode), **_src(name, form)), grads)
    ts.close()


def _step(ts, W, state, batch, **par):
    """one step on the device and in tests/sitestep_model.py fed site_gradient() at the W before the step: W, grad_norm (the ordered
    model norm), factor, clipped and t bit for bit.  -> (the model's W after, its state, the device's report)"""
    method = par.get("method", "sgd")
    grads = ts.site_gradient(**batch)
    if state is None:
        state = st.new_state(method, sum(g.size for g in grads))
    rep = ts.gradient_step(**batch, **par)
    Wm, state, mrep = st.step(W, st.flat(grads), state, **par)
    assert mrep["applied"]
    got = ts.get_mps()
    moved = max(float(np.abs(a - b).max()) for a, b in zip(W, Wm))
    print(method, "t", rep.t, "grad_norm", rep.grad_norm, "factor", rep.factor, "clipped", rep.clipped, "largest move", moved,
          "sites that differ from the model", sum(not np.array_equal(a, b) for a, b in zip(got, Wm)))
    assert moved > 0
    assert _same(got, Wm)
    assert (rep.t, rep.grad_norm, rep.factor, rep.clipped) == (mrep["t"], mrep["grad_norm"], mrep["factor"], mrep["clipped"])
    assert rep.grad_norm == st.factor(st.ordered_sumsq(st.flat(grads)), par.get("scale", 1.), 0.)[0]
    return Wm, state, rep


def _state_equal(ts, state):
    like = ts.get_mps()
    for which in (("m", "v") if state["method"] == "adam" else ("v",)):
        assert _same(ts.step_state(which), st.unflat(state[which], like)), which


@CASE_FORMS
def test_gradient_step_is_the_model_bit_for_bit(name, form):
    """one plain SGD step on all images, then from the W it leaves two Adam steps on two batches of different sizes with a clip between
    their gradient norms, so that exactly one of them is clipped; W after every step, the state after the SGD step and after the last"""
    d = lc.case(name)
    n = len(d["labels"])
    ts = _ctx(name, form)
    batch = dict(labels=d["labels"], **_src(name, form))
    W, state, rep = _step(ts, d["W"], None, batch, method="sgd", lr=LR, scale=1. / n)
    assert rep.t == 1 and not rep.clipped and rep.factor == 1. / n
    _state_equal(ts, state)
    ts.step_reset()
    cut = 2 * n // 3
    batches = [dict(labels=d["labels"][r], **_src(name, form, r)) for r in (slice(0, cut), slice(cut, n))]
    norms = [st.factor(st.ordered_sumsq(st.flat(ts.site_gradient(**b))), 1., 0.)[0] for b in batches]
    assert max(norms) > 1.2 * min(norms), norms
    clip = float(np.sqrt(norms[0] * norms[1]))
    state, clipped = None, []
    for k, b in enumerate(batches):
        W, state, rep = _step(ts, W, state, b, method="adam", lr=LR, clip=clip)
        assert rep.t == k + 1
        clipped.append(rep.clipped)
    assert sum(clipped) == 1, (clipped, norms, clip)
    _state_equal(ts, state)
    _ratio(name, "gradient_step_sites_differ", form, 0.)
    ts.close()


@pytest.mark.parametrize("form", lc.forms("A"))
def test_chunks_tiles_and_repeats_on_case_a(form):
    """37 images in chunks of 16 (three, the last ragged) against one chunk, tile 16 and the dispatch's own against the case's 64, and
    a repeat: the same bits from predict (both types), evaluate's weights and integers, site_response and, at equal chunking,
    site_gradient; the gradient across chunkings, which sums the chunks in another order, inside the model's bound"""
    name = "A"
    d = lc.case(name)
    src = _src(name, form)
    which = lc.given_labels(name)

    def calls(ts):
        rep, (we, pe) = ts.evaluate(d["labels"], want_weights=True, **src)
        out = dict(p64=ts.predict(dtype="f64", **src), p32=ts.predict(dtype="f32", **src), ev=(we, pe) + tuple(np.asarray(getattr(rep, f)) for f in INT_FIELDS))
        ts.set_option("predict_dtype", 0)                                    # (the calls below refuse fp32)
        out["resp"] = ts.site_response(which=which, want_weights=True, **src)
        out["grad"] = ts.site_gradient(labels=d["labels"], want_weights=True, **src)
        return out, rep

    def flat(x):
        return [x] if isinstance(x, np.ndarray) else [a for part in x for a in flat(part)]

    def same_but_gradient(a, b):
        for key in ("p64", "p32", "ev", "resp"):
            assert _same(flat(a[key]), flat(b[key])), key
        assert _same(flat(a["grad"][1]), flat(b["grad"][1]))                 # weights and pred of the gradient call

    ts = _ctx(name, form)
    one, rep_one = calls(ts)
    again, rep_again = calls(ts)
    same_but_gradient(one, again)
    assert _same(one["grad"][0], again["grad"][0]) and rep_again == rep_one
    for tile in (16, 0):
        ts.set_option("predict_tile", tile)
        other, rep = calls(ts)
        same_but_gradient(one, other)
        assert _same(one["grad"][0], other["grad"][0]), tile
        assert rep == rep_one, tile
    ts.set_option("predict_tile", lc.CASES[name]["tile"])
    for key in ("predict_chunk", "response_chunk", "gradient_chunk"):
        ts.set_option(key, 16)
    cut, rep = calls(ts)
    same_but_gradient(one, cut)
    bnd = lc.model(name, form, "labels")["bound"]
    assert _ratio(name, "site_gradient_chunks_of_16", form, sm.worst_ratio(cut["grad"][0], one["grad"][0], bnd)) <= 1.
    cut2, _ = calls(ts)
    assert _same(cut["grad"][0], cut2["grad"][0])
    ts.set_option("predict_tile", 16)
    cut3, _ = calls(ts)
    same_but_gradient(one, cut3)
    assert _same(cut["grad"][0], cut3["grad"][0])
    ts.close()


@pytest.mark.parametrize("name", [k for k in lc.CASES if lc.forms(k) == ("map",)])
def test_under_the_input_map_the_bits_of_the_feature_path(name):
    """raw 28 x 28 bytes through the device map against the features the map defines, given: every call the same bits (the comparison
    with the models is made by the tests above, form "map")"""
    d = lc.case(name)
    raw, phi, labels = d["raw"], d["phi"], d["labels"]
    assert np.array_equal(phi, d["imap"].features(raw)) and phi.shape == (len(raw), d["imap"].N, 2)
    ref, ts = _ctx(name, "phi"), _ctx(name, "map")
    for dtype in ("f32", "f64"):
        a, b = ts.predict(pixels=raw, dtype=dtype), ref.predict(phi=phi, dtype=dtype)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), dtype
    assert ts.evaluate(labels, pixels=raw) == ref.evaluate(labels, phi=phi)
    a, b = ts.site_response(pixels=raw, want_weights=True), ref.site_response(phi=phi, want_weights=True)
    assert np.abs(a[0]).max() > 0 and np.array_equal(a[0], b[0]) and _same(a[1], b[1])
    a, b = ts.site_gradient(labels=labels, pixels=raw, want_weights=True), ref.site_gradient(labels=labels, phi=phi, want_weights=True)
    assert max(np.abs(g).max() for g in a[0]) > 0 and _same(a[0], b[0]) and _same(a[1], b[1])
    ra = ts.gradient_step(labels=labels, pixels=raw, method="adam", lr=LR)
    rb = ref.gradient_step(labels=labels, phi=phi, method="adam", lr=LR)
    assert (ra.t, ra.grad_norm, ra.factor) == (rb.t, rb.grad_norm, rb.factor) and ra.eval == rb.eval
    got = ts.get_mps()
    assert _same(got, ref.get_mps()) and not _same(got, d["W"])
    _ratio(name, "map_against_feature_path", "map", 0.)
    ts.close()
    ref.close()
