"""Gradient steps on the device (tnml_site_step_u8 / tnml_site_step_phi, kernels_sitestep.hip): the gradient of tnml_site_gradient_*,
then one SGD or Adam step on W where it lies.  The yardstick is tests/sitestep_model.py (checked by tests/test_sitestep_model_host.py),
fed the gradient that site_gradient() returns at the W before the step under the same options: every comparison of W, of the state
and of grad_norm and factor is bit for bit.  Contexts are data-less unless the test is about a training context."""
import numpy as np
import pytest

import sitegrad_model as sm
import sitestep_model as st
from conftest import make_problem

pytestmark = pytest.mark.gpu


def _dataless(W, single_label=None, **kw):
    from tnml_amd.fixedl import TrainStates
    maxm = max(max(A.shape[0], A.shape[2]) for A in W)
    ts = TrainStates(np.zeros(1, dtype=np.int32), len(W), maxm, no_data=True, single_label=single_label, **kw)
    ts.set_mps(W)
    return ts


def _plain(W):
    return [A if A.ndim == 3 else A[..., 0] * 3.0 for A in W]


def _src(case, form, rows=slice(None)):
    return dict(phi=case["phi"][rows]) if form == "phi" else dict(pixels=case["pixels"][rows])


def _coefs(case, mode, target=None, rows=slice(None)):
    return dict(labels=case["labels"][rows]) if mode == "labels" else dict(coef=case["coef"][rows, :1 if target is not None else 10])


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _step(ts, W, state, batch, **par):
    """one step on the device and in the model, compared: W, grad_norm, factor, clipped, t.  W: the model's W before the step (= the
    context's); state: the model's state, or None before the first step.  -> (the model's W after, its state, the device's report)"""
    method = par.get("method", "sgd")
    grads = ts.site_gradient(**batch)
    if state is None:
        state = st.new_state(method, sum(g.size for g in grads))
    rep = ts.gradient_step(**batch, **par)
    Wm, state, mrep = st.step(W, st.flat(grads), state, **par)
    assert mrep["applied"]
    got = ts.get_mps()
    assert [a.shape for a in got] == [a.shape for a in W]
    worst = max(float(np.abs(a - b).max()) for a, b in zip(got, Wm))
    moved = max(float(np.abs(a - b).max()) for a, b in zip(W, Wm))
    print(method, "t", rep.t, "grad_norm", rep.grad_norm, "factor", rep.factor, "clipped", rep.clipped, "largest move", moved, "largest |device - model|", worst)
    assert moved > 0
    assert _same(got, Wm)
    assert (rep.t, rep.grad_norm, rep.factor, rep.clipped) == (mrep["t"], mrep["grad_norm"], mrep["factor"], mrep["clipped"])
    return Wm, state, rep


def _state_equal(ts, state):
    like = ts.get_mps()
    for which in (("m", "v") if state["method"] == "adam" else ("v",)):
        assert _same(ts.step_state(which), st.unflat(state[which], like)), which


CASES = [("small", 4, 2), ("small", 4, 3), ("small", 12, 5), ("small", 17, 6)] + [("odd", k, n) for k in range(len(sm.DIMS)) for n in (1, 37, 150)]


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("kind,a,b", CASES)
def test_plain_sgd_is_the_model_bit_for_bit(kind, a, b, form, mode):
    """mu = 0: A - lr f g.  odd_case(0) has less than one norm block, (2) and (3) span many with a ragged last one, (3) has the Label
    site at 512 x 2 x 511 x 10; sites of two elements and of millions, every update workgroup ragged or full"""
    case = sm.small_case(a, b) if kind == "small" else sm.odd_case(a, b)
    ts = _dataless(case["W"])
    batch = dict(_coefs(case, mode), **_src(case, form))
    n = len(case["labels"])
    Wm, state, rep = _step(ts, case["W"], None, batch, method="sgd", lr=1e-3, scale=1. / n)
    assert rep.t == 1 and not rep.clipped and rep.factor == 1. / n
    _state_equal(ts, state)
    ts.close()


def _three_batches(case):
    """three different batches of different sizes (so that their gradient norms differ) and a clip between the first two norms at W0"""
    rows = [slice(0, 40), slice(40, 45), slice(45, 70)]
    return [dict(labels=case["labels"][r], phi=case["phi"][r]) for r in rows]


@pytest.mark.parametrize("method,par", [("sgd", dict(momentum=0.9)), ("adam", dict(beta1=0.9, beta2=0.999, eps=1e-8)), ("adam", dict(beta1=0.5, beta2=0.9, eps=1e-3))])
@pytest.mark.parametrize("which", ["small", "odd1"])
def test_three_steps_with_state_and_clipping(which, method, par):
    """momentum and Adam carry state from step to step; clip is chosen from the model so that at least one step is clipped and one is
    not; W after every step, m and v after the last"""
    case = sm.small_case(12, 5) if which == "small" else sm.odd_case(1, 150)
    batches = _three_batches(case)
    ts = _dataless(case["W"])
    norms = [st.factor(st.ordered_sumsq(st.flat(ts.site_gradient(**b))), 1., 0.)[0] for b in batches[:2]]
    assert max(norms) > 1.5 * min(norms), norms
    clip = float(np.sqrt(norms[0] * norms[1]))
    W, state, clipped = case["W"], None, []
    for k, b in enumerate(batches):
        W, state, rep = _step(ts, W, state, b, method=method, lr=1e-3, clip=clip, **par)
        assert rep.t == k + 1
        clipped.append(rep.clipped)
    assert any(clipped) and not all(clipped), clipped
    _state_equal(ts, state)
    ts.close()


@pytest.mark.parametrize("method", ["sgd", "adam"])
@pytest.mark.parametrize("N", [6, 12])
def test_per_label_variant(N, method):
    """TNML_MODE_SINGLE: one output, site 1 plays the Label site; labels mode (y_n = [label_n == 3]) then coef mode on the same state"""
    base = sm.small_case(N, 5)
    case = dict(base, W=_plain(base["W"]))
    ts = _dataless(case["W"], single_label=3)
    want = ts.evaluate(case["labels"], phi=case["phi"])
    W, state, rep = _step(ts, case["W"], None, dict(labels=case["labels"], phi=case["phi"]), method=method, lr=1e-3, momentum=0.5)
    assert rep.eval == want and want.cost > 0
    W, state, rep = _step(ts, W, state, dict(coef=case["coef"][:, :1], pixels=case["pixels"]), method=method, lr=1e-3, momentum=0.5)
    assert rep.t == 2 and rep.eval.n == 70 and rep.eval.cost == 0
    _state_equal(ts, state)
    ts.close()


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_under_an_input_map(method):
    """raw bytes through the device input map, from_imglen(8, 4): the bits of the feature form on the features the map defines"""
    from tnml_amd import synth
    from tnml_amd.input_map import InputMap
    m = InputMap.from_imglen(8, 4, "normal")
    rng = np.random.default_rng(8)
    raw = rng.integers(0, 256, size=(20, m.S)).astype(np.uint8)
    labels = rng.integers(0, 10, size=20).astype(np.int32)
    W0 = synth.random_mps(m.N, 6, seed=4)
    ref = _dataless(W0)
    ts = _dataless(W0)
    ts.set_input_map(m)
    W, state = W0, None
    for _ in range(2):
        W, state, rep = _step(ts, W, state, dict(labels=labels, pixels=raw), method=method, lr=1e-3, momentum=0.9)
        rep_ref = ref.gradient_step(labels=labels, phi=m.features(raw), method=method, lr=1e-3, momentum=0.9)
        assert _same(ref.get_mps(), W)
        assert (rep.grad_norm, rep.factor, rep.t) == (rep_ref.grad_norm, rep_ref.factor, rep_ref.t) and rep.eval == rep_ref.eval
    ts.close()
    ref.close()


@pytest.mark.parametrize("chunk", [64, 50])
def test_several_chunks_tiles_and_repeats(chunk):
    """n = 150 in chunks: the model fed site_gradient() under the same chunk; identical across predict_tile and on a repeat from the
    same start"""
    case = sm.odd_case(0, 150)
    batch = dict(labels=case["labels"], phi=case["phi"])
    par = dict(method="adam", lr=1e-3)
    ts = _dataless(case["W"])
    ts.set_option("gradient_chunk", chunk)
    W1, state, rep = _step(ts, case["W"], None, batch, **par)
    for tile in (16, 32, 64, 0):
        ts.set_mps(case["W"])
        ts.step_reset()
        ts.set_option("predict_tile", tile)
        again = ts.gradient_step(**batch, **par)
        assert _same(ts.get_mps(), W1), tile
        assert (again.t, again.grad_norm, again.factor) == (1, rep.grad_norm, rep.factor) and again.eval == rep.eval
        _state_equal(ts, state)
    ts.close()


@pytest.mark.parametrize("form", ["phi", "u8"])
def test_report(form):
    """labels mode: eval is evaluate()'s report of the batch at the W before the step under predict_chunk = gradient_chunk, every field
    bit for bit (three chunks, the last ragged); coef mode: zero but for n"""
    case = sm.small_case(12, 5)
    ts = _dataless(case["W"])
    ts.set_option("gradient_chunk", 32)
    ts.set_option("predict_chunk", 32)
    want = ts.evaluate(case["labels"], **_src(case, form))
    rep = ts.gradient_step(labels=case["labels"], method="sgd", lr=1e-3, **_src(case, form))
    assert type(rep.eval) is type(want) and rep.eval == want and want.cost > 0 and want.n == 70
    for f in want.FIELDS:
        assert np.array_equal(getattr(rep.eval, f), getattr(want, f)), f
    after = ts.evaluate(case["labels"], **_src(case, form))
    assert after.cost != want.cost                               # (the report is the W before the step, not after)
    rep = ts.gradient_step(coef=case["coef"], method="sgd", lr=1e-3, **_src(case, form))
    assert rep.t == 2 and rep.eval.n == 70 and rep.eval.ncorrect == 0 and rep.eval.cost == 0
    assert not rep.eval.label_cost.any() and not rep.eval.count.any() and not rep.eval.nincorrect.any() and not rep.eval.confusion.any()
    ts.close()


def test_state_lifetime():
    from tnml_amd import hostlib
    from tnml_amd.fixedl import TnmlError
    from tnml_amd.input_map import InputMap
    case = sm.small_case(12, 5)
    b1 = dict(labels=case["labels"][:30], phi=case["phi"][:30])
    b2 = dict(labels=case["labels"][30:], pixels=case["pixels"][30:])
    ts = _dataless(case["W"])
    W, state, _ = _step(ts, case["W"], None, b1, method="adam", lr=1e-3)
    # the state is no part of the gradient workspace: another chunk, and an input map set and cleared, release that and not the state
    with_ws = ts.device_bytes()
    ts.set_option("gradient_chunk", 16)
    ts.set_input_map(InputMap(6, 8, 2, 0, 0, 3, 4, hostlib.feature_table("normal", 1.0, 2), feature="normal"))
    ts.set_input_map(None)
    assert ts.device_bytes() < with_ws
    _state_equal(ts, state)
    W, state, rep = _step(ts, W, state, b2, method="adam", lr=2e-3, beta1=0.8)     # hyper-parameters may change from call to call
    assert rep.t == 2
    _state_equal(ts, state)
    # another method without a reset
    with pytest.raises(TnmlError, match="made for method adam.*tnml_site_step_reset"):
        ts.gradient_step(method="sgd", lr=1e-3, **b1)
    # other bond dimensions on the bond between sites 3 and 4
    ts.set_site(3, W[2][:, :, :-1])
    ts.set_site(4, W[3][:-1])
    with pytest.raises(TnmlError, match=r"site 3 .*tnml_site_step_reset"):
        ts.gradient_step(method="adam", lr=1e-3, **b1)
    before = ts.device_bytes()
    ts.step_reset()
    assert ts.device_bytes() < before
    with pytest.raises(TnmlError, match="no step has been taken"):
        ts.step_state("v")
    W2, state2, rep = _step(ts, ts.get_mps(), None, b1, method="sgd", lr=1e-3)
    assert rep.t == 1
    _state_equal(ts, state2)
    with pytest.raises(TnmlError, match='keeps no array "m"'):
        ts.step_state("m")
    ts.close()


def test_a_gradient_out_of_range_changes_nothing():
    """coefficients of 1e200 are finite, the sum of squares of the gradient is not: the call fails, W, m, v and t stay bit for bit, the
    next ordinary step is the model's"""
    from tnml_amd.fixedl import TnmlError
    case = sm.small_case(12, 5)
    ts = _dataless(case["W"])
    batch = dict(labels=case["labels"], phi=case["phi"])
    W, state, _ = _step(ts, case["W"], None, batch, method="adam", lr=1e-3)
    m0, v0 = ts.step_state("m"), ts.step_state("v")
    with pytest.raises(TnmlError, match="out of range .*norm"):
        ts.gradient_step(coef=np.full((70, 10), 1e200), phi=case["phi"], method="adam", lr=1e-3)
    assert _same(ts.get_mps(), W) and _same(ts.step_state("m"), m0) and _same(ts.step_state("v"), v0)
    W, state, rep = _step(ts, W, state, batch, method="adam", lr=1e-3)
    assert rep.t == 2
    _state_equal(ts, state)
    ts.close()


def _same_report(a, b):
    for key in a:
        if key == "cg":
            assert a["cg"] == b["cg"]
        else:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


def test_a_step_leaves_a_training_context_as_set_mps_does():
    """a training context with environments and a bond set takes a step; a twin gets the model's W by set_mps(); tnml_env_init and one
    bond update on both give bit-identical reports"""
    from tnml_amd.fixedl import TrainStates
    sweep = (4, 2, 1e-10, 3, 1e-3, 1e-10)
    pixels, labels, phi, W0 = make_problem(12, 60, 4, 3, pixel_boost=200.0)
    others = make_problem(12, 33, 4, 11, pixel_boost=200.0)
    batch = dict(labels=np.asarray(others[1], dtype=np.int32), phi=others[2])
    ts = TrainStates(labels, 12, 4, phi=phi)
    ts.set_mps(W0)
    ts.init()
    ts.bond_update(1, 1, *sweep)
    W1 = ts.get_mps()
    Wm, state, rep = _step(ts, W1, None, batch, method="adam", lr=1e-3)
    twin = TrainStates(labels, 12, 4, phi=phi)
    twin.set_mps(Wm)
    reports = []
    for ctx in (ts, twin):
        ctx.init()
        reports.append(ctx.bond_update(1, 1, *sweep))
        ctx.close()
    _same_report(reports[0], reports[1])


def test_refusals():
    from tnml_amd.fixedl import TnmlError, TrainStates
    case = sm.small_case(12, 5)
    W, phi, labels, coef = case["W"], case["phi"], case["labels"], case["coef"]
    ts = _dataless(W)
    fresh = ts.device_bytes()
    ok = dict(method="adam", lr=1e-3)
    for match, kw in (("exactly one of labels and coef", dict(labels=labels, coef=coef)), ("exactly one of labels and coef", dict()),
                      ("image 41", dict(labels=np.where(np.arange(70) == 41, 10, labels).astype(np.int32))),
                      ("image 57 is not finite", dict(coef=np.where(np.arange(70)[:, None] == 57, np.nan, coef)))):
        with pytest.raises(TnmlError, match=match):
            ts.gradient_step(phi=phi, **kw, **ok)
    for match, par in (("lr", dict(method="sgd", lr=0.)), ("lr", dict(method="sgd", lr=np.inf)), ("beta2", dict(method="adam", lr=1e-3, beta2=1.)),
                       ("beta1", dict(method="adam", lr=1e-3, beta1=-0.1)), ("eps", dict(method="adam", lr=1e-3, eps=0.)),
                       ("scale", dict(method="sgd", lr=1e-3, scale=np.nan)), ("scale", dict(method="sgd", lr=1e-3, scale=0.)),
                       ("momentum", dict(method="sgd", lr=1e-3, momentum=1.)), ("clip", dict(method="sgd", lr=1e-3, clip=-1.))):
        with pytest.raises(TnmlError, match=match):
            ts.gradient_step(labels=labels, phi=phi, **par)
    import ctypes as C
    from tnml_amd import lib as _lib
    x = np.ascontiguousarray(phi)
    assert ts._L.tnml_site_step_phi(ts._h, 70, _lib.dptr(x), labels.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None) != 0
    assert "null argument" in ts._L.tnml_last_error(ts._h).decode()
    ts.set_option("predict_dtype", 1)
    with pytest.raises(TnmlError, match="predict_dtype"):
        ts.gradient_step(labels=labels, phi=phi, **ok)
    ts.set_option("predict_dtype", 0)
    rep = ts.gradient_step(labels=labels[:0], phi=phi[:0], **ok)            # n = 0: no step, a zeroed report
    assert (rep.t, rep.grad_norm, rep.factor, rep.clipped, rep.eval.n) == (0, 0., 0., False, 0)
    assert _same(ts.get_mps(), W) and ts.device_bytes() == fresh        # nothing of the above took a step, made a state or a workspace
    rep = ts.gradient_step(labels=labels, phi=phi, **ok)
    assert rep.t == 1
    ts.close()
    # a context of a multi-rank run: refused before any collective could be entered
    r0 = _dataless(W, rank=0, nranks=2, NT_total=2)
    with pytest.raises(TnmlError, match="rank 0 of 2"):
        r0.gradient_step(labels=labels, phi=phi, **ok)
    assert _same(r0.get_mps(), W)
    r0.close()
    # held-out pairs: the attached context refuses as every streamed call does, the training context as tnml_set_site does
    pixels, tl, tphi, TW = make_problem(12, 60, 4, 3, pixel_boost=200.0)
    train = TrainStates(tl, 12, 4, phi=tphi)
    train.set_mps(TW)
    train.init()
    held = make_problem(12, 40, 4, 17, pixel_boost=200.0)
    hs = TrainStates(held[1], 12, 4, phi=held[2])
    train.attach_heldout(hs)
    with pytest.raises(TnmlError, match="attached as a held-out set"):
        hs.gradient_step(labels=labels, phi=phi, **ok)
    with pytest.raises(TnmlError, match="a held-out context is attached to this context"):
        train.gradient_step(labels=labels, phi=phi, **ok)
    assert _same(train.get_mps(), TW)
    train.close()
    hs.close()


def _formula(W, chunk, nl=10):
    """the workspace of tnml_site_gradient_* for features as include/tnml.h states it"""
    N = len(W)
    C = (chunk + 63) // 64 * 64
    B = 32 + sum((A.shape[2] + 15) // 16 * 16 for A in W[:-1])
    E = sum(A.size for A in W)
    return 16 * N + 16 * nl * C + 8 * C + 4 * (N + 2) + 8 * (N + 1) + 4 * (N + nl) + 8 * E + 16 * B * C + 32 * N * C


def _state_formula(W, method):
    """the optimiser state as include/tnml.h states it"""
    E, N = sum(A.size for A in W), len(W)
    return 8 * (2 if method == "adam" else 1) * E + 8 * -(-E // 65536) + 4 * (N + 1) + 64 + 1040


@pytest.mark.parametrize("method", ["sgd", "adam"])
@pytest.mark.parametrize("mode", ["labels", "coef"])
def test_launches_and_bytes(mode, method):
    """a call with k chunks: k launches each of site_bwd and site_grad, k of eval_tally in the labels mode alone, at most three of the
    new classes; tnml_device_bytes grows by the gradient workspace and the state's formula, and reset gives the state back"""
    case = sm.odd_case(1, 150)
    W = case["W"]
    ts = _dataless(W)
    ts.set_option("gradient_chunk", 64)
    before = ts.device_bytes()
    ts.profile(True)
    ts.profile_reset()
    ts.gradient_step(phi=case["phi"], method=method, lr=1e-3, **_coefs(case, mode))
    prof = ts.profile_read()
    ts.profile(False)
    assert prof["site_bwd"][0] == 3 and prof["site_grad"][0] == 3, prof
    assert prof["eval_tally"][0] == (3 if mode == "labels" else 0), prof
    assert 1 <= prof["site_step"][0] and 1 <= prof["step_norm"][0] and prof["site_step"][0] + prof["step_norm"][0] <= 3, prof
    assert prof["chain"][0] == 0 and prof["site_resp"][0] == 0, prof
    assert ts.device_bytes() - before == _formula(W, 64) + _state_formula(W, method)
    ts.gradient_step(phi=case["phi"], method=method, lr=1e-3, **_coefs(case, mode))
    assert ts.device_bytes() - before == _formula(W, 64) + _state_formula(W, method)
    ts.step_reset()
    assert ts.device_bytes() - before == _formula(W, 64)
    ts.close()


def test_twenty_adam_steps_lower_the_cost():
    """DESCENT of tests/sitestep_model.py: the lr found on the CPU, where the model's cost falls to 0.39 of its start in twenty steps
    (tests/test_sitestep_model_host.py asserts below half); here the cost evaluate() reports must end below its start"""
    d = st.DESCENT
    case = sm.small_case(*d["case"])
    phi, labels = case["phi"][:d["images"]], case["labels"][:d["images"]]
    ts = _dataless(case["W"])
    start = ts.evaluate(labels, phi=phi).cost
    costs = []
    for k in range(d["steps"]):
        rep = ts.gradient_step(labels=labels, phi=phi, method="adam", lr=d["lr"])
        assert rep.t == k + 1
        costs.append(rep.eval.cost)
    end = ts.evaluate(labels, phi=phi).cost
    print("start", start, "reported before each step / start", [round(c / start, 3) for c in costs], "end / start", end / start)
    assert costs[0] == start and end < start
    ts.close()
