"""Streamed evaluation (tnml_evaluate_u8 / tnml_evaluate_phi, kernels_eval.hip): tnml_predict_* on labelled images plus one tally launch
per chunk.  Truth is tests/eval_model.py applied to the oracle's per-image full contraction (toverlap); the problems are those of
tests/test_predict_gpu.py, whose top-two gaps are large enough for predictions to be compared exactly.  Contexts are data-less unless
the test is about a training context."""
import ctypes as C
import functools

import numpy as np
import pytest

import eval_model
from conftest import make_problem

pytestmark = pytest.mark.gpu

C_TOL = 1e-11                        # the "costs" column of the fp64 row of test_gpu_parity.TOL, as tests/test_predict_gpu.py
INT_FIELDS = ("n", "ncorrect", "count", "nincorrect", "confusion")

DIMS = {1: [1, 2, 120, 97, 64, 60, 61, 128, 33, 2, 1],       # a 64-wide tile
        3: [1, 2, 16, 512, 511, 130, 64, 2, 1]}              # bond 512: the parked vector in global scratch, the Label site at its largest


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


def _toverlap(phi, labels, W):
    from oracle import pyoracle
    o = pyoracle.Oracle(phi, labels, W)
    return np.stack([o.toverlap(i) for i in range(len(labels))])


def _label_sets(labels, truth):
    """the problem's labels (every label 0..9 occurs), and labels equal to the oracle's prediction on every second image"""
    labels = np.asarray(labels, dtype=np.int32)
    assert set(labels.tolist()) == set(range(10))
    half = labels.copy()
    half[::2] = np.abs(truth).argmax(axis=1)[::2]
    return {"given": labels, "half_right": half}


@functools.lru_cache(maxsize=None)
def _small(N, m):
    """70 images: (pixels, boosted features, W, truth on the boosted features, truth on the byte feature map, the two label sets)"""
    from oracle import pyoracle
    pixels, labels, phi, W = make_problem(N, 70, m, 3, pixel_boost=200.0)
    t_phi = _toverlap(phi, labels, W)
    return pixels, phi, W, t_phi, _toverlap(pyoracle.features_series(pixels), labels, W), _label_sets(labels, t_phi)


@functools.lru_cache(maxsize=None)
def _odd(k):
    """40 images on the bond dimensions DIMS[k]"""
    from oracle import pyoracle
    dims = DIMS[k]
    N = len(dims) - 1
    pixels, labels, phi, _ = make_problem(N, 40, 2, 5, pixel_boost=200.0)
    W = _mps_with_dims(dims, 11)
    t_phi = _toverlap(phi, labels, W)
    return pixels, phi, W, t_phi, _toverlap(pyoracle.features_series(pixels), labels, W), _label_sets(labels, t_phi)


def _ints_equal(rep, exp):
    for f in INT_FIELDS:
        assert np.array_equal(getattr(rep, f), exp[f]), (f, getattr(rep, f), exp[f])


def _costs_within(rep, exp, rel):
    """cost and label_cost of `rep` against those of `exp` (a model dict or another report), relative to the quantity itself"""
    ec, el = (exp["cost"], exp["label_cost"]) if isinstance(exp, dict) else (exp.cost, exp.label_cost)
    print("cost", rep.cost, "expected", ec, "rel", abs(rep.cost - ec) / max(ec, 1e-300), "allowed", rel)
    assert abs(rep.cost - ec) <= rel * ec, (rep.cost, ec)
    assert np.all(np.abs(rep.label_cost - el) <= rel * np.asarray(el)), (rep.label_cost, el)


def _check_against_oracle(ts, labels, truth, target=None, **images):
    """one evaluate call: weights / pred are predict's, integers the model's on the oracle's weights, costs within C_TOL of them, and
    within the derived bound of the model on the call's own weights; the cost is the sum of label_cost in index order"""
    w_p, p_p = ts.predict(**images)
    rep, (w, pred) = ts.evaluate(labels, want_weights=True, **images)
    assert np.array_equal(w, w_p) and np.array_equal(pred, p_p)
    exp = eval_model.report(truth, labels, target)
    _ints_equal(rep, exp)
    _costs_within(rep, exp, C_TOL)
    own = eval_model.report(w, labels, target)
    _ints_equal(rep, own)
    _costs_within(rep, own, eval_model.cost_bound(len(labels), w.shape[1]))
    s = 0.0
    for x in rep.label_cost.tolist():
        s += x
    assert rep.cost == s
    assert rep.n == len(labels) and rep.ncorrect == rep.n - rep.nincorrect.sum() and rep.confusion.sum() == rep.n
    return rep, w


@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("N,m", [(12, 4), (4, 2), (17, 6)])
def test_evaluate_matches_the_model_on_the_oracle(N, m, form):
    pixels, phi, W, t_phi, t_u8, sets = _small(N, m)
    ts = _dataless(N, m, W)
    for name, labels in sets.items():
        images = dict(phi=phi) if form == "phi" else dict(pixels=pixels)
        rep, _ = _check_against_oracle(ts, labels, t_phi if form == "phi" else t_u8, **images)
        if name == "half_right" and form == "phi":
            assert 35 <= rep.ncorrect < 70 and np.trace(rep.confusion) == rep.ncorrect
            assert (rep.confusion - np.diag(np.diag(rep.confusion))).sum() == 70 - rep.ncorrect > 0
    ts.close()


@pytest.mark.parametrize("form", ["phi", "u8"])
@pytest.mark.parametrize("k", sorted(DIMS))
def test_evaluate_at_wide_tiles_and_bond_512(k, form):
    pixels, phi, W, t_phi, t_u8, sets = _odd(k)
    ts = _dataless(len(W), max(DIMS[k]), W)
    for labels in sets.values():
        images = dict(phi=phi) if form == "phi" else dict(pixels=pixels)
        _check_against_oracle(ts, labels, t_phi if form == "phi" else t_u8, **images)
    ts.close()


def test_cost_follows_the_summation_order_of_the_kernel_header():
    """the order kernels_eval.hip states, restated in eval_model.device_order_label_cost: the same bits, one chunk and five"""
    pixels, phi, W, _, _, sets = _small(12, 4)
    ts = _dataless(12, 4, W)
    for chunk in (8192, 16):
        ts.set_option("predict_chunk", chunk)
        rep, (w, _) = ts.evaluate(sets["given"], phi=phi, want_weights=True)
        assert np.array_equal(rep.label_cost, eval_model.device_order_label_cost(w, sets["given"], chunk=chunk)), chunk
    ts.close()


@pytest.mark.parametrize("chunk", [16, 37])
def test_chunking_changes_neither_integers_nor_weights(chunk):
    """70 images in chunks of 16 (five, the last one ragged) and of 37 against one chunk"""
    pixels, phi, W, _, _, sets = _small(12, 4)
    labels = sets["half_right"]
    one, cut = _dataless(12, 4, W), _dataless(12, 4, W)
    cut.set_option("predict_chunk", chunk)
    cut.profile(True)
    for images in (dict(phi=phi), dict(pixels=pixels)):
        r1, (w1, p1) = one.evaluate(labels, want_weights=True, **images)
        cut.profile_reset()
        r2, (w2, p2) = cut.evaluate(labels, want_weights=True, **images)
        prof = cut.profile_read()
        assert prof["chain"][0] == prof["eval_tally"][0] == -(-70 // chunk), prof
        assert np.array_equal(w1, w2) and np.array_equal(p1, p2)
        _ints_equal(r2, {f: getattr(r1, f) for f in INT_FIELDS})
        _costs_within(r2, r1, eval_model.cost_bound(70, 10))
    one.close()
    cut.close()


def test_report_is_independent_of_the_tile_and_repeatable():
    pixels, phi, W, _, _, sets = _odd(1)
    ts = _dataless(len(W), max(DIMS[1]), W)
    labels = sets["half_right"]
    first = ts.evaluate(labels, phi=phi)
    assert ts.evaluate(labels, phi=phi) == first                # (EvalReport.__eq__: every field, bit for bit)
    for tile in (16, 32, 64):
        ts.set_option("predict_tile", tile)
        assert ts.evaluate(labels, phi=phi) == first, tile
        assert ts.evaluate(labels, phi=phi) == first, tile
    ts.set_option("predict_tile", 0)
    ts.set_option("predict_chunk", 16)
    r = ts.evaluate(labels, phi=phi)
    _ints_equal(r, {f: getattr(first, f) for f in INT_FIELDS})
    ts.close()


def test_evaluate_per_label_variant():
    """TNML_MODE_SINGLE: targets [label == 3], pred = [f > 1/2], confusion columns 2..9 zero, label_cost bucketed by the true label"""
    from oracle import pyoracle
    from tnml_amd import synth
    N, NT, m = 12, 60, 4
    labels = synth.synthetic_labels(NT, seed=3, per_label=NT // 10)
    pixels = synth.synthetic_images(N, labels, seed=3)
    phi = pyoracle.features_single(pixels, True).copy()
    phi[..., 1] *= 300.0
    W = synth.random_mps(N, m, seed=10)
    W[N // 2 - 1] = W[N // 2 - 1][..., 0] * 3.0            # plain MPS: no Label index
    f = np.ones((NT, 1))
    for j, A in enumerate(W):
        f = np.einsum("na,nab->nb", f, np.einsum("ns,asb->nab", phi[:, j, :], A))
    print("closest to 1/2", np.abs(f[:, 0] - 0.5).min(), "predicted 1:", int((f[:, 0] > 0.5).sum()))
    ts = _dataless(N, m, W, single_label=3)
    ts.set_option("predict_chunk", 16)
    rep, w = _check_against_oracle(ts, np.asarray(labels, dtype=np.int32), f, target=3, phi=phi)
    assert w.shape == (NT, 1)
    assert not rep.confusion[:, 2:].any()
    assert np.array_equal(rep.confusion[:, 1], [int(((labels == l) & (f[:, 0] > 0.5)).sum()) for l in range(10)])
    per = (w[:, 0] - (labels == 3)) ** 2
    np.testing.assert_allclose(rep.label_cost, [per[labels == l].sum() for l in range(10)], rtol=1e-13)
    assert np.array_equal(rep.label_cost, eval_model.device_order_label_cost(w, labels, target=3, chunk=16))
    ts.close()


def test_evaluate_fp32():
    """predict_dtype = 1: the weights are predict's fp32 results widened, the integers follow them, the cost is formed from them in fp64"""
    pixels, phi, W, _, _, sets = _small(12, 4)
    ts = _dataless(12, 4, W)
    for images in (dict(phi=phi), dict(pixels=pixels)):
        w32, p32 = ts.predict(dtype="f32", **images)
        assert np.array_equal(w32, w32.astype(np.float32).astype(np.float64))
        for labels in sets.values():
            rep, (w, pred) = ts.evaluate(labels, dtype="f32", want_weights=True, **images)
            assert np.array_equal(w, w32) and np.array_equal(pred, p32)
            own = eval_model.report(w, labels)
            assert np.array_equal(pred, eval_model.predictions(w))
            _ints_equal(rep, own)
            _costs_within(rep, own, eval_model.cost_bound(70, 10))
    w64 = ts.predict(dtype="f64", phi=phi)[0]
    assert not np.array_equal(w64, w32)
    ts.close()


def test_evaluate_under_an_input_map():
    """raw 28 x 28 bytes through the device map against the host's features of the same images: every field equal"""
    from tnml_amd.input_map import InputMap
    m = InputMap.from_imglen(28, 14, "normal")
    assert m.N == 196
    rng = np.random.default_rng(8)
    raw = rng.integers(0, 256, (20, m.S), dtype=np.uint8)
    labels = (np.arange(20) % 10).astype(np.int32)
    W = _mps_with_dims([1, 2] + [3] * (m.N - 3) + [2, 1], 4)
    ts = _dataless(m.N, 3, W)
    ts.set_input_map(m)
    a, (wa, pa) = ts.evaluate(labels, pixels=raw, want_weights=True)
    b, (wb, pb) = ts.evaluate(labels, phi=m.features(raw), want_weights=True)
    assert a == b and np.array_equal(wa, wb) and np.array_equal(pa, pb)
    assert a.n == 20 and np.array_equal(a.count, [2] * 10) and np.isfinite(wa).all()
    assert len({tuple(r) for r in wa.tolist()}) == 20            # every image has weights of its own: a misplaced image would show
    _ints_equal(a, eval_model.report(wa, labels))
    ts.close()


def test_without_per_image_output_only_the_report_comes_back():
    pixels, phi, W, _, _, sets = _small(12, 4)
    ts = _dataless(12, 4, W)
    ts.set_option("predict_chunk", 16)
    asked, _ = ts.evaluate(sets["given"], phi=phi, want_weights=True)
    ts.profile(True)
    ts.profile_reset()
    plain = ts.evaluate(sets["given"], phi=phi)
    prof = ts.profile_read()
    ts.profile(False)
    assert plain == asked
    assert prof["chain"][0] == 5 and prof["eval_tally"][0] == 5, prof
    assert prof["fgemm_shift"][0] == 0 and prof["fgemm_fwd"][0] == 0 and prof["labeldot"][0] == 0, prof
    ts.close()


def _filled():
    from tnml_amd import lib
    r = lib.EvalReport()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    return r


def _raw_call(ts, phi, labels, rep):
    """tnml_evaluate_phi as C sees it; labels may be None (NULL)"""
    from tnml_amd import lib
    x = np.ascontiguousarray(phi, dtype=np.float64)
    lp = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    rc = ts._L.tnml_evaluate_phi(ts._h, len(x), lib.dptr(x), lp, C.byref(rep) if rep is not None else None, None, None)
    return rc, ts._L.tnml_last_error(ts._h).decode()


def _untouched(rep):
    return bytes(rep) == bytes(_filled())


def test_refusals_leave_the_report_and_the_context_alone():
    from tnml_amd.fixedl import TnmlError, TrainStates
    pixels, phi, W, _, _, sets = _small(12, 4)
    labels = sets["given"]
    ts = _dataless(12, 4, W)
    good = ts.evaluate(labels, phi=phi)
    for bad, at in ((10, 7), (-1, 69)):
        lab = labels.copy()
        lab[at] = bad
        rep = _filled()
        rc, msg = _raw_call(ts, phi, lab, rep)
        assert rc != 0 and "label %d of image %d out of range" % (bad, at) in msg and "tnml_evaluate_phi" in msg, msg
        assert _untouched(rep)
    rep = _filled()
    rc, msg = _raw_call(ts, phi, None, rep)
    assert rc != 0 and "null argument" in msg and _untouched(rep)
    rc, msg = _raw_call(ts, phi, labels, None)
    assert rc != 0 and "null argument" in msg
    assert ts.evaluate(labels, phi=phi) == good                 # the context is usable after each of them
    ts.close()
    # bond 513 under fp64: predict's refusal, in predict's words
    Wb = _mps_with_dims([1, 2, 16, 513, 16, 2, 1], 11)
    tb = _dataless(len(Wb), 513, Wb)
    rep = _filled()
    rc, msg = _raw_call(tb, np.zeros((3, len(Wb), 2)), np.zeros(3, dtype=np.int32), rep)
    assert rc != 0 and "the chain kernel serves bond dimensions up to 512: use tnml_classify" in msg and _untouched(rep)
    with pytest.raises(TnmlError, match="tnml_classify"):
        tb.predict(phi=np.zeros((3, len(Wb), 2)))
    tb.close()
    # a bond update in flight, and a context attached as a held-out set
    px, lab, ph, Wt = make_problem(12, 60, 4, 3, pixel_boost=200.0)
    sweep = (4, 2, 1e-10, 3, 1e-3, 1e-10)
    tr = TrainStates(lab, 12, 4, phi=ph)
    tr.set_mps(Wt)
    tr.init()
    tr.bond_update_begin(1, 1, *sweep)
    rep = _filled()
    rc, msg = _raw_call(tr, phi, labels, rep)
    assert rc != 0 and "bond update is in flight" in msg and _untouched(rep)
    tr.bond_update_end()
    tr.evaluate(labels, phi=phi)
    tr.close()
    tr = TrainStates(lab, 12, 4, phi=ph)
    tr.set_mps(Wt)
    tr.init()
    held = make_problem(12, 40, 4, 17, pixel_boost=200.0)
    hs = TrainStates(held[1], 12, 4, phi=held[2])
    tr.attach_heldout(hs)
    rep = _filled()
    rc, msg = _raw_call(hs, phi, labels, rep)
    assert rc != 0 and "attached as a held-out set" in msg and _untouched(rep)
    tr.detach_heldout()
    hs.set_mps(Wt)
    assert hs.evaluate(labels, phi=phi).n == 70
    tr.close()
    hs.close()


def test_no_images_give_a_zeroed_report():
    pixels, phi, W, _, _, sets = _small(12, 4)
    ts = _dataless(12, 4, W)
    rep = _filled()
    rc, msg = _raw_call(ts, phi[:0], sets["given"][:0], rep)
    assert rc == 0, msg
    assert bytes(rep) == bytes(C.sizeof(rep))
    r = ts.evaluate(sets["given"][:0], pixels=pixels[:0])
    assert r.n == 0 and r.cost == 0.0 and not r.confusion.any()
    ts.close()


def test_evaluate_leaves_a_training_context_alone_and_agrees_with_its_follower():
    from tnml_amd.fixedl import TrainStates
    px, lab, ph, W = make_problem(12, 60, 4, 3, pixel_boost=200.0)
    held = make_problem(12, 40, 4, 17, pixel_boost=200.0)
    hlab = np.asarray(held[1], dtype=np.int32)
    ts = TrainStates(lab, 12, 4, phi=ph)
    ts.set_mps(W)
    ts.init()
    ts.setBond(1)
    B = ts.bond_tensor(1)
    envs = [ts.env(j) for j in range(3, 13)]                    # (the right environments tnml_env_init built)
    q0 = ts.quadcost(B, 1e-3)
    rep = ts.evaluate(hlab, phi=held[2])
    _ints_equal(rep, eval_model.report(_toverlap(held[2], hlab, W), hlab))
    assert np.array_equal(ts.bond_tensor(1), B)
    for j, e in zip(range(3, 13), envs):
        assert np.array_equal(ts.env(j), e), j
    q1 = ts.quadcost(B, 1e-3)
    assert q0[0] == q1[0] and np.array_equal(q0[1], q1[1]) and q0[2:] == q1[2:]
    ts.close()
    # with a follower attached: the follower's own numbers for its images
    ts = TrainStates(lab, 12, 4, phi=ph)
    ts.set_mps(W)
    ts.init()
    hs = TrainStates(hlab, 12, 4, phi=held[2])
    ts.attach_heldout(hs)
    h = ts.heldout_report()
    rep = ts.evaluate(hlab, phi=held[2])
    print("follower cost", h["cost"], "streamed", rep.cost, "rel", abs(h["cost"] - rep.cost) / h["cost"])
    assert rep.n == h["count"] and rep.ncorrect == h["ncorrect"]
    assert abs(rep.cost - h["cost"]) <= 1e-10 * h["cost"]      # the tolerance of tests/test_heldout_gpu.py between follower and oracle
    np.testing.assert_allclose(rep.label_cost, h["label_cost"], rtol=1e-10, atol=1e-10 * h["cost"])
    ts.close()
    hs.close()


def test_workspace_grows_by_the_documented_amount():
    """include/tnml.h: 4 C + 1040 bytes from the first tnml_evaluate_* call on, C = predict_chunk rounded up to 64"""
    pixels, phi, W, _, _, sets = _small(12, 4)
    ts = _dataless(12, 4, W)
    ts.set_option("predict_chunk", 100)
    ts.predict(phi=phi)
    before = ts.device_bytes()
    ts.evaluate(sets["given"], phi=phi)
    assert ts.device_bytes() - before == 4 * 128 + 1040
    ts.evaluate(sets["given"], phi=phi)
    assert ts.device_bytes() - before == 4 * 128 + 1040
    ts.set_option("predict_chunk", 16)                          # re-made with the predict workspace
    ts.predict(phi=phi)
    small = ts.device_bytes()
    ts.evaluate(sets["given"], phi=phi)
    assert ts.device_bytes() - small == 4 * 64 + 1040
    fresh = _dataless(12, 4, W)                                 # what the release gave back is what had been counted
    fresh.set_option("predict_chunk", 16)
    fresh.evaluate(sets["given"], phi=phi)
    assert fresh.device_bytes() == ts.device_bytes()
    fresh.close()
    ts.close()
