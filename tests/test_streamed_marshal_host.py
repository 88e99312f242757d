"""CPU tests of how the Python host path of the streamed calls (predict, evaluate, site_response, site_gradient, backward,
gradient_step of tnml_amd/fixedl.py) hands its arrays to the C entry points.  No GPU: a TrainStates that was never created, with a
recorder in the library's place (the pattern of test_device_io_host.py).  The recorder reads every input array through the pointer
it is given, while the call is in progress, and writes a pattern through every output pointer: so the tests see which entry is
called, with which n, that every array argument is C-contiguous memory of the right dtype and shape holding the caller's values,
that absent arrays arrive as None, and that what the wrapper returns is what the library wrote."""
import ctypes as C
import re

import numpy as np
import pytest

N, NL, C0 = 6, 10, 3
# the arguments behind (handle, n) of every streamed entry, in the header's order
SIG = {"predict": ("x", "weights", "pred"), "evaluate": ("x", "labels", "rep", "weights", "pred"),
       "response": ("x", "which", "resp", "weights", "pred"), "site_gradient": ("x", "labels", "coef", "grad", "weights", "pred"),
       "backward": ("x", "labels", "coef", "grad", "dphi", "weights", "pred"), "site_step": ("x", "labels", "coef", "par", "rep")}
OUTPUTS = ("weights", "pred", "resp", "grad", "dphi")


def _dims(j):
    return (1 if j == 1 else 2, 2, 1 if j == N else 2) + ((NL,) if j == C0 else ())


SHAPES = [_dims(j) for j in range(1, N + 1)]
ELEMS = int(sum(np.prod(s) for s in SHAPES))


def _pattern(name, shape, dtype):
    k = OUTPUTS.index(name) + 1
    return (np.arange(int(np.prod(shape))) * 7 % 101 + 1000 * k).astype(dtype).reshape(shape)


class _Recorder:
    """stands where the ctypes library stands; every call succeeds.  calls: (name, n, {argument: value}) of the streamed entries
    and (name, args) of the options set; `every`: every entry point called, in order"""

    def __init__(self, ts):
        self.ts, self.calls, self.every = ts, [], []

    def _shape(self, arg, n, form):
        ts = self.ts
        return {"x": (n, ts._bytes_per_image) if form == "u8" else (n, ts.N, 2), "labels": (n,), "which": (n,), "coef": (n, ts.nl),
                "weights": (n, ts.nl), "pred": (n,), "resp": (n, ts.N, 2), "dphi": (n, ts.N, 2), "grad": (max(ELEMS, 1),)}[arg]

    def _streamed(self, name, family, form, args):
        n, rec = args[1], {}
        assert len(args) == 2 + len(SIG[family]), (name, len(args))
        for arg, v in zip(SIG[family], args[2:]):
            if v is None:
                rec[arg] = None
            elif arg in ("rep", "par"):
                rec[arg] = v._obj                                             # byref(struct)
                if arg == "rep":
                    setattr(v._obj, "n" if family == "evaluate" else "t", n)
            else:
                assert isinstance(v, C._Pointer), (name, arg, type(v))
                a = np.ctypeslib.as_array(v, shape=self._shape(arg, n, form))
                assert a.dtype == np.dtype(type(v)._type_)
                if arg in OUTPUTS:
                    a[...] = _pattern(arg, a.shape, a.dtype)
                    rec[arg] = "out"
                else:
                    rec[arg] = a.copy()
        self.calls.append((name, n, rec))

    def __getattr__(self, name):
        def call(*args):
            self.every.append(name)
            m = re.fullmatch(r"tnml_(predict|evaluate|response|site_gradient|backward|site_step)_(u8|phi)", name)
            if m:
                self._streamed(name, m.group(1), m.group(2), args)
            elif name == "tnml_site_dims":
                s = _dims(args[1])
                args[2].value, args[3].value, args[4].value = s[0], s[2], int(len(s) == 4)
            elif name == "tnml_site_gradient_size":
                args[1]._obj.value = ELEMS
                if args[2] is not None:
                    np.ctypeslib.as_array(args[2], shape=(N + 1,))[...] = np.cumsum([0] + [int(np.prod(s)) for s in SHAPES])
            elif name.startswith("tnml_set_option"):
                self.calls.append((name, args[1:]))
            return 0
        return call


def _uncreated(bytes_per_image=N):
    from tnml_amd.fixedl import TrainStates
    ts = TrainStates.__new__(TrainStates)
    ts._h = C.c_void_p()
    ts.N, ts.nl, ts.device, ts._bytes_per_image, ts.single, ts._last_chunk = N, NL, 0, bytes_per_image, False, None
    ts._L = _Recorder(ts)
    return ts


def _inputs(n, S=N, awkward=False):
    """the caller's arrays; awkward: none of them contiguous or of the C call's dtype"""
    rng = np.random.default_rng(11)
    d = dict(pixels=rng.integers(0, 256, (n, S), dtype=np.uint8), phi=rng.standard_normal((n, N, 2)),
             labels=rng.integers(0, NL, n).astype(np.int32), coef=rng.standard_normal((n, NL)), which=rng.integers(0, NL, n).astype(np.int32))
    if awkward:
        d["pixels"] = np.repeat(d["pixels"].astype(np.int64), 2, axis=1)[:, ::2]
        d["phi"] = np.asfortranarray(d["phi"].astype(np.float32))
        d["labels"] = np.repeat(d["labels"].astype(np.int64), 3)[::3]
        d["coef"] = np.asfortranarray(d["coef"].astype(np.float32))
        d["which"] = np.repeat(d["which"].astype(np.int64), 2)[::2]
        assert not any(d[k].flags.c_contiguous for k in d)
    return d


WANT_DTYPE = dict(x_u8=np.uint8, x_phi=np.float64, labels=np.int32, coef=np.float64, which=np.int32)


def _check(ts, entry, n, given, outputs):
    """the one streamed call recorded: its entry, n, the inputs in `given` value for value in the C call's dtype, every other input
    None, and exactly `outputs` written"""
    streamed = [c for c in ts._L.calls if len(c) == 3]
    assert [c[0] for c in streamed] == [entry]
    name, got_n, rec = streamed[0]
    assert got_n == n
    form = entry.rsplit("_", 1)[1]
    for arg, v in rec.items():
        if arg in ("rep", "par"):
            continue
        if arg in OUTPUTS:
            assert (v == "out") == (arg in outputs), (arg, v)
        elif arg in given:
            dt = WANT_DTYPE["x_" + form if arg == "x" else arg]
            assert v.dtype == dt and v.flags.c_contiguous and np.array_equal(v, np.asarray(given[arg]).astype(dt)), arg
        else:
            assert v is None, arg
    return rec


def _pat(name, *shape):
    return _pattern(name, shape, np.int32 if name == "pred" else np.float64)


def _split(flat):
    out, at = [], 0
    for s in SHAPES:
        k = int(np.prod(s))
        out.append(flat[at:at + k].reshape(s, order="F"))
        at += k
    return out


FORMS = [("pixels", False, N), ("pixels", True, N), ("pixels", False, 15), ("phi", False, N), ("phi", True, N)]


@pytest.mark.parametrize("form,awkward,S", FORMS)
def test_predict(form, awkward, S):
    ts, n = _uncreated(S), 5
    d = _inputs(n, S, awkward)
    w, pred = ts.predict(**{form: d[form]})
    _check(ts, "tnml_predict_" + ("u8" if form == "pixels" else "phi"), n, {"x": d[form]}, {"weights", "pred"})
    assert np.array_equal(w, _pat("weights", n, NL)) and np.array_equal(pred, _pat("pred", n)) and pred.dtype == np.int32
    ts._h = None                                                              # (nothing to destroy)


@pytest.mark.parametrize("want_weights", [False, True])
@pytest.mark.parametrize("form,awkward,S", FORMS)
def test_evaluate(form, awkward, S, want_weights):
    ts, n = _uncreated(S), 4
    d = _inputs(n, S, awkward)
    r = ts.evaluate(d["labels"], want_weights=want_weights, **{form: d[form]})
    _check(ts, "tnml_evaluate_" + ("u8" if form == "pixels" else "phi"), n, {"x": d[form], "labels": d["labels"]}, {"weights", "pred"} if want_weights else set())
    rep = r[0] if want_weights else r
    assert rep.n == n
    if want_weights:
        assert np.array_equal(r[1][0], _pat("weights", n, NL)) and np.array_equal(r[1][1], _pat("pred", n))
    ts._h = None


@pytest.mark.parametrize("with_which,want_weights", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("form,awkward,S", FORMS)
def test_site_response(form, awkward, S, with_which, want_weights):
    ts, n = _uncreated(S), 3
    d = _inputs(n, S, awkward)
    r = ts.site_response(which=d["which"] if with_which else None, want_weights=want_weights, **{form: d[form]})
    given = {"x": d[form], **({"which": d["which"]} if with_which else {})}
    _check(ts, "tnml_response_" + ("u8" if form == "pixels" else "phi"), n, given, {"resp"} | ({"weights", "pred"} if want_weights else set()))
    resp = r[0] if want_weights else r
    assert np.array_equal(resp, _pat("resp", n, N, 2))
    if want_weights:
        assert np.array_equal(r[1][0], _pat("weights", n, NL)) and np.array_equal(r[1][1], _pat("pred", n))
    ts._h = None


@pytest.mark.parametrize("mode,want_weights", [("labels", False), ("coef", False), ("coef", True)])
@pytest.mark.parametrize("form,awkward,S", FORMS)
def test_site_gradient(form, awkward, S, mode, want_weights):
    ts, n = _uncreated(S), 5
    d = _inputs(n, S, awkward)
    r = ts.site_gradient(want_weights=want_weights, **{form: d[form], mode: d[mode]})
    _check(ts, "tnml_site_gradient_" + ("u8" if form == "pixels" else "phi"), n, {"x": d[form], mode: d[mode]}, {"grad"} | ({"weights", "pred"} if want_weights else set()))
    grads = r[0] if want_weights else r
    assert len(grads) == N and all(g.shape == s and np.array_equal(g, e) for g, s, e in zip(grads, SHAPES, _split(_pat("grad", ELEMS))))
    if want_weights:
        assert np.array_equal(r[1][0], _pat("weights", n, NL)) and np.array_equal(r[1][1], _pat("pred", n))
    assert "tnml_backward_u8" not in ts._L.every and "tnml_backward_phi" not in ts._L.every
    assert ts._last_chunk == n
    ts._h = None


@pytest.mark.parametrize("mode,want_sites,want_inputs,want_weights", [("labels", True, True, False), ("coef", True, False, True), ("labels", False, True, True)])
@pytest.mark.parametrize("form,awkward,S", FORMS)
def test_backward(form, awkward, S, mode, want_sites, want_inputs, want_weights):
    ts, n = _uncreated(S), 5
    d = _inputs(n, S, awkward)
    r = ts.backward(want_sites=want_sites, want_inputs=want_inputs, want_weights=want_weights, **{form: d[form], mode: d[mode]})
    outs = ({"grad"} if want_sites else set()) | ({"dphi"} if want_inputs else set()) | ({"weights", "pred"} if want_weights else set())
    _check(ts, "tnml_backward_" + ("u8" if form == "pixels" else "phi"), n, {"x": d[form], mode: d[mode]}, outs)
    assert len(r) == (3 if want_weights else 2)
    if want_sites:
        assert all(g.shape == s and np.array_equal(g, e) for g, s, e in zip(r[0], SHAPES, _split(_pat("grad", ELEMS))))
    else:
        assert r[0] is None
    assert np.array_equal(r[1], _pat("dphi", n, N, 2)) if want_inputs else r[1] is None
    if want_weights:
        assert np.array_equal(r[2][0], _pat("weights", n, NL)) and np.array_equal(r[2][1], _pat("pred", n))
    ts._h = None


@pytest.mark.parametrize("mode", ["labels", "coef"])
@pytest.mark.parametrize("form,awkward,S", FORMS)
def test_gradient_step(form, awkward, S, mode):
    ts, n = _uncreated(S), 5
    d = _inputs(n, S, awkward)
    r = ts.gradient_step(method="adam", lr=1e-3, momentum=.5, beta1=.8, beta2=.95, eps=1e-6, clip=2., scale=.25, **{form: d[form], mode: d[mode]})
    rec = _check(ts, "tnml_site_step_" + ("u8" if form == "pixels" else "phi"), n, {"x": d[form], mode: d[mode]}, set())
    p = rec["par"]
    assert (p.method, p.lr, p.momentum, p.beta1, p.beta2, p.eps, p.clip, p.scale) == (1, 1e-3, .5, .8, .95, 1e-6, 2., .25)
    assert r.t == n and ts._last_chunk == n
    ts._h = None


def _all_methods(ts, d, form="phi", **kw):
    """the six methods on the same images, each as a thunk"""
    x = {form: d[form]}
    return [lambda: ts.predict(**x, **kw), lambda: ts.evaluate(d["labels"], **x, **kw), lambda: ts.site_response(**x, which=d["which"]),
            lambda: ts.site_gradient(labels=d["labels"], **x, **kw), lambda: ts.backward(coef=d["coef"], **x, **kw),
            lambda: ts.gradient_step(labels=d["labels"], lr=.1, **x, **kw)]


def test_wrong_shapes_are_refused_before_any_c_call():
    ts, n = _uncreated(), 4
    d = _inputs(n)
    for call in _all_methods(ts, dict(d, pixels=d["pixels"][:, :5]), "pixels"):
        with pytest.raises(ValueError, match=re.escape("pixels must have shape [n, 6], got (4, 5)")):
            call()
    for call in _all_methods(ts, dict(d, pixels=d["pixels"].ravel()), "pixels"):
        with pytest.raises(ValueError, match=re.escape("pixels must have shape [n, 6], got (24,)")):
            call()
    for call in _all_methods(ts, dict(d, phi=d["phi"][:, :5])):
        with pytest.raises(AssertionError):
            call()
    for form in ("pixels", "phi"):
        x = {form: d[form]}
        for call in (lambda: ts.evaluate(d["labels"][:3], **x), lambda: ts.site_gradient(labels=d["labels"][:3], **x),
                     lambda: ts.backward(labels=d["labels"][:3], **x), lambda: ts.gradient_step(labels=d["labels"][:3], lr=.1, **x)):
            with pytest.raises(ValueError, match=re.escape("labels must have shape [4], got (3,)")):
                call()
        for call in (lambda: ts.site_gradient(coef=d["coef"][:, :9], **x), lambda: ts.backward(coef=d["coef"][:, :9], **x),
                     lambda: ts.gradient_step(coef=d["coef"][:, :9], lr=.1, **x)):
            with pytest.raises(ValueError, match=re.escape("coef must have shape [4, 10], got (4, 9)")):
                call()
        with pytest.raises(ValueError, match=re.escape("which must have shape [4], got (4, 1)")):
            ts.site_response(which=d["which"][:, None], **x)
    assert ts._L.every == []
    ts._h = None


def test_exactly_one_of_pixels_and_phi():
    ts = _uncreated()
    d = _inputs(3)
    for kw in ({}, {"pixels": d["pixels"], "phi": d["phi"]}):
        for call in (lambda: ts.predict(**kw), lambda: ts.evaluate(d["labels"], **kw), lambda: ts.site_response(**kw),
                     lambda: ts.site_gradient(labels=d["labels"], **kw), lambda: ts.backward(labels=d["labels"], **kw),
                     lambda: ts.gradient_step(labels=d["labels"], lr=.1, **kw)):
            with pytest.raises(ValueError, match="need exactly one of pixels or phi"):
                call()
    assert ts._L.every == []
    ts._h = None


@pytest.mark.parametrize("form", ["pixels", "phi"])
def test_dtype_sets_the_option_of_the_call(form):
    ts = _uncreated()
    d = _inputs(3)
    calls = _all_methods(ts, d, form, dtype="f32")
    del calls[2]                                                              # (site_response takes no dtype)
    for call, option, entry in zip(calls, ["predict_dtype"] * 2 + ["gradient_dtype"] * 3, ["predict", "evaluate", "site_gradient", "backward", "site_step"]):
        ts._L.calls.clear()
        call()
        assert ts._L.calls[0] == ("tnml_set_option", (option.encode(), 1))
        assert [c[0] for c in ts._L.calls[1:]] == ["tnml_%s_%s" % (entry, "u8" if form == "pixels" else "phi")]
    assert ts.get_dtype_option("predict_dtype") == 1 and ts.get_dtype_option("gradient_dtype") == 1
    ts.predict(dtype="f64", **{form: d[form]})
    ts.backward(labels=d["labels"], dtype="f64", **{form: d[form]})
    assert ts.get_dtype_option("predict_dtype") == 0 and ts.get_dtype_option("gradient_dtype") == 0
    ts._L.calls.clear()
    ts.predict(**{form: d[form]})                                             # no dtype: no option is set
    assert [c[0] for c in ts._L.calls] == ["tnml_predict_" + ("u8" if form == "pixels" else "phi")]
    ts._h = None


def test_an_unknown_dtype_is_refused_with_no_call():
    ts = _uncreated()
    d = _inputs(3)
    for form in ("pixels", "phi"):
        calls = _all_methods(ts, d, form, dtype="f16")
        del calls[2]
        for call in calls:
            with pytest.raises(ValueError, match="dtype must be one of"):
                call()
    assert ts._L.every == []
    ts._h = None
