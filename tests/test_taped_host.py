"""CPU tests of the taped forward / backward and the batched site upload above the C ABI.  No GPU.
1. How TrainStates.forward_taped / backward_taped / tape_ticket / set_sites hand their arrays to the C entry points: a TrainStates that
   was never created with a recorder in the library's place, the pattern of tests/test_streamed_marshal_host.py.
2. Which calls MPSFunction / MPSFunction32 / MPSLayer (tnml_amd/torch_layer.py) make on CPU tensors, against a stand-in TrainStates
   that records them."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_streamed_marshal_host as mh
from test_streamed_marshal_host import ELEMS, N, NL, SHAPES

TICKET = 4711


class _Recorder(mh._Recorder):
    """the streamed recorder plus the entries of the tape: every input read through its pointer while the call is in progress, a pattern
    written through every output pointer, TICKET through the ticket pointer"""

    def __getattr__(self, name):
        base = super().__getattr__(name)

        def call(*args):
            if name in ("tnml_forward_taped_u8", "tnml_forward_taped_phi"):
                self.every.append(name)
                assert len(args) == 6
                n, form = args[1], name.rsplit("_", 1)[1]
                x = np.ctypeslib.as_array(args[2], shape=self._shape("x", n, form))
                assert x.dtype == (np.uint8 if form == "u8" else np.float64)
                for arg, v in (("weights", args[3]), ("pred", args[4])):
                    a = np.ctypeslib.as_array(v, shape=self._shape(arg, n, form))
                    a[...] = mh._pattern(arg, a.shape, a.dtype)
                args[5]._obj.value = TICKET
                self.n = n
                self.calls.append((name, n, {"x": x.copy()}))
                return 0
            if name == "tnml_backward_taped":
                self.every.append(name)
                assert len(args) == 5
                rec = {"ticket": args[1], "coef": np.ctypeslib.as_array(args[2], shape=(self.n, NL)).copy()}
                assert rec["coef"].dtype == np.float64
                for arg, v in (("grad", args[3]), ("dphi", args[4])):
                    rec[arg] = None if v is None else "out"
                    if v is not None:
                        a = np.ctypeslib.as_array(v, shape=self._shape(arg, self.n, "phi"))
                        a[...] = mh._pattern(arg, a.shape, a.dtype)
                self.calls.append((name, self.n, rec))
                return 0
            if name == "tnml_tape_ticket":
                self.every.append(name)
                args[1]._obj.value, args[2]._obj.value = TICKET, self.n
                return 0
            if name == "tnml_set_site":
                self.every.append(name)
                j, ml, mr, has_label = args[1:5]
                shape = (ml, 2, mr) + ((NL,) if has_label else ())
                self.calls.append((name, j, np.ctypeslib.as_array(args[5], shape=(int(np.prod(shape)),)).reshape(shape, order="F").copy()))
                return 0
            return base(*args)
        return call


def _uncreated(bytes_per_image=N):
    ts = mh._uncreated(bytes_per_image)
    ts._L = _Recorder(ts)
    return ts


@pytest.mark.parametrize("form,awkward,S", mh.FORMS)
def test_forward_taped(form, awkward, S):
    ts, n = _uncreated(S), 5
    d = mh._inputs(n, S, awkward)
    w, pred, t = ts.forward_taped(**{form: d[form]})
    entry = "tnml_forward_taped_" + ("u8" if form == "pixels" else "phi")
    assert ts._L.every == [entry]
    name, got_n, rec = ts._L.calls[0]
    want = np.asarray(d[form]).astype(np.uint8 if form == "pixels" else np.float64)
    assert (name, got_n) == (entry, n) and rec["x"].flags.c_contiguous and np.array_equal(rec["x"], want)
    assert t == TICKET and isinstance(t, int)
    assert np.array_equal(w, mh._pat("weights", n, NL)) and np.array_equal(pred, mh._pat("pred", n)) and pred.dtype == np.int32
    ts._h = None


def test_forward_taped_sets_gradient_dtype_not_predict_dtype():
    ts = _uncreated()
    d = mh._inputs(3)
    ts.forward_taped(phi=d["phi"], dtype="f32")
    assert ts._L.calls[0] == ("tnml_set_option", (b"gradient_dtype", 1)) and ts.get_dtype_option("predict_dtype") == 0
    with pytest.raises(ValueError, match="dtype must be one of"):
        ts.forward_taped(phi=d["phi"], dtype="f16")
    with pytest.raises(ValueError, match="need exactly one of pixels or phi"):
        ts.forward_taped()
    ts._h = None


@pytest.mark.parametrize("want_sites,want_inputs", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("awkward", [False, True])
def test_backward_taped(awkward, want_sites, want_inputs):
    ts, n = _uncreated(), 5
    d = mh._inputs(n, N, awkward)
    _, _, t = ts.forward_taped(phi=d["phi"])
    ts._L.calls.clear(); ts._L.every.clear()
    grads, dphi = ts.backward_taped(t, d["coef"], want_sites=want_sites, want_inputs=want_inputs)
    assert [e for e in ts._L.every if e != "tnml_site_gradient_size" and e != "tnml_site_dims"] == ["tnml_tape_ticket", "tnml_backward_taped"]
    name, _, rec = [c for c in ts._L.calls if c[0] == "tnml_backward_taped"][0]
    assert rec["ticket"] == TICKET
    assert rec["coef"].flags.c_contiguous and np.array_equal(rec["coef"], np.asarray(d["coef"]).astype(np.float64))
    assert (rec["grad"] == "out") == want_sites and (rec["dphi"] == "out") == want_inputs
    if want_sites:
        assert all(g.shape == s and np.array_equal(g, e) for g, s, e in zip(grads, SHAPES, mh._split(mh._pat("grad", ELEMS))))
    else:
        assert grads is None
    assert np.array_equal(dphi, mh._pat("dphi", n, N, 2)) if want_inputs else dphi is None
    assert ts._last_chunk == n
    with pytest.raises(ValueError, match="coef must have shape"):
        ts.backward_taped(t, d["coef"][:, :9])
    # the C call takes no n: fewer or more rows than the live ticket's forward had are refused before any buffer is made or call is sent
    ts._L.every.clear()
    for rows in (n - 1, n + 1, 0):
        with pytest.raises(ValueError, match="coef has %d rows, the forward of ticket %d had %d images" % (rows, TICKET, n)):
            ts.backward_taped(t, np.zeros((rows, NL)))
    assert set(ts._L.every) == {"tnml_tape_ticket"}
    ts._h = None


def test_tape_ticket_and_host_set_sites():
    ts = _uncreated()
    ts._L.n = 7
    assert ts.tape_ticket() == (TICKET, 7)
    rng = np.random.default_rng(1)
    A = {j: rng.standard_normal(mh._dims(j)) for j in (4, 1, 3)}
    ts._L.calls.clear(); ts._L.every.clear()
    ts.set_sites([4, 1, 3], [A[4], torch.from_numpy(A[1]), np.asfortranarray(A[3]).astype(np.float32)])      # host arrays: set_site one by one
    assert ts._L.every == ["tnml_set_site"] * 3
    assert [c[1] for c in ts._L.calls] == [4, 1, 3]
    assert np.array_equal(ts._L.calls[0][2], A[4]) and np.array_equal(ts._L.calls[1][2], A[1]) and np.array_equal(ts._L.calls[2][2], A[3].astype(np.float32))
    ts.set_sites([], [])
    assert len(ts._L.every) == 3
    with pytest.raises(ValueError, match="2 sites, 1 tensors"):
        ts.set_sites([1, 2], [A[1]])
    ts._h = None


# ---- the torch layer on a stand-in ----
class _Stub:
    """what tnml_amd/torch_layer.py asks of a TrainStates; every call recorded.  live: what tape_ticket() answers (None: the ticket the
    last forward_taped gave)"""
    device = 0

    def __init__(self, chunk=8, n_sites=4):
        self.calls, self.options, self.chunk, self.n_sites, self.live, self.next = [], {}, chunk, n_sites, None, 10
        self.N = n_sites

    def _w(self, n):
        return np.arange(n * NL, dtype=np.float64).reshape(n, NL)

    def gradient_chunk(self):
        return self.chunk

    def get_dtype_option(self, name):
        return self.options.get(name, 0)

    def set_option(self, name, value):
        self.calls.append(("set_option", name, value))
        self.options[name] = value

    def get_site(self, j):
        return np.full((2, 2, 2), float(j))

    def get_mps(self, device=False):
        return [torch.full((2, 2, 2), float(j), dtype=torch.float64) for j in range(1, self.n_sites + 1)]

    def set_site(self, j, A):
        self.calls.append(("set_site", j))

    def set_sites(self, js, tensors):
        self.calls.append(("set_sites", list(js), [tuple(t.shape) for t in tensors]))

    def predict(self, phi=None):
        self.calls.append(("predict", len(phi), dict(self.options)))
        return self._w(len(phi)), np.zeros(len(phi), dtype=np.int32)

    def forward_taped(self, phi=None):
        self.next += 1
        self.calls.append(("forward_taped", len(phi), dict(self.options)))
        return self._w(len(phi)), np.zeros(len(phi), dtype=np.int32), self.next

    def tape_ticket(self):
        self.calls.append(("tape_ticket",))
        return (self.next if self.live is None else self.live), 0

    def _grads(self, want_sites):
        return [np.full((2, 2, 2), 10.0 + j) for j in range(self.n_sites)] if want_sites else None

    def backward_taped(self, ticket, coef, want_sites=True, want_inputs=True, inputs32=False):
        self.calls.append(("backward_taped", ticket, bool(want_sites), bool(want_inputs), dict(self.options)))
        return self._grads(want_sites), (np.ones((len(coef), self.N, 2)) if want_inputs else None)

    def backward(self, coef=None, phi=None, want_sites=True, want_inputs=True):
        self.calls.append(("backward", bool(want_sites), bool(want_inputs), dict(self.options)))
        return self._grads(want_sites), (np.ones((len(coef), self.N, 2)) if want_inputs else None)

    def names(self):
        return [c[0] for c in self.calls if c[0] != "set_option"]


def _phi(n, grad=True):
    return torch.ones(n, 4, 2, dtype=torch.float64, requires_grad=grad)


def test_function_takes_the_tape_while_the_ticket_is_live():
    from tnml_amd.torch_layer import MPSFunction
    st = _Stub()
    x = _phi(5)
    sites = [torch.ones(2, 2, 2, dtype=torch.float64, requires_grad=True) for _ in range(4)]
    out = MPSFunction.apply(st, x, *sites)
    assert st.names() == ["forward_taped"] and torch.equal(out, torch.from_numpy(st._w(5)))
    out.sum().backward()
    assert st.names() == ["forward_taped", "tape_ticket", "backward_taped"]
    assert st.calls[-1][:4] == ("backward_taped", 11, True, True)
    assert torch.equal(x.grad, torch.ones(5, 4, 2, dtype=torch.float64)) and all(torch.equal(s.grad, torch.full((2, 2, 2), 10.0 + k, dtype=torch.float64)) for k, s in enumerate(sites))
    # phi alone: no site gradient is asked for
    st.calls.clear()
    MPSFunction.apply(st, _phi(5)).sum().backward()
    assert st.calls[-1][:4] == ("backward_taped", 12, False, True)


def test_function_falls_back_when_the_ticket_is_stale():
    from tnml_amd.torch_layer import MPSFunction
    st = _Stub()
    x = _phi(5)
    out = MPSFunction.apply(st, x)
    st.live = 99                                                                     # the context answers another ticket
    out.sum().backward()
    assert st.names() == ["forward_taped", "tape_ticket", "backward"] and st.calls[-1][:3] == ("backward", False, True)
    assert torch.equal(x.grad, torch.ones(5, 4, 2, dtype=torch.float64))
    st.live, st.calls = 0, []                                                        # or none at all
    out = MPSFunction.apply(st, x)
    out.sum().backward()
    assert st.names() == ["forward_taped", "tape_ticket", "backward"]


def test_function_predicts_when_no_gradient_is_needed_or_the_batch_is_too_large():
    from tnml_amd.torch_layer import MPSFunction, MPSFunctionPlain
    st = _Stub(chunk=8)
    MPSFunction.apply(st, _phi(5, grad=False))                                       # nothing needs a gradient
    with torch.no_grad():
        MPSFunction.apply(st, _phi(5))                                               # under no_grad nothing changes
    assert st.names() == ["predict", "predict"]
    st.calls.clear()
    x = _phi(9)                                                                      # n > gradient_chunk
    MPSFunction.apply(st, x).sum().backward()
    assert st.names() == ["predict", "backward"]
    st.calls.clear()
    MPSFunction.apply(st, _phi(8)).sum().backward()                                  # n = gradient_chunk: one chunk
    assert st.names() == ["forward_taped", "tape_ticket", "backward_taped"]
    st.calls.clear()
    MPSFunction.apply(st, _phi(0)).sum().backward()                                  # n = 0
    assert st.names()[0] == "predict"
    st.calls.clear()
    MPSFunctionPlain.apply(st, _phi(5)).sum().backward()                             # the function without the tape
    assert st.names() == ["predict", "backward"]


def test_function32_sets_and_restores_gradient_dtype():
    from tnml_amd.torch_layer import MPSFunction32, MPSFunction32Plain
    st = _Stub()
    MPSFunction32.apply(st, _phi(5)).sum().backward()
    fwd, bwd = [c for c in st.calls if c[0] == "forward_taped"][0], [c for c in st.calls if c[0] == "backward_taped"][0]
    assert fwd[2] == {"gradient_dtype": 1} and bwd[4].get("gradient_dtype") == 1 and bwd[4].get("predict_dtype", 0) == 0
    assert st.options == {"gradient_dtype": 0}
    st.calls.clear()
    with torch.no_grad():
        MPSFunction32.apply(st, _phi(5))
    assert [c for c in st.calls if c[0] == "predict"][0][2] == {"gradient_dtype": 0, "predict_dtype": 1}
    assert st.options == {"gradient_dtype": 0, "predict_dtype": 0}
    st.calls.clear()
    MPSFunction32Plain.apply(st, _phi(5)).sum().backward()
    assert st.names() == ["predict", "backward"] and [c for c in st.calls if c[0] == "backward"][0][3]["gradient_dtype"] == 1
    assert st.options == {"gradient_dtype": 0, "predict_dtype": 0}


def test_layer_taped_flag_and_one_set_sites_call_with_the_changed_sites():
    from tnml_amd.torch_layer import MPSLayer
    st = _Stub()
    for taped, want in ((False, ["predict", "backward"]), (True, ["forward_taped", "tape_ticket", "backward_taped"])):
        st.calls.clear()
        layer = MPSLayer(st, train_sites=True, taped=taped)
        layer(_phi(5)).sum().backward()
        assert st.names() == want and st.calls[-1][-3 if taped else 1] is True
    assert MPSLayer(st).taped is False                                               # the default: the layer as it was before the tape
    # a device layer (its parameters on the CPU here: the stand-in hands out CPU tensors): ONE set_sites call, exactly the changed sites
    dev = MPSLayer(st, train_sites=True, device="cuda", taped=True)
    assert dev.on_device and dev.sync_sites() == []
    with torch.no_grad():
        dev.sites[2].mul_(0.5); dev.sites[0].add_(1.0)
    st.calls.clear()
    assert dev.sync_sites() == [1, 3]
    assert st.calls == [("set_sites", [1, 3], [(2, 2, 2), (2, 2, 2)])]
    assert dev.sync_sites() == [] and len(st.calls) == 1
    cpu = MPSLayer(st, train_sites=True)
    with torch.no_grad():
        cpu.sites[1].mul_(2.0)
    st.calls.clear()
    assert cpu.sync_sites() == [2] and st.calls == [("set_site", 2)]
