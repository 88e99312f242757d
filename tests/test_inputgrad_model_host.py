"""tests/inputgrad_model.py proved on the host: W is linear in every site's feature, so dphi is the oracle's forward pass on modified
features, exactly; the Euler tie holds at every site; a one-hot coefficient gives the site responses of tests/response_model.py; each
planted defect exceeds the bound of the GPU tests on their own data; and the backward wiring of tnml_amd/torch_layer.py hands the
model's arrays to the right places, on a stub in the place of a TrainStates.  No GPU."""
import numpy as np
import pytest

import inputgrad_model as im
import response_model as rm
import sitegrad_model as sm
from conftest import make_problem

U = 2.0 ** -53


def _chain(N, single):
    """odd, unequal bonds; 12 images with the boosted features of the other tests"""
    dims = [1] + [(3, 5, 7, 2, 9, 5, 3, 7)[b % 8] for b in range(N - 1)] + [1]
    W = sm.mps_with_dims(dims, 40 + N, label_site=0 if single else None)
    _, labels, phi, _ = make_problem(N, 12, 2, 7, pixel_boost=200.0)
    return W, phi, np.asarray(labels, dtype=np.int32)


def _plain(W):
    """the per-label variant's W: no Label index"""
    return [A if A.ndim == 3 else A[..., 0] * 3.0 for A in W]


def _oracle_weights(W, phi, single):
    from oracle import pyoracle
    lab = np.zeros(len(phi), dtype=np.int32)
    if not single:
        o = pyoracle.Oracle(phi, lab, W)
        return np.stack([o.toverlap(i) for i in range(len(phi))])
    o = pyoracle.SingleOracle(phi, lab, 3, W)
    return np.array([[o.output(i)] for i in range(len(phi))])


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("N", [4, 6, 9])
def test_dphi_is_the_forward_pass_on_unit_features(N, single):
    """dphi[n, j, s] = sum_l c_nl W_l(x_n with phi_j := e_s), exactly: neither a step size nor a finite-difference error enters.  The
    right side is the oracle's forward pass on the modified features."""
    W, phi, _ = _chain(N, single)
    n, nl = len(phi), 1 if single else 10
    coef = np.random.default_rng(N).standard_normal((n, nl))
    dphi, _ = im.input_gradient(W, phi, coef=coef)
    bnd = im.bound(W, phi, coef=coef)
    mod = np.repeat(phi[:, None, None], N, axis=1).repeat(2, axis=2)                # [n, j, s, N, 2]
    for j in range(N):
        for s in range(2):
            mod[:, j, s, j] = np.eye(2)[s]
    w = _oracle_weights(W, mod.reshape(n * N * 2, N, 2), single).reshape(n, N, 2, nl)
    want = np.einsum("nl,njsl->njs", coef, w)
    ratio = im.worst_ratio(dphi, want, bnd)
    print("worst |model - oracle| / bound", ratio)
    assert ratio <= 1.
    assert (bnd < 1e-9 * np.abs(want).max()).all()                                  # the check has teeth


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("mode", ["labels", "coef"])
def test_euler_tie_at_every_site(mode, single):
    """sum_s phi[n, j, s] dphi[n, j, s] = sum_l c_nl W_l(x_n), whatever the site"""
    W, phi, labels = _chain(9, single)
    target = 3 if single else None
    nl = 1 if single else 10
    kw = dict(labels=labels, target_label=target) if mode == "labels" else dict(coef=np.random.default_rng(2).standard_normal((len(labels), nl)))
    dphi, w = im.input_gradient(W, phi, **kw)
    bnd = im.bound(W, phi, **kw)
    _, w_abs, c_abs = im.abs_input_gradient(W, phi, **kw)
    coef = kw["coef"] if mode == "coef" else 2. * (w - sm.targets(labels, nl, target))
    want = (coef * w).sum(axis=1)
    K = im.rounding_count(9, 9, nl)
    allowed = (np.abs(phi) * bnd).sum(axis=2) + K * U * (c_abs * w_abs).sum(axis=1)[:, None]
    got = (phi * dphi).sum(axis=2)
    assert (np.abs(got - want[:, None]) <= allowed).all()
    assert (allowed < 1e-9 * (c_abs * w_abs).sum(axis=1)[:, None]).all()


@pytest.mark.parametrize("N", [6, 9])
def test_a_one_hot_coefficient_is_the_site_response(N):
    """with coef = e_l the model equals response_model.response(which = l) inside the sum of both bounds"""
    W, phi, _ = _chain(N, False)
    n = len(phi)
    for label in (0, 4, 9):
        coef = np.zeros((n, 10))
        coef[:, label] = 1.
        which = np.full(n, label)
        dphi, _ = im.input_gradient(W, phi, coef=coef)
        resp, _, _ = rm.response(W, phi, which)
        allowed = im.bound(W, phi, coef=coef) + rm.bound(W, phi, which)
        assert (np.abs(dphi - resp) <= allowed).all(), label
        assert np.abs(resp).max() > 0


@pytest.mark.parametrize("defect", im.DEFECTS)
def test_planted_defects_exceed_the_bound_tenfold(defect):
    """on the data of tests/test_inputgrad_gpu.py: a label's term dropped at the centre, the inward tape's vector where Y belongs right
    of the centre, s swapped at one site, the r side read from the next bond -- the bound is not vacuous"""
    cases = [(sm.odd_case(0, 70), None), (sm.odd_case(1, 17), None), (sm.small_case(12, 5), None), (sm.small_case(4, 2), None),
             (dict(sm.small_case(12, 5), W=_plain(sm.small_case(12, 5)["W"])), 3)]
    for case, target in cases:
        for mode in ("labels", "coef"):
            for form in ("phi", "u8"):
                f = case["phi"] if form == "phi" else case["phi8"]
                kw = dict(labels=case["labels"], target_label=target) if mode == "labels" else dict(coef=case["coef"][:, :1 if target is not None else 10])
                good, _ = im.input_gradient(case["W"], f, **kw)
                bad, _ = im.input_gradient(case["W"], f, defect=defect, **kw)
                ratio = im.worst_ratio(bad, good, im.bound(case["W"], f, **kw))
                assert ratio >= 10., (defect, mode, form, len(case["W"]), ratio)


class _StubStates:
    """what tnml_amd/torch_layer.py asks of a TrainStates, answered by the models"""

    def __init__(self, W):
        self.W, self.N, self.calls = [np.array(A) for A in W], len(W), []

    def get_site(self, j):
        return self.W[j - 1]

    def set_site(self, j, A):
        self.calls.append(("set_site", j))
        self.W[j - 1] = np.array(A)

    def predict(self, phi=None):
        self.calls.append(("predict",))
        w = sm.site_gradient(self.W, phi, coef=np.zeros((len(phi), 10)))[1]
        return w, np.abs(w).argmax(axis=1).astype(np.int32)

    def backward(self, coef=None, phi=None, want_sites=True, want_inputs=True):
        self.calls.append(("backward", want_sites, want_inputs))
        return (sm.site_gradient(self.W, phi, coef=coef)[0] if want_sites else None,
                im.input_gradient(self.W, phi, coef=coef)[0] if want_inputs else None)


def test_backward_wiring_of_the_torch_layer_on_a_stub():
    """backward_arrays makes ONE backward(coef = grad_output) call and returns the model's arrays; through autograd they land on phi and
    on every site, a changed site is uploaded before the next forward, and without train_sites no site gradient is asked for"""
    import torch
    from tnml_amd import torch_layer as tl
    W, phi, _ = _chain(6, False)
    go = np.random.default_rng(5).standard_normal((len(phi), 10))
    want_phi, _ = im.input_gradient(W, phi, coef=go)
    want_sites, _ = sm.site_gradient(W, phi, coef=go)
    stub = _StubStates(W)
    dphi, grads = tl.backward_arrays(stub, phi, go, True)
    assert stub.calls == [("backward", True, True)]
    assert np.array_equal(dphi, want_phi) and all(np.array_equal(a, b) for a, b in zip(grads, want_sites))
    assert tl.backward_arrays(stub, phi, go, False)[1] is None
    for train in (True, False):
        stub = _StubStates(W)
        layer = tl.MPSLayer(stub, train_sites=train)
        assert [tuple(p.shape) for p in layer.sites] == [A.shape for A in W] and all(p.dtype == torch.float64 for p in layer.sites)
        x = torch.tensor(phi, requires_grad=True)
        out = layer(x)
        assert out.shape == (len(phi), 10) and out.dtype == torch.float64
        out.backward(torch.from_numpy(go))
        assert stub.calls == [("predict",), ("backward", train, True)]
        assert np.array_equal(x.grad.numpy(), want_phi)
        for p, g in zip(layer.sites, want_sites):
            assert (np.array_equal(p.grad.numpy(), g) if train else p.grad is None)
    stub.calls.clear()
    with torch.no_grad():
        layer.sites[2].mul_(0.5)
    layer(torch.tensor(phi))
    assert stub.calls == [("set_site", 3), ("predict",)] and np.array_equal(stub.W[2], 0.5 * W[2])
    stub.calls.clear()
    layer(torch.tensor(phi))
    assert stub.calls == [("predict",)]
