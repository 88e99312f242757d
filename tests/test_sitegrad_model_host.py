"""tests/sitegrad_model.py proved on the host: central differences of the cost (tests/eval_model.py on the oracle's weights) are the
model's gradient up to rounding, the Euler identity holds at every site, one image with a one-hot coefficient gives the site responses
of tests/response_model.py, and each planted defect exceeds the bound of the GPU tests on their own data.  No GPU."""
import numpy as np
import pytest

import eval_model
import sitegrad_model as sm
from conftest import make_problem
from response_model import response

U = 2.0 ** -53


def _chain(N, single):
    """odd, unequal bonds; 12 images with the boosted features of the other tests"""
    dims = [1] + [(3, 5, 7, 2, 9, 5, 3, 7)[b % 8] for b in range(N - 1)] + [1]
    W = sm.mps_with_dims(dims, 40 + N, label_site=0 if single else None)
    _, labels, phi, _ = make_problem(N, 12, 2, 7, pixel_boost=200.0)
    return W, phi, np.asarray(labels, dtype=np.int32)


def _oracle_weights(W, phi, labels, target):
    from oracle import pyoracle
    if target is None:
        o = pyoracle.Oracle(phi, labels, W)
        return np.stack([o.toverlap(i) for i in range(len(labels))])
    o = pyoracle.SingleOracle(phi, labels, target, W)
    return np.array([[o.output(i)] for i in range(len(labels))])


def _cost(W, phi, labels, target):
    return eval_model.report(_oracle_weights(W, phi, labels, target), labels, target)["cost"]


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("N", [4, 6, 9])
def test_central_differences_of_the_cost_are_the_gradient(N, single):
    """C is exactly quadratic in any single site tensor, so (C(A + eps D) - C(A - eps D)) / (2 eps) = <G_j, D> up to rounding alone"""
    W, phi, labels = _chain(N, single)
    target = 3 if single else None
    grads, _ = sm.site_gradient(W, phi, labels=labels, target_label=target)
    bnd = sm.bound(W, phi, labels=labels, target_label=target)
    rng = np.random.default_rng(N)
    worst = 0.
    for j in range(N):
        D = rng.standard_normal(W[j].shape)
        eps = sm.fd_eps(W[j], D)
        plus = [A if k != j else A + eps * D for k, A in enumerate(W)]
        minus = [A if k != j else A - eps * D for k, A in enumerate(W)]
        fd = (_cost(plus, phi, labels, target) - _cost(minus, phi, labels, target)) / (2 * eps)
        allowed = sm.fd_allowed(W, phi, labels, j, D, eps, bnd[j], target)        # from the model's abs contractions
        dev = abs(fd - (grads[j] * D).sum())
        worst = max(worst, dev / allowed)
        assert dev <= allowed, (j, fd, (grads[j] * D).sum(), dev, allowed)
        assert allowed < 1e-4 * max(abs(fd), np.abs(grads[j] * D).sum()), (j, allowed, fd)      # the check has teeth
    print("worst deviation / allowed", worst)


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("mode", ["labels", "coef"])
def test_euler_identity_at_every_site(mode, single):
    """W is linear in every site tensor: sum A_j G_j = sum_n sum_l c_nl W_l(x_n), whatever the site"""
    W, phi, labels = _chain(9, single)
    target = 3 if single else None
    nl = 1 if single else 10
    kw = dict(labels=labels, target_label=target) if mode == "labels" else dict(coef=np.random.default_rng(2).standard_normal((len(labels), nl)))
    grads, w = sm.site_gradient(W, phi, **kw)
    bnd = sm.bound(W, phi, **kw)
    _, w_abs, c_abs = sm.abs_gradient(W, phi, **kw)
    coef = kw["coef"] if mode == "coef" else 2. * (w - sm.targets(labels, nl, target))
    want = (coef * w).sum()
    K, _ = sm.rounding_counts(9, 9, len(labels), nl)
    for j in range(9):
        got = (W[j] * grads[j]).sum()
        allowed = (np.abs(W[j]) * bnd[j]).sum() + K * U * (c_abs * w_abs).sum()
        assert abs(got - want) <= allowed, (j, got, want, allowed)
        assert allowed < 1e-9 * (c_abs * w_abs).sum()


@pytest.mark.parametrize("N", [6, 9])
def test_one_image_with_a_one_hot_coefficient_is_the_site_response(N):
    """sum_{a, r} A_j[a, s, r] G_j[a, s, r] = phi_s resp[j][s] for the label the coefficient names"""
    W, phi, _ = _chain(N, False)
    for i, label in ((0, 4), (5, 0), (11, 9)):
        coef = np.zeros((1, 10))
        coef[0, label] = 1.
        grads, _ = sm.site_gradient(W, phi[i:i + 1], coef=coef)
        bnd = sm.bound(W, phi[i:i + 1], coef=coef)
        resp, _, _ = response(W, phi[i:i + 1], np.array([label]))
        for j in range(N):
            axes = (0, 2) if W[j].ndim == 3 else (0, 2, 3)
            got = (W[j] * grads[j]).sum(axis=axes)
            allowed = 2 * (np.abs(W[j]) * bnd[j]).sum(axis=axes)
            assert (np.abs(got - phi[i, j] * resp[0, j]) <= allowed).all(), (i, j, got, phi[i, j] * resp[0, j], allowed)


DEFECTS = ["drop_image", "swap_s", "argmax_seed", "no_factor2"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_exceed_the_bound_tenfold(defect):
    """on the data of tests/test_sitegrad_gpu.py: one image dropped from one site's sum, s swapped at one site, the seed built from
    which = argmax instead of the full c, the factor 2 of the labels mode missing -- the bound is not vacuous"""
    cases = [(sm.odd_case(0, 150), None), (sm.odd_case(1, 37), None), (sm.small_case(12, 5), None), (sm.small_case(4, 2), None),
             (dict(sm.small_case(12, 5), W=_plain(sm.small_case(12, 5)["W"])), 3)]
    for case, target in cases:
        for mode in (("labels",) if defect == "no_factor2" else ("labels", "coef")):
            for form in ("phi", "u8"):
                f = case["phi"] if form == "phi" else case["phi8"]
                kw = dict(labels=case["labels"], target_label=target) if mode == "labels" else dict(coef=case["coef"][:, :1 if target is not None else 10])
                good, _ = sm.site_gradient(case["W"], f, **kw)
                bad, _ = sm.site_gradient(case["W"], f, defect=defect, **kw)
                ratio = sm.worst_ratio(bad, good, sm.bound(case["W"], f, **kw))
                assert ratio >= 10., (defect, mode, form, len(case["W"]), ratio)


def _plain(W):
    """the per-label variant's W: no Label index"""
    return [A if A.ndim == 3 else A[..., 0] * 3.0 for A in W]
