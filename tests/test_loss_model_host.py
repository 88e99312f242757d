"""tests/loss_model.py (the numpy restatement of tnml_amd/csrc/loss_dev.h) held to mpmath at 200 bits, to its own structure, to
central differences of its cost through tests/sitegrad_model.py, and shown to tell planted defects apart.  No GPU.

The bound of the coefficients and costs (bounds())
--------------------------------------------------
u = 2^-53; an error of k ulp is a relative error of at most 2 k u.  For one image, x_l = fl(beta fl(w_l - m)) and p the exact softmax:
  * the subtraction and the product before the exponential shift the argument by at most 2 u |x_l|: e_l moves by 2 u |x_l| relatively;
  * exp_fixed <= 2 ulp: 4 u.                                          e_l:  eps_l = (2 |x_l| + 4) u
  * S adds ten positive terms with nine additions:                     S:    eps_S = sum_l p_l eps_l + 9 u
  * one quotient:                                                      p_l:  eps_l + eps_S + u
  * c_l = fl(beta fl(p_l - y_l)), two roundings:                       |dc_l| <= beta (p_l (eps_l + eps_S + u) + 2 u |p_l - y_l|)
    (an e_l the -708 branch sets to 0 is below 2^-1021 in truth: beta 2^-1021 is added)
  * C = fl(log_fixed(S) - x_y): log_fixed <= 4 ulp of log S (8 u log S), S's own error enters the logarithm as eps_S, x_y carries
    2 u |x_y|, the last subtraction u |C|:                             |dC| <= (8 log S + 2 |x_y| + |C|) u + eps_S
All of it to first order; bounds() multiplies by 1.01 for the higher orders.  No term is taken from a measured difference.
"""
import mpmath as mp
import numpy as np
import pytest

import eval_model as em
import loss_model as lm
import sitegrad_model as sm

U = 2.0 ** -53
mp.mp.prec = 200


def _ulps(got, true):
    """|got - true| in ulps of true (an mpf)"""
    t = float(true)
    return float(abs(mp.mpf(float(got)) - true) / mp.mpf(float(np.spacing(abs(t)))))


def test_exp_fixed_against_mpmath():
    below = np.nextafter(-708.0, -np.inf)
    assert lm.exp_fixed(np.array([below, -1e4, -np.inf])).tolist() == [0.0, 0.0, 0.0]
    half = []
    for j in (0, 1, 2, 3, 10, 57, 100, 511, 1000, 1020):                  # x LOG2E within an ulp of -(j + 1/2): rint at a tie
        x = -(j + 0.5) / lm.LOG2E
        half += [np.nextafter(x, -np.inf), x, np.nextafter(x, 0.0)]
    xs = np.concatenate([[0.0, -708.0, -1e-300, -2.0 ** -53, -2.0 ** -30, -1.0, -0.5 * np.log(2.0)], half, np.linspace(-708.0, 0.0, 4001),
                         -np.logspace(-12, 2.8, 500)])
    xs = xs[xs >= -708.0]
    got = lm.exp_fixed(xs)
    worst = max(_ulps(g, mp.exp(mp.mpf(float(x)))) for g, x in zip(got, xs))
    print("exp_fixed: %d arguments, largest error %.3f ulp" % (len(xs), worst))
    assert worst <= 2.0
    assert lm.exp_fixed(np.array([0.0]))[0] == 1.0
    # a dropped term and a wrong constant show as thousands of ulp
    assert max(_ulps(g, mp.exp(mp.mpf(float(x)))) for g, x in zip(lm.exp_fixed(xs, terms=10), xs)) > 1000


def test_log_fixed_against_mpmath():
    r2 = lm.SQRT2
    S = np.concatenate([[1.0, 1.0 + 2.0 ** -52, np.nextafter(r2, 0.0), r2, np.nextafter(r2, 2.0), 2 * r2, np.nextafter(2 * r2, 0.0), 4 * r2, 10.0,
                         np.nextafter(10.0, 0.0), 2.0, 4.0, 8.0], np.linspace(1.0, 10.0, 4001), 1.0 + np.logspace(-15, 0, 400)])
    got = lm.log_fixed(S)
    assert got[0] == 0.0
    worst = max(_ulps(g, mp.log(mp.mpf(float(s)))) for g, s in zip(got[1:], S[1:]))
    print("log_fixed: %d arguments, largest error %.3f ulp" % (len(S), worst))
    assert worst <= 4.0


def _weights(case):
    _, w = sm.site_gradient(case["W"], case["phi"], coef=np.zeros((len(case["labels"]), 10)))
    return w


CASES = {"small": lambda: sm.small_case(12, 5), "odd": lambda: sm.odd_case(1, 150)}


def _exact(w, labels, beta):
    """(c, C, p, x) in mpmath from the same fp64 weights"""
    n = len(labels)
    c, C, P, X = np.empty((n, 10), dtype=object), np.empty(n, dtype=object), np.empty((n, 10), dtype=object), np.empty((n, 10), dtype=object)
    for i in range(n):
        wi = [mp.mpf(float(v)) for v in w[i]]
        m = max(wi)
        x = [mp.mpf(beta) * (v - m) for v in wi]
        e = [mp.exp(v) for v in x]
        S = mp.fsum(e)
        for l in range(10):
            P[i, l] = e[l] / S
            X[i, l] = x[l]
            c[i, l] = mp.mpf(beta) * (P[i, l] - (1 if l == labels[i] else 0))
        C[i] = mp.log(S) - x[labels[i]]
    return c, C, P, X


def bounds(w, labels, beta):
    """(bound of c [n, 10], bound of C [n]) as the module's header derives them, from the exact quantities rounded to fp64"""
    c, C, P, X = _exact(w, labels, beta)
    p, x = P.astype(np.float64), np.abs(X.astype(np.float64))
    Cf = C.astype(np.float64)
    y = np.eye(10)[np.asarray(labels)]
    eps_l = (2 * x + 4) * U
    eps_S = (p * eps_l).sum(axis=1) + 9 * U
    logS = Cf + X.astype(np.float64)[np.arange(len(labels)), labels]
    bc = beta * (p * (eps_l + eps_S[:, None] + U) + 2 * U * np.abs(p - y)) + beta * 2.0 ** -1021
    bC = (8 * np.abs(logS) + 2 * x[np.arange(len(labels)), labels] + np.abs(Cf)) * U + eps_S
    return 1.01 * bc, 1.01 * bC, c, C


@pytest.mark.parametrize("beta", [1.0, 8.0])
@pytest.mark.parametrize("which", ["small", "odd"])
def test_coefficients_and_costs_against_mpmath(which, beta):
    case = CASES[which]()
    w, labels = _weights(case), case["labels"]
    bc, bC, c_true, C_true = bounds(w, labels, beta)
    c, C = lm.coefficients(w, labels, beta), lm.costs(w, labels, beta)
    err_c = np.array([[float(abs(mp.mpf(float(c[i, l])) - c_true[i, l])) for l in range(10)] for i in range(len(labels))])
    err_C = np.array([float(abs(mp.mpf(float(C[i])) - C_true[i])) for i in range(len(labels))])
    rc, rC = (err_c / bc).max(), (err_C / bC).max()
    print(which, "beta", beta, "largest error / bound: c %.4f, C %.4f" % (rc, rC))
    assert rc <= 1 and rC <= 1
    assert rc > 1e-3 and rC > 1e-3                               # (the bound is not vacuous)
    # structure: the coefficients of an image sum to zero, a cost is not negative
    total = c.sum(axis=1)
    assert (np.abs(total) <= bc.sum(axis=1) + 9 * U * np.abs(c).sum(axis=1)).all()
    assert (C >= 0).all()


@pytest.mark.parametrize("which", ["small", "odd"])
def test_a_constant_added_to_an_image_changes_nothing(which):
    """on weights rounded to multiples of 2^-20 the addition of 1024 is exact, and so is every w_l - m after it"""
    case = CASES[which]()
    w = np.round(_weights(case) * 2.0 ** 20) / 2.0 ** 20
    assert np.abs(w).max() < 2.0 ** 20
    shifted = w + 1024.0
    assert np.array_equal(shifted - 1024.0, w)
    for beta in (1.0, 8.0):
        assert np.array_equal(lm.coefficients(w, case["labels"], beta), lm.coefficients(shifted, case["labels"], beta))
        assert np.array_equal(lm.costs(w, case["labels"], beta), lm.costs(shifted, case["labels"], beta))
    assert np.array_equal(lm.decisions(w), lm.decisions(shifted))


def _total_cost(W, phi, labels, beta):
    _, w = sm.site_gradient(W, phi, coef=np.zeros((len(labels), 10)))
    return float(lm.costs(w, labels, beta).sum()), w


@pytest.mark.parametrize("beta", [1.0, 8.0])
def test_central_differences(beta):
    """<G_j, D> with G = site_gradient(coef = c) against the central difference of sum_n C_n along D, on three sites, the Label site
    among them.  Allowed: the rounding of the two costs over 2 eps and of G (fd_allowed's terms, restated for this cost: a cost moves
    by at most sum_l |c_l| |dw_l| + its own bound when its weights move by dw, |dw| <= Kc u Wabs) plus the third-order term of a cost that
    is not quadratic: along D the weights move linearly, w(t) = w + t delta, and the third derivative of log-sum-exp of beta w along
    delta is beta^3 times a third central moment of delta under the softmax, at most beta^3 R^3 with R = max_l delta_l - min_l delta_l;
    the central difference is off by eps^2 / 6 of it.  With the step halved that error falls by 4."""
    case = sm.small_case(12, 5)
    W, phi, labels = case["W"], case["phi"], case["labels"]
    n, N = len(labels), len(W)
    c0, w = _total_cost(W, phi, labels, beta)
    c = lm.coefficients(w, labels, beta)
    G, _ = sm.site_gradient(W, phi, coef=c)
    bnd = sm.bound(W, phi, coef=c)
    bc, bC, _, _ = bounds(w, labels, beta)
    absW = [np.abs(A) for A in W]
    g_dc, _, _ = sm._contract(absW, np.abs(phi), lambda ww: bc)     # c's own rounding, carried through the contraction
    m = max(max(A.shape[0], A.shape[2]) for A in W)
    _, Kc = sm.rounding_counts(N, m, n, 10)
    rng = np.random.default_rng(7)
    lab_site = N // 2 - 1
    for j in (1, lab_site, N - 2):
        D = rng.standard_normal(W[j].shape)
        eps = sm.fd_eps(W[j], D)
        errs = []
        for e in (eps, eps / 2):
            up, _ = _total_cost([A if k != j else A + e * D for k, A in enumerate(W)], phi, labels, beta)
            dn, _ = _total_cost([A if k != j else A - e * D for k, A in enumerate(W)], phi, labels, beta)
            errs.append((up - dn) / (2 * e) - float((G[j] * D).sum()))
        wide = [a if k != j else a + eps * np.abs(D) for k, a in enumerate(absW)]
        _, w_abs, _ = sm._contract(wide, np.abs(phi), lambda ww: np.zeros_like(ww))
        cost_round = (2 * beta * Kc * U * w_abs.max(axis=1) + bC).sum() + (n + 2) * U * c0
        rounding = 2 * cost_round / (2 * eps) + ((bnd[j] + g_dc[j]) * np.abs(D)).sum()
        _, delta = sm.site_gradient([A if k != j else D for k, A in enumerate(W)], phi, coef=np.zeros((n, 10)))
        R = delta.max(axis=1) - delta.min(axis=1)
        third = eps ** 2 / 6 * beta ** 3 * float((R ** 3).sum())
        print("site", j, "beta", beta, "eps", eps, "error", errs[0], "halved", errs[1], "ratio", errs[0] / errs[1], "rounding", rounding, "third order", third)
        assert abs(errs[0]) <= rounding + third
        assert 3 <= errs[0] / errs[1] <= 5


def test_planted_defects():
    """each lands at least 10 bounds from the model"""
    case = sm.small_case(12, 5)
    labels = case["labels"]
    w = np.round(_weights(case) * 2.0 ** 20) / 2.0 ** 20
    beta = 8.0
    bc, bC, _, _ = bounds(w, labels, beta)
    c, C = lm.coefficients(w, labels, beta), lm.costs(w, labels, beta)

    def away(got, want, bnd):
        with np.errstate(invalid="ignore"):
            r = np.abs(got - want) / bnd
        return float(np.where(np.isnan(r), np.inf, r).max())

    # the max is not subtracted: the same numbers in exact arithmetic, an overflow once the weights sit 1024 higher (an exact shift)
    far = away(lm.coefficients(w + 1024.0, labels, beta, defect="no_max"), c, bc)
    print("no_max", far)
    assert far >= 10
    for defect in ("y_at_pred", "beta_once"):
        far = away(lm.coefficients(w, labels, beta, defect=defect), c, bc)
        print(defect, far)
        assert far >= 10
    assert (em.predictions(w) != labels).any()
    far = away(lm.costs(w, labels, beta, defect="sign_xy"), C, bC)
    print("sign_xy", far)
    assert far >= 10
    # the |W| rule in place of the signed decision: integers, compared exactly
    _, _, wd = lm.decision_set(case["W"], case["phi"])
    lab = labels
    differ = lm.decisions(wd) != em.predictions(wd)
    assert differ.any() and not differ.all()
    good, bad = lm.report(wd, lab, beta), lm.report(wd, lab, beta, decision=em.predictions)
    assert not np.array_equal(good["confusion"], bad["confusion"])
    assert good["cost"] == bad["cost"]
