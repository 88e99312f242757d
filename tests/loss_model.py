"""The softmax cross-entropy of tnml_amd/csrc/loss_dev.h restated in numpy (fp64), operation for operation: every line below is one IEEE
rounding, as on the device, so that the comparisons of tests/test_loss_gpu.py are bit for bit.  tests/test_loss_model_host.py holds
this file to mpmath.

    exp_fixed(x), x <= 0     0 below -708; k = rint(x LOG2E), r = (x - k LN2_HI) - k LN2_LO, Horner of sum_{n<=13} r^n / n!, ldexp(p, k)
    log_fixed(S), 1..10      halve while S >= sqrt 2 (k times); f = (S - 1) / (S + 1), z = f f; Horner of sum_{n<=11} z^n / (2 n + 1);
                             k LN2 + (2 f) q
    per image                m = first maximum of w_l; d = the first l with w_l == m; x_l = beta (w_l - m); e_l = exp_fixed(x_l);
                             S = e_0 + ... + e_9 left to right; p_l = e_l / S; c_l = beta (p_l - [l == y]); C = log_fixed(S) - x_y
A weight that is not finite makes the image's c and C NaN.
"""
import math

import numpy as np

NL = 10
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
E = [1.0 / float(math.factorial(n)) for n in range(14)]
L = [1.0 / float(2 * n + 1) for n in range(12)]


def exp_fixed(x, terms=14):
    """elementwise; x <= 0 (or -inf).  terms: a planted defect drops the highest ones"""
    x = np.asarray(x, dtype=np.float64)
    small = x < -708.0
    xs = np.where(small, 0.0, x)
    k = np.rint(xs * LOG2E)
    r = (xs - k * LN2_HI) - k * LN2_LO
    p = np.full_like(xs, E[terms - 1])
    for n in range(terms - 2, -1, -1):
        p = p * r
        p = p + E[n]
    return np.where(small, 0.0, np.ldexp(p, k.astype(np.int64)))


def log_fixed(S):
    """elementwise; 1 <= S <= 10"""
    S = np.array(S, dtype=np.float64)
    k = np.zeros_like(S)
    for _ in range(4):
        big = S >= SQRT2
        S = np.where(big, 0.5 * S, S)
        k = np.where(big, k + 1.0, k)
    assert not (S >= SQRT2).any()
    f = (S - 1.0) / (S + 1.0)
    z = f * f
    q = np.full_like(S, L[11])
    for n in range(10, -1, -1):
        q = q * z
        q = q + L[n]
    return k * LN2 + (2.0 * f) * q


def decisions(w):
    """the signed decision d: the first maximum of w_l (0 when the maximum is NaN)"""
    w = np.asarray(w, dtype=np.float64)
    m = w[:, 0].copy()
    for l in range(1, NL):
        m = np.where(w[:, l] > m, w[:, l], m)
    d = np.zeros(len(w), dtype=np.int32)
    for l in range(NL - 1, -1, -1):
        d = np.where(w[:, l] == m, l, d)
    return d.astype(np.int32)


def _block(w, labels, beta, defect=None):
    """-> (c[n, 10], C[n], e[n, 10]); defect: one of the planted defects of test_loss_model_host.py"""
    w = np.asarray(w, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    n = len(lab)
    assert w.shape == (n, NL), w.shape
    finite = np.isfinite(w).all(axis=1)
    ws = np.where(finite[:, None], w, 0.0)
    m = ws[:, 0].copy()
    for l in range(1, NL):
        m = np.where(ws[:, l] > m, ws[:, l], m)
    if defect == "no_max":                                     # (arguments above 0: numpy's exp and log stand in for the fixed ones)
        m = np.zeros_like(m)
    x = beta * (ws - m[:, None])
    with np.errstate(over="ignore", invalid="ignore"):
        e = exp_fixed(x) if defect != "no_max" else np.exp(x)
        S = e[:, 0].copy()
        for l in range(1, NL):
            S = S + e[:, l]
        p = e / S[:, None]
    if defect == "y_at_pred":
        lab = np.abs(ws).argmax(axis=1)
    y = np.eye(NL)[lab]
    c = (p - y) if defect == "beta_once" else beta * (p - y)
    xy = x[np.arange(n), lab]
    logS = log_fixed(S) if defect != "no_max" else np.log(S)
    C = (logS + xy) if defect == "sign_xy" else (logS - xy)
    c = np.where(finite[:, None], c, np.nan)
    C = np.where(finite, C, np.nan)
    return c, C, e


def coefficients(w, labels, beta, defect=None):
    return _block(w, labels, beta, defect)[0]


def costs(w, labels, beta, defect=None):
    return _block(w, labels, beta, defect)[1]


def exponentials(w, beta):
    """e[n, 10]: what a test needs to see the -708 branch taken"""
    return _block(w, np.zeros(len(w), dtype=np.int64), beta)[2]


def device_order_label_cost(C, labels, chunk=8192, threads=256):
    """label_cost in k_eval_tally's order (the structure of eval_model.device_order_label_cost) from the images' costs C[n]"""
    C = np.asarray(C, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    total = np.zeros(NL)
    for off in range(0, len(lab), chunk):
        s = np.zeros((threads, NL))
        for i in range(off, min(off + chunk, len(lab))):
            s[(i - off) % threads, lab[i]] += C[i]
        stride = threads // 2
        while stride > 0:
            s[:stride] += s[stride:2 * stride]
            stride //= 2
        total += s[0]
    return total


def report(w, labels, beta, chunk=8192, threads=256, decision=None):
    """dict with the fields of tnml_eval_report under loss = 1, costs in the device's order; decision: a planted defect puts another
    rule in place of decisions()"""
    w = np.asarray(w, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    n = len(lab)
    d = decisions(w) if decision is None else decision(w)
    label_cost = device_order_label_cost(costs(w, lab, beta), lab, chunk, threads)
    cost = 0.0
    for x in label_cost.tolist():
        cost += x
    wrong = d != lab
    confusion = np.zeros((NL, NL), dtype=np.int64)
    np.add.at(confusion, (lab, d), 1)
    return dict(n=n, ncorrect=int((~wrong).sum()), cost=cost, label_cost=label_cost, count=np.bincount(lab, minlength=NL).astype(np.int64),
                nincorrect=np.bincount(lab[wrong], minlength=NL).astype(np.int64), confusion=confusion)


def same_report(rep, want):
    """an EvalReport of tnml_amd.fixedl against report()'s dict: costs bit for bit, the integers exact"""
    for f in want:
        assert np.array_equal(np.asarray(getattr(rep, f)), np.asarray(want[f])), (f, getattr(rep, f), want[f])


def decision_set(W, phi):
    """the set of the decision tests: W with one label slice of the Label site times -3, the first slice for which, on the weights
    of tests/sitegrad_model.py, the signed decision differs from the first maximum of |w_l| on at least one image and on fewer than
    all -> (the slice, that W, the model's weights)"""
    import eval_model as em
    import sitegrad_model as sm
    c = [j for j, A in enumerate(W) if A.ndim == 4][0]
    for l0 in range(NL):
        V = [np.array(A, dtype=np.float64) for A in W]
        V[c][..., l0] *= -3.0
        _, w = sm.site_gradient(V, phi, coef=np.zeros((len(phi), NL)))
        differ = decisions(w) != em.predictions(w)
        if differ.any() and not differ.all():
            return l0, V, w
    raise AssertionError("no label slice separates the two decision rules")
