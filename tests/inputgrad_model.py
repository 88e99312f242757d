"""Input gradients restated in numpy (fp64): the yardstick of tests/test_inputgrad_gpu.py, itself proved by
tests/test_inputgrad_model_host.py (the oracle's forward pass on modified features, the Euler tie, the tie to tests/response_model.py).

For n images and coefficients c[n, l] = dC/dW_l(x_n)

    dphi[n, j, s] = sum_{a, r} L_j[n, a] A_j[a, s, r] Xr_j[n, r]                  (j left of the Label site c)
    dphi[n, j, s] = sum_{a, r} Yl_j[n, a] A_j[a, s, r] R_j[n, r]                  (j right of it)
    dphi[n, c, s] = sum_l c[n, l] sum_{a, r} L_c[n, a] A_c[a, s, r, l] R_c[n, r]

with the explicit environments of tests/sitegrad_model.py: L_j everything left of site j, R_j everything right of it (Label-free), Xr_j
everything right of site j with the Label site's tensor contracted with c, Yl_j everything left of site j likewise.  Sites are 0-based
here.  W is a list of N arrays [ml, 2, mr]; at most one of them, the Label site, is [ml, 2, mr, nl].  Without one (the per-label variant)
there is a single output and site 0 plays the Label site.

The bound
---------
Every dphi[n, j, s] is a sum of products of one factor per site and a coefficient, so a first-order rounding analysis bounds its error
by K 2^-53 x the same contraction on |c|, |A| and |phi| (and so on |L|, |X|, ..: abs_input_gradient), K the number of roundings on the
longest path from the inputs to an element.  For the device's order (kernels_inputgrad.hip behind k_site_backward of
kernels_sitegrad.hip), with N sites, m the largest bond and nl labels, counting a rounding for every product and one for every addition:
  * the tape vectors on both sides of site j have crossed every other site by a chain step, which forms fl(phi_s v[k]) (1 rounding)
    and accumulates 2 m such terms: at most 4 m + 1 roundings a step, (N - 1)(4 m + 1) in all;
  * when the path crosses the Label site (j is not it), the seed there accumulates nl labels in one chain step, (nl - 1) 4 m further
    terms, and forms fl(c phi_s): + 1;
  * site j itself: P_s accumulates at most m terms, a product and an addition each -- at the Label site nl m terms, each with the
    product fl(c R[r]) in front: at most 3 nl m; the dot over a takes at most m fused multiply-adds (counted as 2 m), then 3 additions
    over the lane groups and 8 over the waves: 2 m + 11.
K_dev = (N - 1)(4 m + 1) + (nl - 1) 4 m + 1 + 3 nl m + 2 m + 11.
The other side of a comparison is the model (einsum / tensordot sums of the same term counts in another order: no more than K_dev) or
the oracle's forward pass on modified features followed by the sum over the labels, K_w + 2 nl roundings with K_w = N (4 m + 1) + 2 m + 1
the count of a weight (tests/sitegrad_model.py).  rounding_count is K_dev + max(K_dev, K_w + 2 nl), which covers either.
In the labels mode c = 2 (W - y) carries the error of the weight itself, |dc| <= 2 (2 K_w + 1) 2^-53 (Wabs + |y|) as in
tests/sitegrad_model.py; the same contraction on |dc| is added."""
import numpy as np

import sitegrad_model as sm

U = 2.0 ** -53

DEFECTS = ("drop_label", "inward_for_Y", "swap_s", "bond_off_by_one")


def _fit(v, dim):
    """v[n, d] cut or padded with zeros to [n, dim]: what reading dim rows of another bond's vector gives"""
    out = np.zeros((v.shape[0], dim))
    k = min(dim, v.shape[1])
    out[:, :k] = v[:, :k]
    return out


def _contract(W, phi, coef_of, defect=None):
    """the contraction on W and phi as given; coef_of(weights) -> c[n, nl].  -> (dphi[n, N, 2], weights[n, nl], c)"""
    n, N = phi.shape[0], len(W)
    assert phi.shape == (n, N, 2)
    lab_sites = [j for j, A in enumerate(W) if A.ndim == 4]
    assert len(lab_sites) <= 1
    c = lab_sites[0] if lab_sites else 0
    Wc = W[c] if lab_sites else W[c][..., None]
    nl = Wc.shape[3]
    M = [np.tensordot(phi[:, j], W[j], axes=(1, 1)) if j != c else None for j in range(N)]          # [n, a, r]
    L = [np.ones((n, 1))]
    for j in range(c):
        L.append(np.einsum("na,nar->nr", L[-1], M[j]))
    R = {N - 1: np.ones((n, 1))}
    for j in range(N - 1, c, -1):
        R[j - 1] = np.einsum("nar,nr->na", M[j], R[j])
    LA = np.tensordot(L[c], Wc, axes=(1, 0))                                       # [n, s, r, l]
    LAR = np.einsum("nsrl,nr->nsl", LA, R[c])                                      # [n, s, l]
    weights = np.einsum("ns,nsl->nl", phi[:, c], LAR)
    coef = np.asarray(coef_of(weights), dtype=np.float64)
    assert coef.shape == (n, nl), coef.shape
    Xr, Yl = {}, {}
    if c > 0:
        AR = np.tensordot(R[c], Wc, axes=(1, 2))                                   # [n, a, s, l]
        Xr[c - 1] = np.einsum("nl,ns,nasl->na", coef, phi[:, c], AR)
        for j in range(c - 1, 0, -1):
            Xr[j - 1] = np.einsum("nar,nr->na", M[j], Xr[j])
    if c < N - 1:
        Yl[c + 1] = np.einsum("nl,ns,nsrl->nr", coef, phi[:, c], LA)
        for j in range(c + 1, N - 1):
            Yl[j + 1] = np.einsum("na,nar->nr", Yl[j], M[j])
    dphi = np.zeros((n, N, 2))
    for j in range(N):
        if j == c:
            cc = coef
            if defect == "drop_label":                                             # the last label's term is left out at the centre
                cc = coef.copy()
                cc[:, -1] = 0.
            dphi[:, j] = np.einsum("nl,nsl->ns", cc, LAR)
            continue
        if j < c:
            left, right = L[j], Xr[j]
            if defect == "bond_off_by_one" and j == c - 2:                         # the r side taken from the next bond
                right = _fit(Xr[j + 1], right.shape[1])
        else:
            left, right = Yl[j], R[j]
            if defect == "inward_for_Y" and j == c + 1:                            # the inward tape's vector on that bond where the outward one belongs
                left = R[j - 1]
            if defect == "bond_off_by_one" and c < 2 and j == c + 1 and j + 1 < N:   # (no site two left of the centre: the same on the right)
                right = _fit(R[j + 1], right.shape[1])
        d = np.einsum("nsr,nr->ns", np.tensordot(left, W[j], axes=(1, 0)), right)
        if defect == "swap_s" and j == (c + 1 if c + 1 < N else c - 1):
            d = d[:, ::-1]
        dphi[:, j] = d
    return dphi, weights, coef


def input_gradient(W, phi, coef=None, labels=None, target_label=None, defect=None):
    """-> (dphi[n, N, 2], weights[n, nl]).  Exactly one of coef[n, nl] and labels[n] (then c = 2 (weights - y), y by
    sitegrad_model.targets()).  defect: one of DEFECTS, the planted defects of test_inputgrad_model_host.py."""
    assert (coef is None) != (labels is None)
    assert defect is None or defect in DEFECTS
    W = [np.asarray(A, dtype=np.float64) for A in W]
    phi = np.asarray(phi, dtype=np.float64)
    if coef is not None:
        coef_of = lambda w: np.asarray(coef, dtype=np.float64)
    else:
        coef_of = lambda w: 2. * (w - sm.targets(labels, w.shape[1], target_label))
    dphi, weights, _ = _contract(W, phi, coef_of, defect)
    return dphi, weights


def rounding_count(N, m, nl):
    """K of the comparison of the device's dphi with the model's, or of either with the oracle's forward pass: see the module's header"""
    k_dev = (N - 1) * (4 * m + 1) + (nl - 1) * 4 * m + 1 + 3 * nl * m + 2 * m + 11
    k_w = N * (4 * m + 1) + 2 * m + 1
    return k_dev + max(k_dev, k_w + 2 * nl)


def abs_input_gradient(W, phi, coef=None, labels=None, target_label=None):
    """the same contraction on |A|, |phi| and |c| (labels mode: c of the true contraction) -> (dphi_abs, weights_abs, |c|)"""
    W = [np.asarray(A, dtype=np.float64) for A in W]
    phi = np.asarray(phi, dtype=np.float64)
    if coef is None:
        _, w = input_gradient(W, phi, labels=labels, target_label=target_label)
        coef = 2. * (w - sm.targets(labels, w.shape[1], target_label))
    c_abs = np.abs(np.asarray(coef, dtype=np.float64))
    d, w_abs, _ = _contract([np.abs(A) for A in W], np.abs(phi), lambda w: c_abs)
    return d, w_abs, c_abs


def bound(W, phi, coef=None, labels=None, target_label=None):
    """elementwise bound [n, N, 2] on |dphi_a - dphi_b| between two fp64 evaluations"""
    W = [np.asarray(A, dtype=np.float64) for A in W]
    N = len(W)
    m = max(max(A.shape[0], A.shape[2]) for A in W)
    d_abs, w_abs, c_abs = abs_input_gradient(W, phi, coef, labels, target_label)
    nl = c_abs.shape[1]
    out = rounding_count(N, m, nl) * U * d_abs
    if labels is not None:                                                         # c's own error, carried through the same contraction
        _, Kc = sm.rounding_counts(N, m, 1, nl)
        dc = 2. * Kc * U * (w_abs + sm.targets(labels, nl, target_label))
        out = out + _contract([np.abs(A) for A in W], np.abs(np.asarray(phi, dtype=np.float64)), lambda w: dc)[0]
    return out


def worst_ratio(got, want, bnd):
    """max |got - want| / bound (0 / 0 counts as 0)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == bnd.shape, (got.shape, want.shape, bnd.shape)
    d = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0, 0., d / bnd).max())


_CACHE = {}


def model_of(case, form, mode, target_label=None):
    """(dphi, weights, bound) of the model on a case of tests/sitegrad_model.py, once per (case, input form, mode)"""
    key = (id(case), form, mode, target_label)
    if key not in _CACHE:
        f = case["phi"] if form == "phi" else case["phi8"]
        kw = dict(labels=case["labels"], target_label=target_label) if mode == "labels" else dict(coef=case["coef"][:, :1 if target_label is not None else 10])
        d, w = input_gradient(case["W"], f, **kw)
        _CACHE[key] = (d, w, bound(case["W"], f, **kw), case)                      # (the case is kept alive: its id is the key)
    return _CACHE[key][:3]
