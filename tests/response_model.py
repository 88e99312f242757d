"""Site responses restated in numpy (fp64): the yardstick of tests/test_response_gpu.py, itself held to the oracle by
tests/test_response_model_host.py.

For image n and label l, resp[n, j, s] is the contraction of W with label index l and the features of the image on every site but j
(0-based here), site j getting the unit vector e_s.  The model keeps explicit lists of the left and right environments of every
image: Lf[j] is everything left of site j, Rf[j] everything right of it, both with the chosen label contracted in, so that

    resp[n, j, s] = sum_{a, r} Lf[j][n, a] A_j[a, s, r] Rf[j][n, r].

W is a list of N arrays [ml, 2, mr]; at most one of them, the Label site, is [ml, 2, mr, nl].  Without one (the per-label
variant) there is a single output and `which` must be None or all zero.

The bound
---------
Every resp[n, j, s] is a sum of products of one factor per site, so a first-order rounding analysis bounds its error by K 2^-53 x the
same contraction on absolute values, K the number of roundings on the longest path from the inputs to an element.  For the device's
order (kernels_response.hip), with N sites and m the largest bond, counting a rounding for every product and one for every addition:
  * every site but j is crossed by a chain step.  An inward step (chain_step) forms fl(phi_s v[k]) and accumulates 2 m such terms: at
    most 4 m + 1 roundings.  An outward step forms U_s from m terms (2 m) and fl(fl(phi_0 U_0) + fl(phi_1 U_1)) (2): 2 m + 2, no more
    than 4 m + 1.  The Label site, when it is not site j, is one outward step on the chosen label: (N - 1)(4 m + 1);
  * site j itself: U_s from m terms (2 m), then the dot with the environment over at most m rows: an fma per row of a lane (at most 4
    per row tile), three additions over the q groups, one per row tile of the wave, eight over the waves -- never more than the 2 m of a
    product and an addition per term, + 16 for the fixed additions when m is small: 4 m + 16.
K_dev = (N - 1)(4 m + 1) + 4 m + 16.  The model's einsum / tensordot sums have the same term counts in another order and no more
roundings than that: the comparison of the two is bounded with K = 2 K_dev."""
import numpy as np

U = 2.0 ** -53


def _site_matrices(A, phi_j):
    """M[n, a, r(, l)] = sum_s phi_j[n, s] A[a, s, r(, l)]"""
    return np.tensordot(phi_j, A, axes=(1, 1))


def response(W, phi, which=None):
    """-> (resp[n, N, 2], weights[n, nl], label[n]); label is which, or the first maximum of |weights| when which is None"""
    W = [np.asarray(A, dtype=np.float64) for A in W]
    phi = np.asarray(phi, dtype=np.float64)
    n, N = phi.shape[0], len(W)
    assert phi.shape == (n, N, 2)
    lab_sites = [j for j, A in enumerate(W) if A.ndim == 4]
    assert len(lab_sites) <= 1
    c = lab_sites[0] if lab_sites else 0
    Wc = W[c] if lab_sites else W[c][..., None]
    nl = Wc.shape[3]
    M = [_site_matrices(W[j], phi[:, j]) for j in range(N)]                       # (unused at the Label site)
    # Label-free environments up to the Label site
    L = [np.ones((n, 1))]
    for j in range(c):
        L.append(np.einsum("na,nar->nr", L[-1], M[j]))
    R = {N - 1: np.ones((n, 1))}
    for j in range(N - 1, c, -1):
        R[j - 1] = np.einsum("nar,nr->na", M[j], R[j])
    LA = np.tensordot(L[c], Wc, axes=(1, 0))                                      # [n, s, r, l]
    LAR = np.einsum("nsrl,nr->nsl", LA, R[c])                                     # [n, s, l]
    weights = np.einsum("ns,nsl->nl", phi[:, c], LAR)
    if which is None:
        label = np.abs(weights).argmax(axis=1) if lab_sites else np.zeros(n, dtype=np.int64)
    else:
        label = np.asarray(which, dtype=np.int64)
        assert label.shape == (n,) and (label >= 0).all() and (label < nl).all()
    rows = np.arange(n)
    # the lists of environments with the chosen label: Lf[j] left of site j, Rf[j] right of it
    Lf = L[:c + 1] + [None] * (N - c - 1)
    if c + 1 < N:
        Lf[c + 1] = np.einsum("ns,nsr->nr", phi[:, c], LA[rows, :, :, label])
    for j in range(c + 1, N - 1):
        Lf[j + 1] = np.einsum("na,nar->nr", Lf[j], M[j])
    Rf = [None] * N
    for j in range(c, N):
        Rf[j] = R[j]
    if c > 0:
        AR = np.tensordot(R[c], Wc, axes=(1, 2))                                  # [n, a, s, l]
        Rf[c - 1] = np.einsum("ns,nas->na", phi[:, c], AR[rows, :, :, label])
    for j in range(c - 1, 0, -1):
        Rf[j - 1] = np.einsum("nar,nr->na", M[j], Rf[j])
    resp = np.zeros((n, N, 2))
    for j in range(N):
        if j == c:
            resp[:, j] = LAR[rows, :, label]
        else:
            resp[:, j] = np.einsum("nsr,nr->ns", np.tensordot(Lf[j], W[j], axes=(1, 0)), Rf[j])
    return resp, weights, label.astype(np.int32)


def rounding_count(N, m):
    """K of the comparison of two fp64 evaluations of resp (the device's and the model's): see the module's header"""
    return 2 * ((N - 1) * (4 * m + 1) + 4 * m + 16)


def bound(W, phi, label):
    """elementwise bound [n, N, 2] on |resp_a - resp_b| between two fp64 evaluations for the labels `label` (as response() returns
    them): K 2^-53 x the same contraction on |A| and |phi|"""
    W = [np.abs(np.asarray(A, dtype=np.float64)) for A in W]
    m = max(max(A.shape[0], A.shape[2]) for A in W)
    lab = None if not any(A.ndim == 4 for A in W) else np.asarray(label)
    return rounding_count(len(W), m) * U * response(W, np.abs(np.asarray(phi, dtype=np.float64)), lab)[0]
