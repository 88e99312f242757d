"""The arithmetic of a gradient step on the device (tnml_site_step_u8 / tnml_site_step_phi, kernels_sitestep.hip) restated in numpy:
the yardstick of tests/test_sitestep_gpu.py, itself checked by tests/test_sitestep_model_host.py.  A function of (W, flat gradient,
state, parameters) and nothing else.

Every operation is one IEEE fp64 rounding, as numpy's elementwise +, -, *, / and sqrt on float64 arrays are (none of them fuses two
operations, quotient and root are correctly rounded).  g is the flat gradient: the sites concatenated in site order, each flattened
first index fastest (order="F"), as tnml_site_gradient_* lays grad out; m and v have the same layout.

  1. total: g is cut into consecutive blocks of STEP_NORM_BLOCK = 65 536 elements.  In a block, 256 partial sums start from 0; partial
     sum t adds fl(g g) of the block's elements t, t + 256, ... in ascending order; the 256 are joined by a tree (stride 128, ..., 1:
     element t += element t + stride); the block sums are added in block order, starting from 0.
  2. grad_norm = fl(|scale| fl(sqrt(total)));  f = scale, unless clip > 0 and grad_norm > clip: then f = fl(scale fl(clip / grad_norm)),
     clipped.  gh = fl(f g).
  3. sgd:   v <- fl(fl(mu v) + gh);  A <- fl(A - fl(lr v))
  4. adam:  p1 <- fl(p1 beta1), p2 <- fl(p2 beta2) (both start at 1); c1 = fl(1 - p1), c2 = fl(1 - p2), o1 = fl(1 - beta1), o2 = fl(1 - beta2);
            m <- fl(fl(beta1 m) + fl(o1 gh));  v <- fl(fl(beta2 v) + fl(fl(o2 gh) gh));
            A <- fl(A - fl(lr fl(fl(m / c1) / fl(fl(sqrt(fl(v / c2))) + eps))))
  5. total not finite: nothing is applied, W, the state and t stay as they were (step() returns applied = False).

The bound of the ordered norm (norm_bound)
------------------------------------------
Every term fl(g g) carries one rounding, and on its way into the total it passes through at most
    D = 255 (its partial sum: at most 256 terms) + 8 (the tree) + (B - 1) (B block sums) additions,
each one rounding of a sum of non-negative terms.  So total = sum g^2 (1 + d), |d| <= (1 + u)^(D + 1) - 1 =: gamma_total, u = 2^-53.
math.fsum of the rounded squares is the exact sum rounded once and carries the squares' roundings too: the two differ by at most
(gamma_total + 2 u) x sum g^2 to first order; norm_bound returns (D + 3) u (1 + 1e-9), the first-order count with room for the higher
orders (D u < 1e-12).  The root halves a relative error and adds a rounding, the product with |scale| one more:
|grad_norm - |scale| sqrt(sum g^2)| <= (gamma / 2 + 2 u) grad_norm.

The bound of Adam against another formulation (AdamBound)
---------------------------------------------------------
torch.optim.Adam (fp64, one tensor, no amsgrad, no weight decay) computes the same quantities in another order:
    m <- m + (g - m)(1 - beta1);  v <- beta2 v, v <- v + (1 - beta2) g g;  bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (pow);
    A <- A + (-(lr / bc1)) m / (sqrt(v) / sqrt(bc2) + eps).
For the same gradients (they do not depend on A here) the difference of the two A is bounded step by step, elementwise, to first
order in u with every count doubled (one formulation's roundings on each side):
  m:  at most four roundings each (ours: two products and a sum; torch's lerp: a difference, a product and a sum, and for a weight
      of 1/2 or more the complement of the weight as well), every intermediate at most |m| + |g| in magnitude, and an earlier
      difference is carried on with the factor beta1 in both:                                              dm <- beta1 dm + 8 u (|m| + |g|).
  v:  four roundings each, all terms non-negative and at most v + g^2:                                     dv <- beta2 dv + 8 u (v + g^2).
  c1: ours has t - 1 roundings in p1 and one in 1 - p1, torch one in pow (taken as within 1 ulp) and one in 1 - pow:
      |dc1| <= ((t + 1) p1 + 2 c1) u, likewise c2.  The cancellation in 1 - p is in the bound, not hidden: p / c is 999 for beta2 = 0.999.
  update U = lr (m / c1) / (sqrt(v / c2) + eps): at most eight roundings in either formulation (quotients, roots, the sum with eps,
      the products), each a relative error u of U or less, since sqrt halves relative errors and eps > 0 only damps them: 16 u |U|;
      from dm: lr dm / (c1 den);  from dc1: |U| dc1 / c1;  from v and c2 through the root r = sqrt(v / c2):
      dr <= min(sqrt(dv / c2), dv / (2 sqrt(v c2))) + r dc2 / (2 c2), contributing |U| dr / den (den = r + eps).
  A:  one rounding of the final difference on each side: 2 u |A|.
The sum over the steps, times 1.01 for the higher orders, is the bound; no term of it is taken from a measured difference.
"""
import math

import numpy as np

U = 2.0 ** -53
STEP_NORM_BLOCK = 65536
STEP_THREADS = 256


def flat(arrays):
    """a list of site arrays -> the flat layout of grad"""
    return np.concatenate([np.asarray(a, dtype=np.float64).ravel(order="F") for a in arrays])


def unflat(x, like):
    out, at = [], 0
    for a in like:
        out.append(x[at:at + a.size].reshape(a.shape, order="F").copy(order="F"))
        at += a.size
    assert at == x.size
    return out


def ordered_sumsq(g):
    """total of step 1, in the device's order"""
    g = np.asarray(g, dtype=np.float64).ravel()
    E = g.size
    nblk = max(1, -(-E // STEP_NORM_BLOCK))
    sq = np.zeros(nblk * STEP_NORM_BLOCK)
    with np.errstate(over="ignore"):
        sq[:E] = g * g                                        # beyond the end: + 0, which changes no partial sum (they are >= +0)
    sq = sq.reshape(nblk, STEP_NORM_BLOCK // STEP_THREADS, STEP_THREADS)      # [block][k][t]: element t + 256 k
    part = np.zeros((nblk, STEP_THREADS))
    for k in range(sq.shape[1]):
        part = part + sq[:, k, :]
    stride = STEP_THREADS // 2
    while stride > 0:
        part[:, :stride] = part[:, :stride] + part[:, stride:2 * stride]
        stride //= 2
    total = np.float64(0.)
    for b in range(nblk):
        total = total + part[b, 0]
    return float(total)


def norm_bound(E):
    """relative bound on |ordered_sumsq(g) - math.fsum(g g)|: see the module's header"""
    nblk = max(1, -(-E // STEP_NORM_BLOCK))
    depth = (STEP_NORM_BLOCK // STEP_THREADS - 1) + 8 + (nblk - 1)
    return (depth + 3) * U * (1 + 1e-9)


def factor(total, scale, clip):
    """step 2 -> (grad_norm, f, clipped)"""
    scale, clip = np.float64(scale), np.float64(clip)
    with np.errstate(all="ignore"):
        grad_norm = np.abs(scale) * np.sqrt(np.float64(total))
        if clip > 0 and grad_norm > clip:
            return float(grad_norm), float(scale * (clip / grad_norm)), True
    return float(grad_norm), float(scale), False


def new_state(method, E):
    """the state the first step makes: zeros, t = 0, both powers 1"""
    assert method in ("sgd", "adam")
    st = dict(method=method, t=0, p1=1., p2=1., v=np.zeros(E))
    if method == "adam":
        st["m"] = np.zeros(E)
    return st


def step(W, g, state, method="sgd", lr=None, momentum=0., beta1=.9, beta2=.999, eps=1e-8, clip=0., scale=1.):
    """one step: (W_new as a list shaped like W, new state, report); W, g and state are not modified.
    report: dict(t, grad_norm, factor, clipped, applied)"""
    assert state["method"] == method
    g = np.asarray(g, dtype=np.float64).ravel()
    A = flat(W)
    assert A.shape == g.shape == state["v"].shape
    total = ordered_sumsq(g)
    grad_norm, f, clipped = factor(total, scale, clip)
    if not math.isfinite(total):
        return [np.array(a, dtype=np.float64, order="F") for a in W], state, dict(t=state["t"], grad_norm=grad_norm, factor=f, clipped=clipped, applied=False)
    lr, f = np.float64(lr), np.float64(f)
    gh = f * g
    st = dict(state, t=state["t"] + 1)
    if method == "sgd":
        v = np.float64(momentum) * state["v"] + gh
        A = A - lr * v
        st["v"] = v
    else:
        b1, b2 = np.float64(beta1), np.float64(beta2)
        p1, p2 = np.float64(state["p1"]) * b1, np.float64(state["p2"]) * b2
        c1, c2, o1, o2 = np.float64(1.) - p1, np.float64(1.) - p2, np.float64(1.) - b1, np.float64(1.) - b2
        m = b1 * state["m"] + o1 * gh
        v = b2 * state["v"] + (o2 * gh) * gh
        A = A - lr * ((m / c1) / (np.sqrt(v / c2) + np.float64(eps)))
        st.update(m=m, v=v, p1=float(p1), p2=float(p2))
    return unflat(A, W), st, dict(t=st["t"], grad_norm=grad_norm, factor=f.item(), clipped=clipped, applied=True)


class AdamBound:
    """elementwise bound on the difference of A between this model's Adam and another fp64 formulation fed the same gradients (no
    clipping, scale 1): see the module's header.  Feed it every step's quantities as this model has them AFTER the step."""

    def __init__(self, E):
        self.dm, self.dv, self.dA = np.zeros(E), np.zeros(E), np.zeros(E)

    def after_step(self, A_new, g, m_prev, v_prev, st, lr, beta1, beta2, eps):
        t, p1, p2 = st["t"], st["p1"], st["p2"]
        c1, c2 = 1. - p1, 1. - p2
        m, v = st["m"], st["v"]
        self.dm = beta1 * self.dm + 8 * U * (np.abs(m_prev) + np.abs(g))
        self.dv = beta2 * self.dv + 8 * U * (v_prev + g * g)
        dc1 = ((t + 1) * p1 + 2 * c1) * U
        dc2 = ((t + 1) * p2 + 2 * c2) * U
        r = np.sqrt(v / c2)
        den = r + eps
        upd = lr * np.abs(m / c1) / den
        with np.errstate(divide="ignore", invalid="ignore"):
            dr = np.minimum(np.sqrt(self.dv / c2), np.where(v > 0, self.dv / (2 * np.sqrt(v * c2)), np.inf)) + r * dc2 / (2 * c2)
        self.dA = self.dA + 16 * U * upd + lr * self.dm / (c1 * den) + upd * dc1 / c1 + upd * dr / den + 2 * U * np.abs(flat(A_new))
        return 1.01 * self.dA


def cost(W, phi, labels, target_label=None):
    """the cost tnml_evaluate_* reports: sum over images and labels of (W_l(x_n) - y_nl)^2, on the weights of tests/sitegrad_model.py"""
    import sitegrad_model as sm
    _, w = sm.site_gradient(W, phi, labels=labels, target_label=target_label)
    return float(((w - sm.targets(labels, w.shape[1], target_label)) ** 2).sum())


# What the descent tests share: twenty Adam steps (default betas and eps) on the first ten images of small_case(12, 5), boosted
# features.  tests/test_sitestep_model_host.py shows that this lr brings the model's cost below half its start (on the CPU: to 0.39 of
# it; all 70 images were not halved in twenty steps at any lr between 0.003 and 0.1); tests/test_sitestep_gpu.py takes the same lr.
DESCENT = dict(case=(12, 5), images=10, steps=20, lr=2e-2)
