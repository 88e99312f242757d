"""Ground truth for LARGE image counts from a SMALL base set (helper of test_dispatch_at_scale.py; not a test module).

The large data set repeats K base images: features phi0[idx], labels l0[idx] for an index vector idx of length NT, with c_k = bincount(idx).
Everything the training step computes is then known from the base set alone:
  P_big[n] = P_base[idx[n]] and likewise every environment row;
  G_big = sum_k c_k dP_k (x) v_k; the cost, the per-label costs and #correct are the c_k-weighted base values;
  if every c_k = R, the CG and the bond update are those of the base set at lambda/R and cconv/R: the same B after every pass (so the same
  split, new bond dimension and truncation error), cost_big = R cost_base, |r|_big = R |r|_base, alpha_big = alpha_base / R,
  pAp_big = R^3 pAp_base, #correct_big = R #correct_base.
idx is a seeded PERMUTATION of arange(NT) % K, so the copies of a base image do not line up with the 32/64/128/256-image tiles of the kernels.

BondReference evaluates one bond from per-base-image factors of t.v (left environment, the two site features, right environment) in
np.longdouble where that is an extended type (fp64 otherwise).  t.v itself is never formed: at m = 120 it has 576 000 entries per image."""
import numpy as np

NL = 10
XP = np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else np.float64      # the referee's number type


def mps_with_dims(dims, seed):
    """random weight MPS with the given bond dimensions d_0 = 1, d_1, ..., d_N = 1 (Label index on site N/2)"""
    rng = np.random.default_rng(seed)
    N = len(dims) - 1
    W = []
    for j in range(1, N + 1):
        ml, mr = dims[j - 1], dims[j]
        shape = (ml, 2, mr, NL) if j == N // 2 else (ml, 2, mr)
        A = rng.standard_normal(shape) / np.sqrt(2. * max(ml, mr) * (NL if j == N // 2 else 1))
        A[:, 0] += (np.eye(ml, mr) if A.ndim == 3 else np.eye(ml, mr)[:, :, None] / np.sqrt(float(NL)))
        W.append(A)
    return W


def plain_mps_with_dims(dims, seed):
    """the same recipe without the Label index: the plain weight MPS of the per-label variant (single.cc)"""
    rng = np.random.default_rng(seed)
    W = []
    for j in range(1, len(dims)):
        ml, mr = dims[j - 1], dims[j]
        A = rng.standard_normal((ml, 2, mr)) / np.sqrt(2. * max(ml, mr))
        A[:, 0] += np.eye(ml, mr)
        W.append(A)
    return W


def without_label(W):
    """a Label-carrying weight MPS as a plain one: the first label's slice of site N/2 (scaled back up, as the per-label tests do)"""
    W = list(W)
    c0 = len(W) // 2
    W[c0 - 1] = W[c0 - 1][..., 0] * 3.0
    return W


class TiledProblem:
    """base problem (phi0, labels0, W), the index vector and its counts; the materialised large set on demand"""

    def __init__(self, phi0, labels0, W, idx):
        self.phi0, self.labels0, self.W, self.idx = phi0, np.asarray(labels0, dtype=np.int32), W, idx
        self.K, self.NT = phi0.shape[0], int(idx.shape[0])
        self.counts = np.bincount(idx, minlength=self.K).astype(np.int64)
        self.R = int(self.counts[0]) if (self.counts == self.counts[0]).all() else None      # the uniform repeat count, if there is one

    @property
    def phi(self):
        return np.ascontiguousarray(self.phi0[self.idx])

    @property
    def labels(self):
        return np.ascontiguousarray(self.labels0[self.idx])


def tiled_problem(N, K, NT, m, seed, pixel_boost=200.0, dims=None):
    """K base images of conftest.make_problem (W = random_mps(N, m), or hand-chosen bond dimensions `dims`), repeated to NT images"""
    from conftest import make_problem
    pixels, labels, phi, W = make_problem(N, K, m, seed, pixel_boost=pixel_boost)
    if dims is not None:
        assert len(dims) == N + 1
        W = mps_with_dims(dims, seed + 7)
    idx = np.random.default_rng(seed + 1000).permutation(np.arange(NT) % K)
    return TiledProblem(phi, labels, W, idx)


def extended_environments(tp, upto_bond):
    """the numpy restatement of the reference on the base set in XP: right environments of init, left ones up to bond `upto_bond`"""
    from oracle import np_restatement as npr
    n = npr.NpFixedL(tp.phi0, tp.labels0, tp.W)
    n.phi = n.phi.astype(XP); n.W = [None] + [x.astype(XP) for x in n.W[1:]]; n.delta = n.delta.astype(XP)
    n.init()
    for b in range(1, upto_bond):
        n.shiftE(b, True)
    return n


class BondReference:
    """B*t.v, dP*dag(t.v) and the count-weighted sums of one bond from per-base-image factors: LE [K][a(,l)], fs, ft [K][2], RE [K][r(,l)]
    (chain ends: a [K][1] array of ones); tensors in ITensor index order B[a,s,t,r(,l)]"""

    def __init__(self, LE, fs, ft, RE, labels0):
        self.LE, self.fs, self.ft, self.RE = (np.asarray(x, dtype=XP) for x in (LE, fs, ft, RE))
        self.labels0 = np.asarray(labels0)
        self.K = self.fs.shape[0]
        self.delta = np.eye(NL, dtype=XP)[self.labels0]
        self.kind = "LE" if self.LE.ndim == 3 else "RE" if self.RE.ndim == 3 else "B"
        st = self.fs[:, :, None] * self.ft[:, None, :]
        if self.kind == "LE":                                               # F[k][(s,t,r)]
            self.F = (st[:, :, :, None] * self.RE[:, None, None, :]).reshape(self.K, -1)
        else:                                                               # F[k][(a,s,t)]
            self.F = (self.LE[:, :, None, None] * st[:, None, :, :]).reshape(self.K, -1)

    @classmethod
    def at_bond(cls, n, b, labels0):
        """from an NpFixedL-like object whose E holds the left environment of bond b (site b-1) and the right one (site b+2)"""
        K = n.phi.shape[0]
        LE = n.E[b - 1] if b - 1 > 0 else np.ones((K, 1))
        RE = n.E[b + 2] if b + 2 < n.N + 1 else np.ones((K, 1))
        return cls(LE, n.phi[:, b - 1], n.phi[:, b], RE, labels0)

    def forward(self, B):
        B = np.asarray(B, dtype=XP)
        mL, mR = B.shape[0], B.shape[3]
        if self.kind == "RE":
            return np.einsum('kr,krl->kl', self.F @ B.reshape(mL * 4, mR), self.RE)
        if self.kind == "LE":
            return np.einsum('ka,kal->kl', self.F @ B.reshape(mL, 4 * mR).T, self.LE)
        return np.einsum('krl,kr->kl', (self.F @ B.reshape(mL * 4, mR * NL)).reshape(self.K, mR, NL), self.RE)

    def backward(self, w):
        """sum_k w_k (x) v_k for per-image weights w [K][10] (the residuals dP_k, times the counts)"""
        w = np.asarray(w, dtype=XP)
        if self.kind == "RE":
            mL, mR = self.LE.shape[1], self.RE.shape[1]
            return (self.F.T @ np.einsum('kl,krl->kr', w, self.RE)).reshape(mL, 2, 2, mR)
        if self.kind == "LE":
            mL, mR = self.LE.shape[1], self.RE.shape[1]
            return (np.einsum('kl,kal->ka', w, self.LE).T @ self.F).reshape(mL, 2, 2, mR)
        mL, mR = self.LE.shape[1], self.RE.shape[1]
        return (self.F.T @ (self.RE[:, :, None] * w[:, None, :]).reshape(self.K, -1)).reshape(mL, 2, 2, mR, NL)

    def evaluate(self, B):
        """per-base-image outputs of one bond tensor: P, dP, the unit-count gradient sum_k dP_k (x) v_k, squared residuals, hits"""
        P = self.forward(B)
        dP = self.delta - P
        return dict(P=P, dP=dP, G1=self.backward(dP), sq=np.sum(dP * dP, axis=1),
                    hit=(np.argmax(np.abs(P), axis=1) == self.labels0))                 # first maximum, util.h:42-57

    def weighted(self, ev, counts, B, lam):
        """the large set's gradient, cost, per-label costs, regulariser and #correct from evaluate(B) and the counts c_k"""
        c = np.asarray(counts)
        if (c == c[0]).all():
            G = ev["G1"] * XP(int(c[0]))
        else:
            G = self.backward(ev["dP"] * c.astype(XP)[:, None])
        wsq = ev["sq"] * c.astype(XP)
        lc = np.array([wsq[self.labels0 == l].sum() for l in range(NL)], dtype=XP)
        CR = XP(lam) * np.sum(np.asarray(B, dtype=XP) ** 2)
        return dict(G=G, cost=float(lc.sum() + CR), label_cost=lc.astype(np.float64), reg_cost=float(CR), ncorrect=int(c[ev["hit"]].sum()))

    def pAp(self, p, lam, counts):
        """sum_n |p*t.v_n|^2 + lambda |p|^2 over the large set (fixedL.cc:394-403)"""
        Pp = self.forward(p)
        return float(np.sum(np.sum(Pp * Pp, axis=1) * np.asarray(counts).astype(XP)) + XP(lam) * np.sum(np.asarray(p, dtype=XP) ** 2))


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def scaled_trace(tr, R):
    """the large set's CG trace from the base set's at lambda/R, cconv/R"""
    return dict(cost=[R * x for x in tr["cost"]], rnorm=[R * x for x in tr["rnorm"]], alpha=[x / R for x in tr["alpha"]],
                pAp=[float(R) ** 3 * x for x in tr["pAp"]])


# ---------------------------------------------------------------------------------------------------------------------------------------
# The per-label variant (single.cc / single.h: plain weight MPS, one output f_n per image, target y_n = [l_n == target]).  With a uniform
# repeat count R the large set follows from the base set alone:
#   f_big[n] = f_base[idx[n]];  G_big = R G_base;  cost_big(lambda) = R cost_base(lambda / R);  #correct_big = R #correct_base;
#   the CG (conj) on the large set is the base set's at lambda / R, cconv / R: the same B after every pass, traces scaled as scaled_trace does;
#   the density-matrix split with a noise term is the base set's at noise * R: rho = B B^dag does not depend on the images while
#   drho = sum_n dr_n dr_n^dag does, so rho + noise drho_big = rho + (noise R) drho_base -- also at the chain ends, where drho = NT rho.
def single_hits(f, labels, target):
    """#correct of the per-label variant (single.h:103,193): the decision f > 1/2 against [label == target]"""
    return int(((np.asarray(f) > 0.5) == (np.asarray(labels) == target)).sum())


def single_tiled(tp, target, f_base, G_base, cost_base_at_lam_over_R):
    """outputs, gradient, cost and #correct of the large set from the base set's (uniform repeat count)"""
    assert tp.R is not None
    return dict(P=np.asarray(f_base)[tp.idx], G=tp.R * np.asarray(G_base), cost=tp.R * cost_base_at_lam_over_R,
                ncorrect=tp.R * single_hits(f_base, tp.labels0, target))
