"""A numpy model of the arithmetic of the reduced-precision modes (dtype f32, bf16, bf16x3) -- TEST INFRASTRUCTURE ONLY.

The kernels of these modes (kernels_gemm32.hip, kernels_bf16e.hip, the float instantiations of k_labeldot and k_zprime_t) state their
arithmetic exactly, so the model restates it: every operand is rounded where the kernel of that path rounds it, by the same formula,
and every sum over rounded quantities is then taken in fp64.  What is left between a device result and the model is the device's fp32
accumulation, and `bound` is a worst-case figure for that.

Where the kernels round
  all modes      features are stored in fp32; the bond tensor / site tensor is rounded fp64 -> fp32 once (k_cvt, k_pack, k_m_bf16t)
  staged paths   X[n][2a + s] = fl32(E[n][a] * phi[n][s]) is formed in fp32 (k_fgemm and k_bgemm on either matrix pipe); in the bf16
                 modes X and every element of M are then rounded to bf16, round to nearest even by the bit formula of f2bf
  converted once k_fgemm_bf16e rounds the RAW environment to bf16 (k_env_bf16t) and the bond matrix to bf16 (k_m_bf16t); both site
                 features are applied to the fp32 accumulators: T = sum_t phiO_t sum_s phiI_s acc[s][t]
  bf16x3         x = hi + lo, hi = bf16(x), lo = bf16(fl32(x - hi)); the products summed are lo hi + hi lo + hi hi
  gradient       dP = fl32(target - P) from the fp32 P of the forward pass; Label on an environment: Z = the fp32 fma chain of
                 k_zprime_t over the ten labels, in order; Label on B: z = fl32(EX * dP); then Y = fl32(z * phiO) -- all reproduced
                 bit for bit (an fp32 fma is emulated as fl32 of the fp64 sum of the exact product: a double rounding once in ~2^29)
  slab sum       fp64 (k_slab_reduce)
  cost, pAp      the scalar epilogue of the fp32 label dot: d = fl32(target - P), val = fma(d, d, val) (pAp: fma(P, P, val)) over the labels
                 in fp32, then fp64 sums over the images -- exact functions of the P the device returns (cost_model, pap_model), held to
                 NT 2^-52 relative plus one fp32 ulp of one image; #correct exactly
  shift          k_fgemm without phiO in every one of these modes: fp32 operands on the fp32 matrix pipe

The bound: the same contraction with every rounded operand replaced by its absolute value, times
    (n_mfma + 4) u_mfma + n_valu u_32
n_mfma: products on the longest accumulation chain of the GEMM (the real reduction length, times three with hi + lo operands; for the
gradient the real images of one slab, or `chain`: the images of one slab whose product is not zero); n_valu: the fp32 operations behind it (epilogue: 2 staged, 4 converted once; label dot: mO fma
plus at most 15 adds across the waves).  u_32 = 2^-24: the VALU and v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain with one rounding per
product.  u_mfma = 2^-23 inside v_mfma_f32_16x16x32_bf16, whose internal summation is not documented: the extra bit covers an adder that
truncates.  A derived worst case, not a fitted tolerance.

Array conventions (those of oracle/pyoracle.py and tnml_amd/fixedl.py): B[a, s, t, r(, L)], A_j[a, s, r(, L)], environments [n, m(, L)],
features of one site [n, 2].  `kind`: 0 Label on the right environment, 1 on the left one, 2 on B (with label extent 1: the per-label
variant).  (EI, phiI) is the Label-free input side of the bond plan, (EX, phiO) the other one: see `plan`."""
import math

import numpy as np

NL = 10
U32 = 2.0 ** -24
UBF = 2.0 ** -23
MODES = ("f32", "bf16", "bf16x3")


# ---- rounding helpers ------------------------------------------------------------------------------
def to_f32(x):
    """float64 -> float32 (round to nearest even) -> float64"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def to_bf16(x):
    """float64 -> float32 (round to nearest even) -> bf16 by the kernels' bit formula (u + 0x7fff + ((u >> 16) & 1)) >> 16 -> float64"""
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))
    u = f.view(np.uint32)
    h = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) & np.uint32(0xFFFF)
    return (h << np.uint32(16)).astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def trunc_bf16(x):
    """the defect the gate must catch: bf16 by dropping the low 16 bits"""
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))
    return (f.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64).reshape(np.shape(x))


def split_bf16(x):
    """(hi, lo): hi = bf16(x), lo = bf16(fl32(x - hi))"""
    x = to_f32(x)
    hi = to_bf16(x)
    return hi, to_bf16(to_f32(x - hi))


def _ru(x, k):
    return (x + k - 1) // k * k


def bgemm_cut(mode, mI, mO, L, NTp, maxm):
    """the slab cut of the gradient GEMM, restated from launch_bgemm: tile class, slab count, images per slab, images of the
    last slab.  `mode` is the context's dtype (the bf16 modes pad the reduction dimension to 32), maxm the context's.
    The library does not report its cut, so this is a copy that has to be kept in step with launch_bgemm BY HAND (tile classes, the 1024-tile
    target, the slab workspace of 128 Kmax^2 floats): after a change of the cut there, the bound's `per` and the shapes that reach a short
    last slab / one chunk per slab have to be worked out again here and in test_rp_model_gpu.py."""
    bf = mode != "f32"
    Kp, Np = (_ru(2 * mI, 32) if bf else _ru(2 * mI, 16)), _ru(2 * mO, 16)
    Kmax = _ru(2 * maxm, 32) if bf else _ru(2 * maxm, 16)
    if Kp % 80 == 0 and Np % 80 == 0:
        tile = 80
    elif Kp > 32 and Np > 32:
        tile = 64
    else:
        tile = 32
    tiles = -(-Kp // tile) * -(-Np // tile) * L
    chunks = NTp // 32
    nsplit = max(1, min(-(-1024 // tiles), chunks))
    n, cap = L * Kp * Np, 128 * Kmax * Kmax
    while nsplit > 1 and nsplit * n > cap:
        nsplit -= 1
    per = -(-chunks // nsplit) * 32
    nsplit = -(-NTp // per)
    return dict(tile=tile, Kp=Kp, Np=Np, tiles=tiles, nsplit=nsplit, per=per, last=NTp - (nsplit - 1) * per)


def plan(kind, EL, phiL, ER, phiR):
    """(EI, phiI, phiO, EX) of the bond plan from the left / right environments and the features of the bond's two sites"""
    return (ER, phiR, phiL, EL) if kind == 1 else (EL, phiL, phiR, ER)


def kind_of(B, EL, ER):
    """the bond kind from where the Label index sits (neither environment and a 4-index B: the per-label variant, planned as kind 2)"""
    if np.ndim(ER) == 3:
        return 0
    return 1 if np.ndim(EL) == 3 else 2


class Model:
    """The model.  The small methods are the places a planted defect or the exact-operand variant replaces."""

    # -- what a variant overrides
    def f32(self, x):
        return to_f32(x)

    def bf(self, x):
        return to_bf16(x)

    def terms(self, nplanes):
        """(plane of the first operand, plane of the second) of every product summed: small terms first, as the kernels"""
        return [(0, 0)] if nplanes == 1 else [(1, 0), (0, 1), (0, 0)]

    def klen(self, K):
        """reduction indices summed of K real ones"""
        return K

    def nimg(self, NT):
        """images summed of NT real ones"""
        return NT

    def epilogue_phi(self, phiO):
        return phiO

    def images(self, NT):
        """the images the gradient sums, as indices into its arguments (a defect repeats or leaves out some)"""
        return np.arange(self.nimg(NT))

    def cost_images(self, NT):
        """the images the scalar epilogue of the label dot sums"""
        return np.arange(NT)

    def bucket(self, labels):
        """the per-label cost an image is summed into"""
        return labels

    def argmax(self, a):
        """k_labeldot: best = a[0]; a[l] > best moves it -- the first maximum"""
        return np.argmax(a, axis=1)

    # -- pieces
    def planes(self, mode, x):
        if mode == "f32":
            return [x]
        hi = self.bf(x)
        return [hi] if mode == "bf16" else [hi, self.bf(self.f32(x - hi))]

    def dot(self, mode, A, B):
        """A [r, K] x B [K, c] with both operands in the planes of `mode`: (sum of the products in fp64, the same of absolute values, products per element)"""
        Ap, Bp = self.planes(mode, A), self.planes(mode, B)
        val = np.zeros((A.shape[0], B.shape[1]))
        ab = np.zeros_like(val)
        for i, j in self.terms(len(Ap)):
            val += Ap[i] @ Bp[j]
            ab += np.abs(Ap[i]) @ np.abs(Bp[j])
        return val, ab, (1 if len(Ap) == 1 else 3)

    @staticmethod
    def m_layout(kind, B):
        """M[l, a, s, q, t] of bond_pack_desc: a / s on the input side, q / t on the output side"""
        B = np.asarray(B, dtype=np.float64)
        if kind == 1:
            return B.transpose(3, 2, 0, 1)[None]
        if B.ndim == 4:
            return B.transpose(0, 1, 3, 2)[None]
        return B.transpose(4, 0, 1, 3, 2)

    @staticmethod
    def from_m_layout(kind, G, ndim):
        if kind == 1:
            return G[0].transpose(2, 3, 1, 0)
        if ndim == 4:
            return G[0].transpose(0, 1, 3, 2)
        return G.transpose(1, 2, 4, 3, 0)

    def zprime(self, EX, dP):
        """k_zprime_t<float, float>: z = fma(EX[l], dP[l], z), l = 0 .. 9"""
        z = np.zeros(EX.shape[:2])
        for l in range(EX.shape[2]):
            z = self.f32(EX[:, :, l] * dP[:, None, l] + z)
        return z

    # -- the scalar epilogue of the fp32 label dot: exact functions of the P the device returns
    def _sq_chain(self, D):
        """val = fma(D[l], D[l], val), l in order, in fp32 (the emulation of zprime)"""
        val = np.zeros(D.shape[0])
        for l in range(D.shape[1]):
            val = self.f32(D[:, l] * D[:, l] + val)
        return val

    def cost_model(self, P, labels, target=None):
        """LD_MODE_COST of k_labeldot<.., float, float, float> from a device P ([NT, L], fp32 values): d = fl32(tgt - P_l),
        val = fl32(d d + val) over l in order, the per-label cost the fp64 sum (math.fsum) of val over the images of that label;
        #correct by the first maximum of |P_l| (strict >), in the per-label variant (P_0 > 0.5) == (label == target).
        Returns dict(label_cost [10], cost (without the regulariser), ncorrect, gate [10], cost_gate): |device - model| <= gate with
        gate = NT 2^-52 model + 2^-23 max_n val_n -- fp64 summation in another order, and one fp32 ulp of one image for the rare
        double rounding of the emulated fma."""
        labels = np.asarray(labels)
        P = self.f32(np.asarray(P, dtype=np.float64).reshape(labels.shape[0], -1))
        NT = P.shape[0]
        if target is None:
            tgt = (labels[:, None] == np.arange(NL)[None, :]).astype(np.float64)
            cor = self.argmax(np.abs(P)) == labels
        else:
            tgt = (labels == target).astype(np.float64)[:, None]
            cor = (P[:, 0] > 0.5) == (labels == target)
        val = self._sq_chain(self.f32(tgt - P))
        idx = self.cost_images(NT)
        val, cor, bucket = val[idx], cor[idx], np.asarray(self.bucket(labels))[idx]
        lc = np.array([math.fsum(val[bucket == l]) for l in range(NL)])
        cost = math.fsum(val)
        ulp = 2.0 ** -23 * (val.max() if val.size else 0.)
        return dict(label_cost=lc, cost=cost, ncorrect=int(cor.sum()), gate=NT * 2.0 ** -52 * lc + ulp, cost_gate=NT * 2.0 ** -52 * cost + ulp)

    def pap_model(self, P):
        """LD_MODE_PAP: val = fl32(P_l P_l + val) over l in order, then the fp64 sum over the images; (sum_n |p v_n|^2, its gate)"""
        P = np.asarray(P, dtype=np.float64)
        P = self.f32(P.reshape(P.shape[0], -1))
        val = self._sq_chain(P)[self.cost_images(P.shape[0])]
        s = math.fsum(val)
        return s, P.shape[0] * 2.0 ** -52 * s + 2.0 ** -23 * (val.max() if val.size else 0.)

    # -- the three launch sequences
    def forward_model(self, mode, path, kind, EI, phiI, B, phiO, EX):
        """P [NT, L] of TrainStates.forward (L = 10; 1 for a 4-index B with kind 2, the per-label variant) and its bound.
        path "staged": k_fgemm on the mode's matrix pipe; "once": k_fgemm_bf16e (bf16 modes, Label on an environment)."""
        EI, phiI, phiO, EX = self.f32(EI), self.f32(phiI), self.f32(phiO), self.f32(EX)
        M = self.f32(self.m_layout(kind, B))
        L, mI, mO = M.shape[0], M.shape[1], M.shape[3]
        NT = EI.shape[0]
        ph = self.epilogue_phi(phiO)
        if path == "staged":
            X = self.f32(EI[:, :, None] * phiI[:, None, :]).reshape(NT, 2 * mI)
            Mk = M.reshape(L, 2 * mI, 2 * mO).transpose(1, 0, 2).reshape(2 * mI, L * 2 * mO)
            K = self.klen(2 * mI)
            U, Ua, nt = self.dot(mode, X[:, :K], Mk[:K])
            U, Ua = U.reshape(NT, L, mO, 2), Ua.reshape(NT, L, mO, 2)
            T = (U * ph[:, None, None, :]).sum(axis=3)
            Ta = (Ua * np.abs(ph)[:, None, None, :]).sum(axis=3)
            n_mfma, n_epi = 2 * mI * nt, 2
        else:
            assert path == "once" and kind != 2 and mode != "f32"
            K = self.klen(mI)
            acc, acca, nt = self.dot(mode, EI[:, :K], M[0, :K].reshape(K, 4 * mO))
            acc, acca = acc.reshape(NT, 2, mO, 2), acca.reshape(NT, 2, mO, 2)
            u = (acc * phiI[:, :, None, None]).sum(axis=1)
            ua = (acca * np.abs(phiI)[:, :, None, None]).sum(axis=1)
            T = (u * ph[:, None, :]).sum(axis=2)[:, None, :]
            Ta = (ua * np.abs(ph)[:, None, :]).sum(axis=2)[:, None, :]
            n_mfma, n_epi = mI * nt, 4
        if kind == 2:                                             # k_labeldot: A = U (per label), Bv = EX
            P = (T * EX[:, None, :]).sum(axis=2)
            Pa = (Ta * np.abs(EX)[:, None, :]).sum(axis=2)
        else:                                                     # A = EX (Label-carrying), Bv = U
            P = (EX * T[:, 0, :, None]).sum(axis=1)
            Pa = (np.abs(EX) * Ta[:, 0, :, None]).sum(axis=1)
        u_mfma = U32 if mode == "f32" else UBF
        return P, ((n_mfma + 4) * u_mfma + (n_epi + mO + 15) * U32) * Pa

    def gradient_model(self, mode, kind, EI, phiI, phiO, EX, P, labels, per, Bndim, target=None, bf16_grad=True, chain=None, weights=None):
        """G in the shape of B (TrainStates.gradient) and its bound.  P: what the device's forward pass returned for the same B
        ([NT, L]); per: images per slab (bgemm_cut); target: the per-label variant's label; bf16_grad False: k_bgemm on the fp32 pipe
        in a bf16 mode; chain: the length of the longest fp32 accumulation chain where it is shorter than min(per, NT) -- the largest
        number of images of ONE slab whose product is not zero (adding an exact zero does not round, so the bound stays a worst case);
        weights ([NT, L]): the per-image weights of the sum as the device holds them, in place of fl32(target - P) -- the dP a CG pass left, or
        p*t.v for the image sum A p of the merged CG and of fast_conj (P is then not read)."""
        EI, phiI, phiO, EX = self.f32(EI), self.f32(phiI), self.f32(phiO), self.f32(EX)
        labels = np.asarray(labels)
        NT, mI = EI.shape
        if weights is not None:
            dP = self.f32(np.asarray(weights, dtype=np.float64).reshape(NT, -1))
        else:
            P = np.asarray(P, dtype=np.float64).reshape(NT, -1)
            if target is None:
                tgt = (labels[:, None] == np.arange(NL)[None, :]).astype(np.float64)
            else:
                tgt = (labels == target).astype(np.float64)[:, None]
            dP = self.f32(tgt - P)
        X = self.f32(EI[:, :, None] * phiI[:, None, :]).reshape(NT, 2 * mI)
        if kind == 2:
            z = self.f32(EX[:, None, :] * dP[:, :, None])                                   # [n, l, q]
            Y = self.f32(z[..., None] * phiO[:, None, None, :])
        else:
            Y = self.f32(self.zprime(EX, dP)[:, :, None] * phiO[:, None, :])[:, None]       # [n, 1, q, t]
        L, mO = Y.shape[1], Y.shape[2]
        idx = self.images(NT)
        X, Y = X[idx], Y[idx].reshape(len(idx), L * 2 * mO)
        live = np.any(X != 0, axis=1) & np.any(Y != 0, axis=1)
        if not live.all():                                  # an image whose X or Y is zero adds exact zeros: left out, so that the sum over
            X, Y = X[live], Y[live]                         # a set equals the sum over its live images bit for bit, whatever the BLAS does
        gm = mode if bf16_grad else "f32"
        G, Ga, nt = self.dot(gm, X.T, Y)
        G = G.reshape(mI, 2, L, mO, 2).transpose(2, 0, 1, 3, 4)
        Ga = Ga.reshape(mI, 2, L, mO, 2).transpose(2, 0, 1, 3, 4)
        u_mfma = U32 if gm == "f32" else UBF
        bound = ((min(per, NT) if chain is None else chain) * nt + 4) * u_mfma * Ga
        return self.from_m_layout(kind, G, Bndim), self.from_m_layout(kind, bound, Bndim)

    def shift_model(self, mode, Eprev, phi, A, from_left):
        """the environment TrainStates.shiftE writes at a site with tensor A from the previous environment (None: the chain end) and
        the site's features, and its bound; [NT, m_out] or [NT, m_out, 10]"""
        assert mode in MODES
        A = self.f32(np.asarray(A, dtype=np.float64))
        phi = self.f32(phi)
        NT = phi.shape[0]
        if A.ndim == 3:
            A = A[..., None]
        M = A if from_left else A.transpose(2, 1, 0, 3)                                      # [x, s, y, l]
        m_in, m_out, LA = M.shape[0], M.shape[2], M.shape[3]
        E = np.ones((NT, m_in)) if Eprev is None else self.f32(Eprev)
        K = self.klen(2 * m_in)
        Mk = M.reshape(2 * m_in, m_out * LA)
        if E.ndim == 3:                                                                     # Label on the environment: one GEMM per label
            X = self.f32(E[:, :, None, :] * phi[:, None, :, None]).reshape(NT, 2 * m_in, NL)
            out = np.empty((NT, m_out, NL))
            outa = np.empty_like(out)
            for l in range(NL):
                out[:, :, l], outa[:, :, l], _ = self.dot("f32", X[:, :K, l], Mk[:K])
        else:
            X = self.f32(E[:, :, None] * phi[:, None, :]).reshape(NT, 2 * m_in)
            out, outa, _ = self.dot("f32", X[:, :K], Mk[:K])
            out, outa = out.reshape(NT, m_out, LA), outa.reshape(NT, m_out, LA)
            if LA == 1:
                out, outa = out[:, :, 0], outa[:, :, 0]
        return out, (2 * m_in + 4) * U32 * outa


class ExactModel(Model):
    """the model with its rounding helpers replaced by the identity: must equal the fp64 oracle"""

    def f32(self, x):
        return np.asarray(x, dtype=np.float64)

    def bf(self, x):
        return np.asarray(x, dtype=np.float64)

    def planes(self, mode, x):
        return [x]


_M = Model()
forward_model = _M.forward_model
gradient_model = _M.gradient_model
shift_model = _M.shift_model
cost_model = _M.cost_model
pap_model = _M.pap_model


# ---- the shapes of the gate (test_rp_model_host.py plants its defects at them, test_rp_model_gpu.py runs them) ---------------------
FORWARD_DIMS = [1, 2, 16, 17, 33, 64, 65, 120, 40, 2, 1]            # NT = 40, every bond
# chains that carry the gradient tile classes at a Label-on-environment bond and at a Label-on-B bond: dims, {bond: (mI, mO)}
GRAD_CHAINS = [([1, 80, 120, 40, 120, 40, 120, 40, 2, 2, 1], {2: (80, 40), 3: (120, 120), 4: (40, 40), 5: (120, 120), 6: (40, 40)}),
               ([1, 2, 16, 33, 16, 17, 16, 33, 16, 2, 1], {3: (16, 16), 4: (33, 17), 5: (16, 16), 6: (33, 17), 7: (16, 16)}),
               ([1, 2, 9, 80, 9, 40, 5, 2, 9, 2, 1], {4: (80, 40), 5: (9, 5), 7: (9, 5)})]
GRAD_NT = 40
SLAB_DIMS, SLAB_NT, SLAB_BOND = [1, 2, 150, 150, 150, 150, 2, 2, 2, 2, 1], 700, 4          # bond 4: 150 x 150, Label on B
RAGGED_DIMS, RAGGED_NTS, RAGGED_BONDS = [1, 2, 61, 61, 61, 61, 2, 2, 2, 2, 1], (130, 257), (3, 4)
SINGLE_DIMS, SINGLE_NT = [1, 2, 17, 65, 40, 2, 1], 40
STALE = dict(N=24, NT=300, m=24, bond=6, far=21)                   # the copy-cache case: a 24 x 24 bond, Label on the right environment
NTPAD = 256
# at real image counts, per kernel: one short chain with maxm = 40.  Bond 2: 2 x 40 and 3: 16 x 16, Label on the right environment; 4: 40 x 40 and
# 5: 16 x 16, Label on B; 6: 17 x 40, 7: 2 x 16 and 8: 2 x 17, Label on the left environment.  Gradient tile classes: 80 (bond 4 in f32), 64 (bond 4
# in the bf16 modes, bond 6), 32 (bonds 3, 5); the label dot has more than one row per wave of its sixteen-wave form from mO = 17 on
SCALE_DIMS = [1, 2, 16, 40, 16, 40, 16, 17, 2, 2, 1]
SCALE_LDOT_NT = 300                                                 # both fp32 label-dot forms, forced
SCALE_THRESHOLD = {24320: 2, 24576: 1}                              # image count -> the form (ldot_cfg) the default dispatch takes: 190 / 192 blocks of 128
SCALE_THRESHOLD_BONDS = {4: (40, 40), 6: (17, 40)}
SCALE_NTS = (24576, 25000)                                          # the gradient with long slabs
SCALE_GRAD_BONDS = {4: (40, 40), 5: (16, 16), 6: (17, 40)}


def probe_set(cut, NT):
    """the images that keep their features in the sparse gradient cases: the first and the last real image of every slab of `cut`
    (bgemm_cut), the first image of one interior chunk of every slab, the last real image; and the largest number of them in one slab"""
    per = cut["per"]
    S = {NT - 1}
    for k in range(cut["nsplit"]):
        lo, hi = k * per, min((k + 1) * per, NT) - 1
        if lo < NT:
            S.update((lo, hi, lo + 32 * ((hi - lo + 1) // 64)))
    S = np.array(sorted(S))
    return S, int(np.bincount(S // per).max())


def bonds_of(dims, single=False):
    """(bond, kind, mI, mO, L) of every bond of a chain with link dimensions dims (Label index on site N / 2; none: the per-label variant)"""
    N = len(dims) - 1
    c0 = -1 if single else N // 2
    out = []
    for b in range(1, N):
        mL, mR = dims[b - 1], dims[b + 1]
        if single:
            out.append((b, 2, mL, mR, 1))
        elif c0 in (b, b + 1):
            out.append((b, 2, mL, mR, NL))
        elif c0 > b:
            out.append((b, 0, mL, mR, 1))
        else:
            out.append((b, 1, mR, mL, 1))
    return out
