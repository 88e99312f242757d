"""A bit-exact numpy model of the fp32 chain kernel (k_chain<float> in kernels_chain.hip, option predict_dtype = 1): operands rounded where the kernel
rounds them, every sum one fp32 fma chain in the kernel's order.

  1. A32 = fl32(A), phi32 = fl32(phi) with phi as the fp64 path forms it;
  2. the B operand of every product is fl32(phi32_s * v);
  3. an output element of a site is one fmaf chain from 0 over the contraction index kk of the site tensor's memory order (right chain
     kk = s + 2 r, left chain and centre kk = a + ml s), in blocks of 16: for i = 0..3, for q = 0..3, kk = base + 4 q + i; kk past the
     end of the last block contribute fma(0, 0, acc);
  4. centre, per label: one left-chain step, then w = fmaf(T[r], R[r], w) for r ascending; the output is (double)w.

fp32 values are carried in float64 arrays (every fp32 is an fp64).  The fp32 fma is emulated correctly rounded: the product of two fp32
is exact in fp64; the fp64 sum is corrected to round-to-odd with its TwoSum error, after which the rounding to fp32 is the rounding of
the exact value (fl32(fl64(a b + c)) alone double-rounds)."""
import numpy as np

F32 = np.float32


def fl32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(F32).astype(np.float64)


def fma32_plain(a, b, c):
    """the double-rounding form: wrong on ties of the fp64 sum (kept to show that the crafted family bites)"""
    return fl32(np.asarray(a, dtype=np.float64) * b + c)


def fma32(a, b, c):
    """correctly rounded fp32 fma of fp32 values held in float64 arrays"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b                                   # exact: 24 x 24 bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)             # TwoSum: p + c = s + err exactly
        even = (s.view(np.int64) & 1) == 0
        fix = (err != 0) & even & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)      # round to odd
    return fl32(s)


def features_u8(pixels):
    """the byte expression of the chain kernels in fp64: [1, ((byte / 255) / 255) / 4]"""
    x = np.asarray(pixels, dtype=np.float64)
    return np.stack([np.ones_like(x), ((x / 255.) / 255.) / 4.], axis=-1)


def _block_order(K, reverse):
    """the kernel's kk sequence over the blocks of 16, -1 for the masked kk of the last block"""
    order = []
    for base in range(0, K, 16):
        blk = [base + 4 * q + i for i in range(4) for q in range(4)]
        if reverse:
            blk = blk[::-1]
        order += [kk if kk < K else -1 for kk in blk]
    return order


def _step(A, phi_j, vin, left, exact, reverse):
    """one site.  A: [ml, 2, mr] or [ml, 2, mr, nl] (centre, left only); phi_j: [n, 2]; vin: [rows, n] -> [M, n] or [nl, M, n]"""
    ml, _, mr = A.shape[:3]
    lab = A.ndim == 4
    if left:                                        # kk = a + ml s; output index r
        K, Amat = 2 * ml, A.reshape((2 * ml,) + A.shape[2:], order="F")           # [kk, r(, l)]
        Amat = np.moveaxis(Amat, 0, -1)                                             # [r(, l), kk]
        if lab:
            Amat = np.moveaxis(Amat, 1, 0)                                          # [l, r, kk]
        srow = [(kk // ml, kk % ml) for kk in range(K)]
    else:                                           # kk = s + 2 r; output index a
        K, Amat = 2 * mr, A.reshape((ml, 2 * mr), order="F")                        # [a, kk]
        srow = [(kk & 1, kk >> 1) for kk in range(K)]
    acc = np.zeros(Amat.shape[:-1] + (vin.shape[1],))
    for kk in _block_order(K, reverse):
        if kk < 0:
            if not exact:
                acc = acc + 0.                      # fma(0, 0, acc): -0 becomes +0, everything else stays
            continue
        s, row = srow[kk]
        a = Amat[..., kk, None]
        if exact:
            acc = acc + a * (phi_j[:, s] * vin[row])
        else:
            acc = fma32(a, fl32(phi_j[:, s] * vin[row]), acc)
    return acc


def chain32(W, phi, exact=False, reverse=False):
    """weights [n, nl] (float64 holding the fp32 results) of the model for the site tensors W (list of [ml, 2, mr], one [ml, 2, mr, nl]
    at the centre; none: the per-label variant, site 1 plays the centre) and fp64 features phi [n, N, 2].
    exact: no rounding anywhere (fp64 operands, fp64 sums) -- the index order alone; reverse: the k order inside a block reversed"""
    N = len(W)
    cs = next((j for j in range(1, N + 1) if W[j - 1].ndim == 4), 1)
    rnd = (lambda x: np.asarray(x, dtype=np.float64)) if exact else fl32
    A = [rnd(w) for w in W]
    phi = rnd(phi)
    n = phi.shape[0]
    R = np.ones((1, n))
    for j in range(N, cs, -1):
        R = _step(A[j - 1], phi[:, j - 1], R, False, exact, reverse)
    L = np.ones((1, n))
    for j in range(1, cs):
        L = _step(A[j - 1], phi[:, j - 1], L, True, exact, reverse)
    Ac = A[cs - 1] if A[cs - 1].ndim == 4 else A[cs - 1][..., None]
    T = _step(Ac, phi[:, cs - 1], L, True, exact, reverse)          # [nl, mr, n]
    w = np.zeros((T.shape[0], n))
    for r in range(T.shape[1]):
        w = w + T[:, r] * R[r] if exact else fma32(T[:, r], R[r], w)
    return np.ascontiguousarray(w.T)


def predict32(W, phi, single=False):
    """(weights, pred) as tnml_predict_* returns them under predict_dtype = 1"""
    w = chain32(W, phi)
    pred = (w[:, 0] > 0.5).astype(np.int32) if single else np.abs(w).argmax(axis=1).astype(np.int32)
    return w, pred
