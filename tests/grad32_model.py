"""A numpy restatement of the fp32 streamed gradients (option gradient_dtype = 1: k_site_backward<float>, k_site_grad<float> in
kernels_sitegrad.hip, k_input_grad<float> in kernels_inputgrad.hip): operands rounded where the kernels round them, every sum in the
kernels' order.  Built on chain32_model.py: every chain step of the backward pass is the one modelled there (_step), fp32 values are
carried in float64 arrays, fma32 is the correctly rounded fp32 fma.  tests/test_grad32_model_host.py proves this file,
tests/test_grad32_gpu.py holds the kernels to it.

  1. Operands: A32 = fl32(A); phi32 = fl32(phi) with phi as the fp64 path forms it; given coefficients c = fl32(coef).
  2. Phase A is chain32_model's walk and centre, call for call: every L_b and R_b is kept (the inward tape).
  3. Labels mode: c = fl32(2 ((double)w - y)) (softmax: fl32 of loss_model.coefficients on the widened weights).
  4. Seeds: X_{c-1} (right-chain index order kk = s + 2 r over R) and Y_c (left-chain order kk = a + ml s over L), each ONE fmaf chain per
     element over the labels l ascending and, inside a label, chain32_model's block order; the operand is fl32(fl32(c_l phi_s) v).
  5. Outward walk: chain32_model._step itself (X to the left with the right-chain order, Y to the right with the left-chain order).
  6. k_site_grad<float>: per output element and chunk one fmaf chain from 0 over the chunk's images ascending (tiles in order, four
     images per MFMA step, q ascending: the image index itself), acc = fmaf(fl32(f_s Z[r]), E[a], acc) with f_s = phi32_s (Label site:
     fl32(c_l phi32_s)); then G = G + (double)acc in fp64, chunk after chunk.
  7. k_input_grad<float>, per image: (1) P_s[a] one fmaf chain over r in blocks of 16 (k = base + 4 q + i, i outer), at the Label site
     label after label into the same chain with the operand fl32(c_l Z[r]); (2) per wave w and lane group q: v = fmaf(E[row], P_s[row], v)
     over the rows 16 rt + 4 q + reg, reg = 0..3, rt = w, w + 8, ..; (3) ((v_0 + v_1) + v_2) + v_3; (4) the wave sums added in order from 0.

Defects (test_grad32_model_host.py plants them, each must change bits): "reverse_images" (6 with the images descending), "f64_rowmap"
(the fp64 C/D map q + 4 reg where the fp32 MFMA delivers row 4 q + reg: the rows r of every 16-row block of G land permuted),
"coef_unrounded" (c kept in fp64), "chunk_sum_f32" (G = fl32(G + acc)).

The bound against the fp64 models (sitegrad_model.py, inputgrad_model.py)
--------------------------------------------------------------------------
Those files count the roundings K_dev on the longest path to an element for exactly this order of operations; here every one of them
is an fp32 rounding, u = 2^-24.  On top come the operand roundings: every factor of a path -- at most N site tensors, N features, one
coefficient -- has been rounded to fp32 once, 2 N + 1 roundings, and the fp64 model's own K_dev 2^-53 (less than one fp32 rounding:
+ 1).  So |G32 - G64| <= (K_dev + 2 N + 2) 2^-24 x the contraction on absolute values, likewise for dphi with inputgrad_model's K_dev.
In the labels mode c carries the error of the fp32 weight, |dc| <= 2 (K_w + 2 N + 2) 2^-24 (Wabs + |y|) with sitegrad_model's K_w; the
same contraction on |dc| is added."""
import functools

import numpy as np

import chain32_model as cm
import inputgrad_model as im
import sitegrad_model as sm
from chain32_model import fl32, fma32

U32 = 2.0 ** -24
DEFECTS = ("reverse_images", "f64_rowmap", "coef_unrounded", "chunk_sum_f32")
DIMS1024 = [1, 2, 16, 8, 1024, 1023, 513, 8, 2, 1]      # bonds to 1 024; the Label site (N = 9, site 4) carries 8 x 2 x 1024 x 10


def add32(a, b):
    """correctly rounded fp32 sum of fp32 values held in float64 (fl32 of the fp64 sum alone double-rounds)"""
    return fma32(a, 1.0, b)


def fma32_fast(a, b, c):
    """chain32_model.fma32 with fewer passes over large arrays, for the image chain of the GEMM.  s = fl64(a b + c) rounds to the
    fp32 that the exact a b + c rounds to unless s lies exactly half way between two fp32 numbers (the halfway points are fp64 numbers,
    so the exact value, within half an fp64 ulp of s, cannot lie across one from s); those elements, and every array with a result near
    the fp32 subnormals, where half way lies elsewhere, go through fma32 itself"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        s = a * b + c
        mag = np.abs(s)
        if not np.isfinite(s).all() or ((mag < 2.0 ** -120) & (mag > 0)).any():
            return fma32(a, b, c)
        out = fl32(s)
        tie = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
        if tie.any():
            out[tie] = fma32(a[tie], b[tie], c[tie])
    return out


def _seed(Ac, phi_c, c, vin, left):
    """the seed of an outward walk.  Ac [ml, 2, mr, nl], phi_c [n, 2], c [n, nl], vin [rows, n] -> [M, n]"""
    ml, _, mr, nl = Ac.shape
    K = 2 * ml if left else 2 * mr
    acc = np.zeros((mr if left else ml, vin.shape[1]))
    for l in range(nl):
        if left:                                        # kk = a + ml s; output index r
            Amat = Ac[..., l].reshape((2 * ml, mr), order="F").T
            srow = [(kk // ml, kk % ml) for kk in range(K)]
        else:                                           # kk = s + 2 r; output index a
            Amat = Ac[..., l].reshape((ml, 2 * mr), order="F")
            srow = [(kk & 1, kk >> 1) for kk in range(K)]
        cphi = [fl32(c[:, l] * phi_c[:, 0]), fl32(c[:, l] * phi_c[:, 1])]
        for kk in cm._block_order(K, False):
            if kk < 0:
                acc = acc + 0.
                continue
            s, row = srow[kk]
            acc = fma32_fast(Amat[:, kk, None], fl32(cphi[s] * vin[row]), acc)
    return acc


def _gemm(Ea, Z, f, chunk, defect):
    """k_site_grad<float> for one (virtual) site: Ea [ml, n], Z [mr, n], f [n, 2] the feature operand -> G [ml, 2, mr] (fp64)"""
    ml, n = Ea.shape
    mr = Z.shape[0]
    G = np.zeros((ml, 2, mr))
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        acc = np.zeros((ml, 2, mr))
        imgs = range(hi - 1, lo - 1, -1) if defect == "reverse_images" else range(lo, hi)
        for i in imgs:
            y = fl32(f[i][:, None] * Z[:, i][None, :])                              # [2, mr]
            acc = fma32_fast(y[None, :, :], Ea[:, i][:, None, None], acc)
        G = fl32(G + acc) if defect == "chunk_sum_f32" else G + acc
    if defect == "f64_rowmap":                                                       # lane group q, register reg: row 4 q + reg stored at q + 4 reg
        out = np.zeros_like(G)
        for r0 in range(0, mr, 16):
            for q in range(4):
                for reg in range(4):
                    src, dst = r0 + 4 * q + reg, r0 + q + 4 * reg
                    if dst < mr and src < mr:
                        out[:, :, dst] = G[:, :, src]
        G = out
    return G


def _input_site(A, Ea, Z, c):
    """k_input_grad<float> for one site: A [ml, 2, mr] (Label site: [ml, 2, mr, nl] with c [n, nl]), Ea [ml, n], Z [mr, n] -> [n, 2]"""
    ml, _, mr = A.shape[:3]
    n = Ea.shape[1]
    labs = range(A.shape[3]) if A.ndim == 4 else [None]
    P = np.zeros((2, ml, n))
    for l in labs:
        Al = A if l is None else A[..., l]
        for k in cm._block_order(mr, False):
            if k < 0:
                P = P + 0.
                continue
            b = Z[k] if l is None else fl32(c[:, l] * Z[k])
            P = fma32_fast(np.moveaxis(Al[:, :, k], 1, 0)[:, :, None], b[None, None, :], P)
    nrt = (ml + 15) // 16
    nk = (nrt + 7) // 8
    rows = 16 * 8 * nk
    Ep = np.zeros((rows, n))
    Ep[:ml] = Ea
    Pp = np.zeros((2, rows, n))
    Pp[:, :ml] = P
    live = (np.arange(rows) < ml).reshape(nk, 8, 4, 4)                               # [k][wave][q][reg]: row 16 (wave + 8 k) + 4 q + reg
    Ep = Ep.reshape(nk, 8, 4, 4, n)
    Pp = Pp.reshape(2, nk, 8, 4, 4, n)
    v = np.zeros((2, 8, 4, n))
    for k in range(nk):
        for reg in range(4):
            v = np.where(live[k, :, :, reg][None, :, :, None], fma32(Ep[k, :, :, reg][None], Pp[:, k, :, :, reg], v), v)
    t = add32(add32(add32(v[:, :, 0], v[:, :, 1]), v[:, :, 2]), v[:, :, 3])          # [2, wave, n]
    total = np.zeros((2, n))
    for w in range(8):
        total = add32(total, t[:, w])
    return total.T


def backward32(W, phi, coef=None, labels=None, target_label=None, chunk=512, loss="quadratic", beta=1.0, want_grads=True, want_dphi=True, defect=None):
    """-> dict(weights [n, nl], pred [n], coef [n, nl] (the fp32 values the kernels used), grads (list shaped like W) | None,
    dphi [n, N, 2] | None), everything float64 holding what the device returns.  Exactly one of coef and labels; chunk: option
    gradient_chunk; loss "softmax": the labels mode forms c by loss_model.py with the inverse temperature beta."""
    assert (coef is None) != (labels is None)
    assert defect is None or defect in DEFECTS
    N = len(W)
    lab_sites = [j for j in range(1, N + 1) if W[j - 1].ndim == 4]
    single = not lab_sites
    cs = lab_sites[0] if lab_sites else 1
    A = [fl32(w) for w in W]
    phi = fl32(phi)
    n = phi.shape[0]
    Ac = A[cs - 1] if not single else A[cs - 1][..., None]
    nl = Ac.shape[3]
    inward, outward = {N: np.ones((1, n)), 0: np.ones((1, n))}, {}
    for j in range(N, cs, -1):                                                       # R_j on bond j - 1
        inward[j - 1] = cm._step(A[j - 1], phi[:, j - 1], inward[j], False, False, False)
    for j in range(1, cs):                                                           # L_j on bond j
        inward[j] = cm._step(A[j - 1], phi[:, j - 1], inward[j - 1], True, False, False)
    Lc, Rc = inward[cs - 1], inward[cs]
    T = cm._step(Ac, phi[:, cs - 1], Lc, True, False, False)                         # [nl, mr, n]
    w = np.zeros((nl, n))
    for r in range(T.shape[1]):
        w = fma32(T[:, r], Rc[r], w)
    w = np.ascontiguousarray(w.T)
    pred = (w[:, 0] > 0.5).astype(np.int32) if single else np.abs(w).argmax(axis=1).astype(np.int32)
    if coef is not None:
        c = np.asarray(coef, dtype=np.float64)
    elif loss == "softmax":
        import loss_model
        c = loss_model.coefficients(w, labels, beta)
    else:
        c = 2. * (w - sm.targets(labels, nl, target_label))
    if defect != "coef_unrounded":
        c = fl32(c)
    if cs > 1:
        outward[cs - 1] = _seed(Ac, phi[:, cs - 1], c, Rc, False)
        for j in range(cs - 1, 1, -1):                                               # X_{j-1} on bond j - 1
            outward[j - 1] = cm._step(A[j - 1], phi[:, j - 1], outward[j], False, False, False)
    if cs < N:
        outward[cs] = _seed(Ac, phi[:, cs - 1], c, Lc, True)
        for j in range(cs + 1, N):                                                   # Y_j on bond j
            outward[j] = cm._step(A[j - 1], phi[:, j - 1], outward[j - 1], True, False, False)
    grads = [] if want_grads else None
    dphi = np.zeros((n, N, 2)) if want_dphi else None
    for j in range(1, N + 1):
        Ea = (inward if j <= cs else outward)[j - 1]
        Z = (outward if j < cs else inward)[j]
        if want_grads:
            if j == cs:
                G = np.stack([_gemm(Ea, Z, fl32(c[:, l, None] * phi[:, j - 1]), chunk, defect) for l in range(nl)], axis=-1)
                grads.append(G[..., 0] if single else G)
            else:
                grads.append(_gemm(Ea, Z, phi[:, j - 1], chunk, defect))
        if want_dphi:
            dphi[:, j - 1] = _input_site(Ac if j == cs else A[j - 1], Ea, Z, c if j == cs else None)
    return dict(weights=w, pred=pred, coef=np.asarray(c, dtype=np.float64), grads=grads, dphi=dphi)


# ---- the bounds against the fp64 models ----
def _counts(W, n):
    N = len(W)
    m = max(max(A.shape[0], A.shape[2]) for A in W)
    nl = max([A.shape[3] for A in W if A.ndim == 4] + [1])
    k_g = sm.rounding_counts(N, m, n, nl)[0] // 2                                    # K_dev of the site gradient
    k_w = (sm.rounding_counts(N, m, n, nl)[1] - 1) // 2                              # K_w of a weight
    k_d = (N - 1) * (4 * m + 1) + (nl - 1) * 4 * m + 1 + 3 * nl * m + 2 * m + 11     # K_dev of inputgrad_model.py's header
    return N, nl, k_g, k_w, k_d


def weight_bound(W, phi):
    """elementwise bound [n, nl] on |w32 - w64|"""
    N, nl, _, k_w, _ = _counts(W, len(phi))
    _, w_abs, _ = sm.abs_gradient(W, phi, coef=np.zeros((len(phi), nl)))
    return (k_w + 2 * N + 2) * U32 * w_abs


def _dc(W, phi, labels, target_label):
    N, nl, _, k_w, _ = _counts(W, len(phi))
    _, w_abs, _ = sm.abs_gradient(W, phi, coef=np.zeros((len(phi), nl)))
    return 2. * (k_w + 2 * N + 2) * U32 * (w_abs + sm.targets(labels, nl, target_label))


def bound_grads(W, phi, coef=None, labels=None, target_label=None):
    """elementwise bound on |G32 - G64|, a list shaped like the gradients (quadratic loss)"""
    W = [np.asarray(A, dtype=np.float64) for A in W]
    phi = np.asarray(phi, dtype=np.float64)
    N, nl, k_g, _, _ = _counts(W, len(phi))
    g_abs, _, _ = sm.abs_gradient(W, phi, coef, labels, target_label)
    out = [(k_g + 2 * N + 2) * U32 * g for g in g_abs]
    if labels is not None:
        dc = _dc(W, phi, labels, target_label)
        g_dc, _, _ = sm._contract([np.abs(A) for A in W], np.abs(phi), lambda w: dc)
        out = [a + b for a, b in zip(out, g_dc)]
    return out


def bound_dphi(W, phi, coef=None, labels=None, target_label=None):
    """elementwise bound [n, N, 2] on |dphi32 - dphi64| (quadratic loss)"""
    W = [np.asarray(A, dtype=np.float64) for A in W]
    phi = np.asarray(phi, dtype=np.float64)
    N, nl, _, _, k_d = _counts(W, len(phi))
    d_abs, _, _ = im.abs_input_gradient(W, phi, coef, labels, target_label)
    out = (k_d + 2 * N + 2) * U32 * d_abs
    if labels is not None:
        dc = _dc(W, phi, labels, target_label)
        out = out + im._contract([np.abs(A) for A in W], np.abs(phi), lambda w: dc)[0]
    return out


# ---- the inputs the two test files share, each model computed once per process ----
def case(kind, key):
    """dict(pixels, labels, coef, forms {"phi", "u8"}, W).  kind "small", key (N, m): chain32_cases' 70 images; kind "dims", key k:
    40 images on chain32_cases.DIMS[k]; kind "1024": 8 images on DIMS1024"""
    return _case(kind, key)


@functools.lru_cache(maxsize=None)
def _case(kind, key):
    import chain32_cases as cases
    from conftest import make_problem
    if kind == "1024":
        N = len(DIMS1024) - 1
        pixels, labels, phi, _ = make_problem(N, 40, 2, 5, pixel_boost=200.0)
        pixels, labels, phi = pixels[:8], labels[:8], phi[:8]
        forms, W = {"phi": phi, "u8": cm.features_u8(pixels)}, cases.mps_with_dims(DIMS1024, 11)
    else:
        pixels, forms, W = cases.inputs(kind, key)
        N = len(W)
        labels = make_problem(N, 70, key[1], 3, pixel_boost=200.0)[1] if kind == "small" else make_problem(N, 40, 2, 5, pixel_boost=200.0)[1]
    n = len(pixels)
    labels = np.asarray(labels[:n], dtype=np.int32)
    coef = np.random.default_rng(n + len(W)).standard_normal((n, 10))
    return dict(pixels=pixels, labels=labels, coef=coef, forms=forms, W=W)


@functools.lru_cache(maxsize=None)
def model(kind, key, form, mode, chunk=512):
    """backward32 on a case: form "phi" | "u8", mode "labels" | "coef" """
    d = case(kind, key)
    kw = dict(labels=d["labels"]) if mode == "labels" else dict(coef=d["coef"])
    return backward32(d["W"], d["forms"][form], chunk=chunk, **kw)
