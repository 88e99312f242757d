"""The conjugate-gradient solve at a bond, checked pass by pass -- TEST INFRASTRUCTURE ONLY.

cgrad_device (tnml_bond.hip) is a short chain of single launches per pass, and every one of those launches has a derived elementwise bound
in rp_model.py.  Rounding that the CG amplifies over its passes is kept out of the comparison by taking the DEVICE's own state before a
pass as the input of the model of that pass: `before` and `after` are what two prefix runs cgrad(B0, k) and cgrad(B0, k + 1) from the same
B0 left on the device (TrainStates.cg_state), and check_pass returns, by name, |device - model| / bound of every relation between them.

What a run of k passes leaves (the loop breaks after the step of the last pass, fixedL.cc:409):
    B    B_k = B_{k-1} + alpha_k p_k                                  Pv   p_k
    Pp   p_k * t.v, the outputs of the pAp pass of pass k (fast_cg = 0: not written)   R    r_{k-1}
    P, dP   fast_cg = 1: the outputs of B_{k-1} and tgt - P;  fast_cg = 0: P is not written by the CG, dP = tgt - B_{k-1} * t.v
    G    literal and folded form: the gradient sum G_{k-1} (weights dP);  merged form: A p_{k-1} = sum_n (p_{k-1}.v_n) v_n (weights Pp of
         pass k - 1);  fast_conj (per-label variant): r_{k-2} - alpha_{k-1} A p_{k-1}, what k_cg_fast_resid0 wrote over A p_{k-1}
    trace   pAp and alpha of passes 1 .. k, cost and |r| of passes 1 .. k - 1; zeros behind

Paths (`path`): "folded" (fast_cg = 1 on one rank, the default), "literal" (fast_cg = 0), "merged" (merged_cg = 2), "fast_conj" (per-label
variant, cg_method = 1).  Modes: rp.MODES and "f64".

The fp64 mode goes through the same relations with exact operands.  Its bound for a sum is (terms + 4) 2^-52 sum |terms|: any summation
order of n terms is within (n - 1) 2^-53 sum |terms| to first order, a term is a product of at most five factors (four roundings, or fewer
where an fma contracts one), and the factor two between 2^-53 and 2^-52 covers the second-order terms -- so the slab cuts and the MFMA
orders of k_fgemm64, k_bgemm64, k_grad_quad and the resident kernels need no model of their own.  sum |terms| is the same contraction on
the absolute values of every operand.

Vector relations (k_cg_init1, k_cg_step2, k_cg_resid1 / k_cg_resid2), u = 2^-52:
    r = G - lambda B                      2 u (|G| + |lambda B|): one product, one difference (or their fma)
    r = r' - alpha (Ap + lambda p)        3 u (|r'| + |alpha| (|Ap| + |lambda p|)): one more operation
    p = r + beta p'                       2 u (|r| + beta |p'|), beta = (sqrt(nn) / sqrt(rr))^2 formed as k_cg_resid2 forms it from the
                                          device's own |r|: trace.rnorm holds sqrt(nn), and sqrt(rr) of the pass before.  In pass 1 rr =
                                          |r_0|^2 is not reported: it is summed here from the device's r_0, which differs from the device's
                                          sum by (n + 2) u relative (another order of n terms) -- that term is added to beta |p'| there
    B = B' + alpha p                      u (|B'| + |alpha p|), with or without contraction to an fma
    alpha = rr / pAp                      2 u relative: the trace holds sqrt(nn), whose exact square is nn to 2^-52; the device's division rounds
                                          once (2^-53), and so does the conversion of the exact quotient formed here.  Pass 1: (n + 3) u,
                                          with rr summed here from the device's r_0
    |r| = sqrt(sum r^2)                   n u relative
The outputs of the fast CG are exact arithmetic, P = fma((T) alpha, Pp, P') and dP = tgt - P in the context's type T, and are compared bit
for bit: a ratio of 0 or infinity.  The padded rows of dP (label -1) are exactly zero; those rows feed the gradient GEMM."""
import math
from fractions import Fraction

import numpy as np

import rp_model as rp

NL = rp.NL
U64 = 2.0 ** -52
PATHS = ("folded", "literal", "merged", "fast_conj")
_EX = rp.ExactModel()


# ---- exact arithmetic of the output update ---------------------------------------------------------
def _two_sum(x, y):
    s = x + y
    bb = s - x
    return s, (x - (s - bb)) + (y - bb)


def add_f32(x, y):
    """fl32(x + y) for doubles x, y whose sum is not representable in general, with ONE rounding: the fp64 sum is rounded to odd (the
    neighbour with an odd last bit when inexact), which the second rounding to 24 bits cannot tell from the exact sum"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    s, e = _two_sum(x, y)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return rp.to_f32(s)


def _two_prod(a, b):
    """a b = p + e exactly (Dekker, Veltkamp's split); no overflow at the magnitudes of these tests"""
    p = a * b
    c = 134217729.0
    ah = c * a
    ah = ah - (ah - a)
    al = a - ah
    bh = c * b
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma_t(mode, a, x, y):
    """fma(a, x, y) elementwise in the context's type with one rounding: fp64 by the exact product and math.fsum, the fp32 modes by the
    exact fp64 product of two fp32 numbers and add_f32"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if mode != "f64":
        return add_f32(a * x, y)
    p, e = _two_prod(np.full(x.shape, float(a)), x)
    return np.array([math.fsum(t) for t in zip(p.ravel(), e.ravel(), y.ravel())]).reshape(x.shape)


def sub_t(mode, x, y):
    """x - y in the context's type"""
    return np.asarray(x, dtype=np.float64) - y if mode == "f64" else add_f32(x, -np.asarray(y, dtype=np.float64))


def store(mode, x):
    """a model value as the context's type holds it"""
    return np.asarray(x, dtype=np.float64) if mode == "f64" else rp.to_f32(x)


def alpha_t(mode, a):
    """(T) alpha of k_pupdate"""
    return float(a) if mode == "f64" else float(np.float32(a))


# ---- the launches of a pass, by mode --------------------------------------------------------------------
class Kernels:
    """forward pass, gradient sum, cost and pAp of one bond in one mode: (value, bound).  operands: dict(kind, EI, phiI, phiO, EX, labels,
    target (None: ten labels), per (images per slab of the gradient GEMM, rp.bgemm_cut), fwd ("staged" / "once"), bf16_grad, chain, rows).
    rows: the images the operands are given for, as indices into the NT = len(labels) real images (sparse cases: every other image has
    all-zero features, so its outputs are exactly zero and it adds exact zeros to the image sums); the forward model and its bound are then
    those rows, cost and pAp always take the outputs of all real images"""

    def __init__(self, mode, operands, model=None):
        self.mode, self.o = mode, operands
        self.model = model or (_EX if mode == "f64" else rp._M)
        o = operands
        self.NT = len(o["labels"])
        self.rows = np.arange(self.NT) if o.get("rows") is None else np.asarray(o["rows"])
        assert o["EI"].shape[0] == len(self.rows)
        self.ops = (o["EI"], o["phiI"], o["phiO"], o["EX"])
        self.aops = tuple(np.abs(x) for x in self.ops)
        lab = np.asarray(o["labels"])
        if o.get("target") is None:
            self.tgt = (lab[:, None] == np.arange(NL)[None, :]).astype(np.float64)
        else:
            self.tgt = (lab == o["target"]).astype(np.float64)[:, None]

    def sel(self, x):
        """the modelled rows of an array over the padded images"""
        return np.asarray(x)[:self.NT][self.rows]

    def forward(self, B):
        o, (EI, phiI, phiO, EX) = self.o, self.ops
        if self.mode != "f64":
            return self.model.forward_model(self.mode, o.get("fwd", "staged"), o["kind"], EI, phiI, B, phiO, EX)
        P, _ = self.model.forward_model("f32", "staged", o["kind"], EI, phiI, B, phiO, EX)
        aEI, aphiI, aphiO, aEX = self.aops
        Pa, _ = _EX.forward_model("f32", "staged", o["kind"], aEI, aphiI, np.abs(B), aphiO, aEX)
        return P, (2 * EI.shape[1] * 2 * EX.shape[1] + 4) * U64 * Pa

    def gradient(self, w, Bndim):
        """the image sum with the weights w over all real images"""
        o, (EI, phiI, phiO, EX) = self.o, self.ops
        w = np.asarray(w, dtype=np.float64).reshape(self.NT, -1)[self.rows]
        lab, n = np.asarray(o["labels"])[self.rows], len(self.rows)
        if self.mode != "f64":
            return self.model.gradient_model(self.mode, o["kind"], EI, phiI, phiO, EX, None, lab, o["per"], Bndim, target=o.get("target"),
                                             bf16_grad=o.get("bf16_grad", True), chain=o.get("chain"), weights=w)
        G, _ = self.model.gradient_model("f32", o["kind"], EI, phiI, phiO, EX, None, lab, n, Bndim, weights=w)
        aEI, aphiI, aphiO, aEX = self.aops
        Ga, _ = _EX.gradient_model("f32", o["kind"], aEI, aphiI, aphiO, aEX, None, lab, n, Bndim, weights=np.abs(w))
        terms = n * (NL if o["kind"] != 2 else 1)
        return G, (terms + 4) * U64 * Ga

    def cost(self, P):
        """sum_n sum_l (tgt - P)^2 from the outputs as the device holds them, and its gate"""
        P = np.asarray(P, dtype=np.float64).reshape(self.NT, -1)
        if self.mode != "f64":
            cm = self.model.cost_model(P, self.o["labels"], self.o.get("target"))
            return cm["cost"], cm["cost_gate"]
        d = (self.tgt - P)[self.model.cost_images(self.NT)]
        c = math.fsum((d * d).ravel())
        return c, (d.size + 4) * U64 * c

    def pap_rows(self, Pm):
        """pap of model outputs given for the modelled rows alone (every other image has zero outputs)"""
        full = np.zeros((self.NT, Pm.shape[1]))
        full[self.rows] = Pm
        return self.pap(full)

    def pap(self, Pp):
        Pp = np.asarray(Pp, dtype=np.float64).reshape(self.NT, -1)
        if self.mode != "f64":
            return self.model.pap_model(Pp)
        Pp = Pp[self.model.cost_images(self.NT)]
        s = math.fsum((Pp * Pp).ravel())
        return s, (Pp.size + 4) * U64 * s


# ---- the checker ----------------------------------------------------------------------------------------
def _ratio(dev, model, bound):
    dev, model = np.asarray(dev, dtype=np.float64), np.asarray(model, dtype=np.float64)
    d = np.abs(dev.reshape(model.shape) - model)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), d.shape)
    if not (np.all(np.isfinite(d)) and np.all(np.isfinite(bound))):
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / bound, 0.)                     # bound == 0: the device must give the model's value
    return float(r.max()) if r.size else 0.


def _bits(dev, model):
    """a bit-for-bit relation: 0, or infinity"""
    dev, model = np.asarray(dev, dtype=np.float64), np.asarray(model, dtype=np.float64)
    return 0. if np.array_equal(dev.reshape(model.shape), model) else math.inf


def _sq(x):
    return math.fsum((np.asarray(x, dtype=np.float64) ** 2).ravel())


def _beta(nn_root, rr_root):
    q = nn_root / rr_root                                      # k_cg_resid2: q = sqrt(nn) / sqrt(rr); beta = q * q
    return q * q


def _outputs(out, mode, path, K, st, B, NT, what):
    """P and dP that a state holds against the forward model of B (the start, and every pass of the literal form)"""
    Pm, bound = K.forward(B)
    if path == "literal":                                      # P is not written: dP = tgt - P, one more rounding of the type
        u = U64 / 2 if mode == "f64" else rp.U32
        out[what + " dP=tgt-fwd(B)"] = _ratio(K.sel(st["dP"]), K.sel(K.tgt) - Pm, bound + u * np.abs(K.sel(K.tgt) - Pm))
    else:
        out[what + " P=fwd(B)"] = _ratio(K.sel(st["P"]), Pm, bound)
        out[what + " dP=tgt-P bits"] = _bits(st["dP"][:NT], sub_t(mode, K.tgt, st["P"][:NT]))
    out[what + " dP padded rows zero"] = 0. if not np.any(st["dP"][NT:]) else math.inf


def _pap_and_step(out, mode, path, K, st, tr, k, Bprev, rr, rr_rel, lam):
    """the pAp pass and the step of pass k (1-based) from the state of the run that ends with it: Pp against the forward model of p_k, the
    trace's pAp against pap_model on the device's Pp, alpha = rr / pAp, B_k = Bprev + alpha p_k.  rr: |r_{k-1}|^2 as a Fraction, within rr_rel
    relative of the device's"""
    NT, p, n = K.NT, st["Pv"], st["Pv"].size
    Pm, bound = K.forward(p)
    reg = lam * _sq(p)
    if path == "literal":
        # fast_cg = 0 keeps no p * t.v (the pAp pass writes its sum alone): the sum is held against the forward model itself, inside
        # sum_n 2 |Pm| bound + bound^2 -- what outputs inside their bound can move it by -- beside the gate of the summation
        s, gate = K.pap_rows(Pm)
        slack = float(np.sum(2 * np.abs(Pm) * bound + bound * bound))
        out["pAp trace=fwd(p)"] = abs(tr["pAp"][k - 1] - (s + reg)) / (gate + slack + (n + 2) * U64 * reg)
    else:
        out["pAp Pp=fwd(p)"] = _ratio(K.sel(st["Pp"]), Pm, bound)
        s, gate = K.pap(st["Pp"][:NT])
        out["pAp trace"] = abs(tr["pAp"][k - 1] - (s + reg)) / (gate + (n + 2) * U64 * reg)
        rest = np.setdiff1d(np.arange(NT), K.rows)
        if rest.size:                                          # images without features: outputs exactly zero
            out["pAp Pp zero off the probes"] = 0. if not np.any(st["Pp"][rest]) and not np.any(st["P"][rest]) else math.inf
    a = tr["alpha"][k - 1]
    out["step alpha"] = abs(a - float(rr / Fraction(tr["pAp"][k - 1]))) / ((rr_rel + U64) * abs(a))
    out["step B"] = _ratio(st["B"], Bprev + a * p, U64 * (np.abs(Bprev) + np.abs(a * p)))
    last = all(tr[f][k - 1] == 0. for f in ("cost", "rnorm")) and tr["npass_done"] == k and not tr["converged"]
    out["trace last pass"] = 0. if last else math.inf            # fixedL.cc:409: the last pass of a run reports pAp and alpha only


def check_start(mode, path, after, B0, operands, lam, model=None):
    """the start of the CG from the run of ONE pass: P_0, dP_0, G_0, r_0 = G_0 - lambda B_0, p_1 = r_0 exactly, then pass 1's pAp and step"""
    K = Kernels(mode, operands, model)
    st, tr, NT, out = after, after["trace"], K.NT, {}
    _outputs(out, mode, path, K, st, B0, NT, "start")
    Gm, bound = K.gradient(st["dP"][:NT], B0.ndim)
    out["start G"] = _ratio(st["G"], Gm, bound)
    out["start r=G-lam B"] = _ratio(st["R"], st["G"] - lam * B0, 2 * U64 * (np.abs(st["G"]) + np.abs(lam * B0)))
    out["start p=r bits"] = _bits(st["Pv"], st["R"])
    n = B0.size
    _pap_and_step(out, mode, path, K, st, tr, 1, B0, Fraction(_sq(st["R"])), (n + 2) * U64, lam)
    return out


def check_pass(mode, path, before, after, k, operands, lam, model=None):
    """pass k (1-based): `before` is the state and trace of cgrad(B0, k), `after` of cgrad(B0, k + 1).  Checks the output update, the cost,
    the residual, |r| and the direction of pass k, then the pAp pass and the step of pass k + 1.  Returns {relation: ratio}."""
    assert path in PATHS
    K = Kernels(mode, operands, model)
    NT, out = K.NT, {}
    tb, ta = before["trace"], after["trace"]
    same = all(tb[f][j] == ta[f][j] for f in ("pAp", "alpha") for j in range(k)) and all(tb[f][j] == ta[f][j] for f in ("cost", "rnorm") for j in range(k - 1))
    out["trace prefix bits"] = 0. if same else math.inf             # the prefix runs are the same computation: what the scheme rests on
    Bk, pk, a = before["B"], before["Pv"], tb["alpha"][k - 1]
    n = Bk.size
    # outputs
    if path == "literal":
        _outputs(out, mode, path, K, after, Bk, NT, "outputs")
    elif path == "fast_conj":                                   # no output update on this path: P and dP stay those of B_0
        out["outputs untouched bits"] = max(_bits(after["P"], before["P"]), _bits(after["dP"], before["dP"]))
    else:
        out["outputs P=fma(a,Pp,P) bits"] = _bits(after["P"][:NT], fma_t(mode, alpha_t(mode, a), before["Pp"][:NT], before["P"][:NT]))
        out["outputs dP=tgt-P bits"] = _bits(after["dP"][:NT], sub_t(mode, K.tgt, after["P"][:NT]))
        out["outputs dP padded rows zero"] = 0. if not np.any(after["dP"][NT:]) else math.inf
    # cost of pass k: in the trace of the longer run (literal and folded form: written by pass k; merged: by the step of pass k + 1)
    reg = lam * _sq(Bk)
    if path == "fast_conj":
        out["cost"] = abs(ta["cost"][k - 1] - reg) / ((n + 2) * U64 * reg) if reg else (0. if ta["cost"][k - 1] == 0. else math.inf)
    else:
        Pk = K.tgt - after["dP"][:NT] if path == "literal" else after["P"][:NT]
        if path == "literal":                                     # the cost is a function of dP there
            d = after["dP"][:NT]
            if mode == "f64":
                c = math.fsum((d * d).ravel())
                gate = (d.size + 4) * U64 * c
            else:
                val = K.model._sq_chain(d)[K.model.cost_images(NT)]
                c = math.fsum(val)
                gate = NT * U64 * c + 2.0 ** -23 * val.max()
        else:
            c, gate = K.cost(Pk)
        out["cost"] = abs(ta["cost"][k - 1] - (c + reg)) / (gate + (n + 2) * U64 * reg)
    # residual
    if path in ("folded", "literal"):
        Gm, bound = K.gradient(after["dP"][:NT], Bk.ndim)
        out["residual G"] = _ratio(after["G"], Gm, bound)
        out["residual r=G-lam B"] = _ratio(after["R"], after["G"] - lam * Bk, 2 * U64 * (np.abs(after["G"]) + np.abs(lam * Bk)))
    elif path == "merged":
        Gm, bound = K.gradient(before["Pp"][:NT], Bk.ndim)
        out["residual G=Ap"] = _ratio(after["G"], Gm, bound)
        t = after["G"] + lam * pk
        out["residual r=r-a(Ap+lam p)"] = _ratio(after["R"], before["R"] - a * t, 3 * U64 * (np.abs(before["R"]) + abs(a) * (np.abs(after["G"]) + np.abs(lam * pk))))
    else:                                                         # fast_conj: G <- r - a Ap (k_cg_fast_resid0), then r = G - lambda B
        Gm, bound = K.gradient(before["Pp"][:NT], Bk.ndim)
        out["residual G=r-a Ap"] = _ratio(after["G"], before["R"] - a * Gm, abs(a) * bound + 2 * U64 * (np.abs(before["R"]) + np.abs(a * Gm)))
        out["residual r=G-lam B"] = _ratio(after["R"], after["G"] - lam * Bk, 2 * U64 * (np.abs(after["G"]) + np.abs(lam * Bk)))
    rn = ta["rnorm"][k - 1]
    out["residual |r| trace"] = abs(rn - math.sqrt(_sq(after["R"]))) / (n * U64 * rn)
    # direction
    if k >= 2:
        beta, brel = _beta(rn, ta["rnorm"][k - 2]), 0.
    else:
        beta, brel = _beta(rn, math.sqrt(_sq(before["R"]))), (n + 2) * U64
    out["direction p=r+beta p"] = _ratio(after["Pv"], after["R"] + beta * pk, 2 * U64 * (np.abs(after["R"]) + beta * np.abs(pk)) + brel * beta * np.abs(pk))
    # pass k + 1: pAp and step
    _pap_and_step(out, mode, path, K, after, ta, k + 1, Bk, Fraction(rn) ** 2, U64, lam)
    return out


def check_converged(runs, j, free_j, free_j1):
    """the runs of npass = j + 1, j + 2, ... of a CG that converges in pass j: B, every array of the state and the trace identical bit for
    bit; the trace says so (converged, npass_done = j); and the state is the one the pass left -- B_j and p_j of the unconstrained run of j
    passes (free_j), r_j of the unconstrained run of j + 1 passes (free_j1).  Returns None, or the name of what differs."""
    first = runs[0]
    if first["trace"]["converged"] != 1 or first["trace"]["npass_done"] != j:
        return "converged / npass_done"
    for r in runs[1:]:
        for key in ("B", "Pv", "R", "G", "P", "Pp", "dP"):
            if not np.array_equal(first[key], r[key]):
                return key
        for f in ("npass_done", "converged"):
            if first["trace"][f] != r["trace"][f]:
                return f
        for f in ("cost", "rnorm", "pAp", "alpha"):
            if list(first["trace"][f]) != list(r["trace"][f]):
                return "trace." + f
    if not np.array_equal(first["B"], free_j["B"]):
        return "B against the unconstrained run"
    if not np.array_equal(first["Pv"], free_j["Pv"]):
        return "p against the unconstrained run"
    if not np.array_equal(first["R"], free_j1["R"]):
        return "r against the unconstrained run"
    return None
