"""The per-pass checker of the CG (tests/cg_model.py) proved before it judges the device -- no GPU.

`emulate` restates cgrad_device (tnml_bond.hip) and its kernels k_cg_init1/2, k_cg_step2, k_cg_resid1/2, k_cg_fast_resid0, k_pupdate launch by
launch in numpy, in every mode and on every path; its roundings are those of rp_model (to_f32, the planes, the fma emulation) and the exact
fma / difference of cg_model.  The big sums are the models' fp64 sums, so an emulated state differs from a model of its own pass by the
roundings of the storage type alone.

1. the states of prefix runs of the emulation pass check_start / check_pass with every ratio <= 1, in every mode and on every path;
2. with exact operands the emulation follows oracle.pyoracle's cgrad (fast_cgrad for fast_conj) to fp64 tolerance;
3. each planted defect of the emulation shows a ratio >= 10 in some relation, at every shape test_cg_model_gpu.py runs;
4. the weights= extension of rp.gradient_model: with exact operands, A p formed with weights p * t.v equals the oracle's gradient
   difference (G(B) - G(B + p) = A p, the sum being linear in the weights), and weights = tgt - P reproduces the unextended model bit for bit."""
import functools
import math

import numpy as np
import pytest

import cg_model as cg
import rp_model as rp
from conftest import make_problem

NL = rp.NL
MODES = ("f64",) + rp.MODES
K_PASSES = 4
MAXP = 8
# (name, dims, NT, bond, per-label target): the bonds test_cg_model_gpu.py runs -- one per Label position at 300 images, the 120 x 120 bond, the per-label variant
SHAPES = [("scale-b3", rp.SCALE_DIMS, rp.SCALE_LDOT_NT, 3, None), ("scale-b4", rp.SCALE_DIMS, rp.SCALE_LDOT_NT, 4, None),
          ("scale-b6", rp.SCALE_DIMS, rp.SCALE_LDOT_NT, 6, None), ("grad0-b3", rp.GRAD_CHAINS[0][0], rp.GRAD_NT, 3, None),
          ("single-b3", rp.SINGLE_DIMS, rp.SINGLE_NT, 3, 3)]
# at real image counts on the sparse probe set of each mode's slab cut (K = 3 passes there)
SPARSE = [("sparse-%d-b%d" % (NT, b), NT, b) for NT in sorted(rp.SCALE_THRESHOLD) for b in rp.SCALE_THRESHOLD_BONDS]


# ---- the emulation ---------------------------------------------------------------------------------------
def emulate(mode, path, operands, B0, npass, lam, cconv=0., defect=None, model=None):
    """cgrad_device for `npass` passes from B0: dict(B, Pv, R, G, P, Pp, dP, trace) as TrainStates.cg_state / the raw trace would return them"""
    K = cg.Kernels(mode, operands, model)
    NT, L = K.NT, K.tgt.shape[1]
    NTp = -(-NT // rp.NTPAD) * rp.NTPAD
    fast, merged, fastc = path != "literal", path == "merged", path == "fast_conj"
    single = operands.get("target") is not None
    tr = dict(npass_done=0, converged=0, cost=[0.] * MAXP, rnorm=[0.] * MAXP, pAp=[0.] * MAXP, alpha=[0.] * MAXP)
    sq = lambda x: float(np.sum(np.asarray(x) ** 2))
    B = np.array(B0, dtype=np.float64)

    def fwd(X):                                               # the outputs of all real images (zero where an image has no features)
        full = np.zeros((NT, L))
        full[K.rows] = K.forward(X)[0]
        return full
    # grad_eval: forward pass of B (P kept with the fast CG), dP, the gradient sum; k_cg_init1 / k_cg_init2
    Pfull = cg.store(mode, fwd(B))
    dP = cg.sub_t(mode, K.tgt, Pfull)
    P = Pfull if fast else np.zeros_like(Pfull)              # fast_cg = 0: the P buffer is not the CG's
    G = K.gradient(dP, B.ndim)[0]
    r = G - lam * B if lam != 0. else G.copy()
    p = r.copy()
    rr = [sq(r), 0.]                                          # the two |r|^2 slots
    slot = 0
    flag = [0., 0.]                                           # SC_CONVP by pass parity
    if single and math.sqrt(rr[0]) < cconv:                   # the entry check of the per-label variant (single.h:202-206)
        flag[0] = 2.
        tr["converged"] = 2
    Pp = np.zeros_like(P)
    cost_late = cost_prev = bn2 = alpha_prev = a = 0.
    pn2_part = 0.
    rd = (lambda ps: ps & 1) if defect == "flag parity" else (lambda ps: (ps - 1) & 1)     # the slot the kernels of pass ps read
    for ps in range(1, npass + 1):
        Pp = cg.store(mode, fwd(p))                           # the pAp pass is not gated by the flag
        pp = K.pap(Pp)[0]
        if merged and ps < npass:
            G = K.gradient(Pp, B.ndim)[0]                     # A p, before alpha is known
        # k_cg_step2
        if merged and ps > 1 and flag[ps & 1] == 0.:
            tr["cost"][ps - 2] = cost_late
        if flag[rd(ps)] == 0.:
            pn2 = rr[slot] if ps == 1 else pn2_part
            pAp = pp + lam * pn2
            a = rr[slot] / pAp
            B = B + a * p
            tr["pAp"][ps - 1], tr["alpha"][ps - 1], tr["npass_done"] = pAp, a, ps
        if ps == npass:
            break
        live = flag[rd(ps)] == 0.
        # the output update / the forward pass of the new B, then the image sum
        if live and fast and not fastc:
            au = alpha_prev if defect == "previous alpha" else a
            at = float(au) if defect == "alpha not rounded" else cg.alpha_t(mode, au)
            Pn = cg.fma_t(mode, at, Pp, P) if defect != "alpha not rounded" else cg.store(mode, at * Pp + P)
            if defect == "skip last unit":
                lo = 128 * ((NT - 1) // 128)                  # the last 128-image unit that holds a real image
                Pn[lo:] = P[lo:]
            P = Pn
            dP = cg.sub_t(mode, K.tgt, P)
        elif not fast:
            dP = cg.sub_t(mode, K.tgt, cg.store(mode, fwd(B)))
        if fastc:
            if live:
                G = r - a * K.gradient(Pp, B.ndim)[0]         # k_cg_fast_resid0; no cost on this path
            cs = 0.
        else:
            cs = K.cost(P)[0] if fast else (float(np.sum(dP * dP)) if mode == "f64" else math.fsum(K.model._sq_chain(dP)))
            if not merged:
                G = K.gradient(dP, B.ndim)[0]
        alpha_prev = a if live else alpha_prev
        # k_cg_resid1 / k_cg_resid2
        was = flag[rd(ps)]
        if was != 0.:
            flag[ps & 1] = was
            continue
        if merged:
            t = G + lam * p if lam != 0. and defect != "lambda p missing" else G
            nr = r - a * t
        else:
            nr = G - lam * B if lam != 0. and defect != "lambda B missing" else G.copy()
        nn, bn2 = sq(nr), sq(B)
        rr_in = rr[slot ^ 1] if (defect == "beta slot" and ps >= 2) else rr[slot]
        q = math.sqrt(nn) / math.sqrt(rr_in)
        beta, rn = q * q, math.sqrt(nn)
        conv = rn < cconv
        r = nr
        if not conv or defect == "p updated on convergence":
            p = nr + beta * p
            pn2_part = sq(p)
        if merged:
            cost_late = cs + lam * bn2
        else:
            c_now = cs + lam * bn2
            tr["cost"][ps - 1] = cost_prev if (defect == "cost one pass late" and ps >= 2) else c_now
            cost_prev = c_now
        tr["rnorm"][ps - 1] = rn
        rr[slot ^ 1] = nn
        slot ^= 1
        flag[ps & 1] = float(conv)
        tr["converged"] = int(conv)

    def pad(x, fill_defect=False):
        out = np.zeros((NTp, L))
        out[:NT] = x
        if fill_defect:
            out[NT:] = 1.                                     # tgt - P without the label test
        return out
    if not fast:
        Pp = np.full_like(Pp, 7.)                             # fast_cg = 0: the pAp pass keeps no p * t.v -- whatever the buffer held
    return dict(B=B, Pv=p, R=r, G=G, P=pad(P), Pp=pad(Pp), dP=pad(dP, defect == "padded dP"), trace=tr)


# ---- operands at the shapes of the GPU tests, from the oracle ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    from oracle import pyoracle
    _, dims, NT, b, target = next(s for s in SHAPES if s[0] == name)
    N = len(dims) - 1
    if target is None:
        from test_gpu_parity import _mps_with_dims
        _, labels, phi, _ = make_problem(N, NT, 2, 5, pixel_boost=200.0)
        o = pyoracle.Oracle(phi, labels, _mps_with_dims(dims, 11))
    else:
        import tiled_reference as tr
        from tnml_amd import synth
        labels = synth.synthetic_labels(NT, seed=5, per_label=NT // 10)
        phi = pyoracle.features_single(synth.synthetic_images(N, labels, seed=5), True).copy()
        phi[..., 1] *= 300.0
        o = pyoracle.SingleOracle(phi, labels, target, tr.plain_mps_with_dims(dims, 11))
    o.init()
    for bb in range(1, b):
        o.shiftE(bb, True)
    o.set_bond(b)
    B = o.bond_tensor(b)
    B0 = B + 0.1 * np.abs(B).max() * np.random.default_rng(2).standard_normal(B.shape)
    one = np.ones((NT, 1))
    EL = o.env(b - 1) if b > 1 else one
    ER = o.env(b + 2) if b + 2 <= N else one
    kind = rp.kind_of(B0, EL, ER)
    EI, phiI, phiO, EX = rp.plan(kind, EL, phi[:, b - 1], ER, phi[:, b])
    return o, B0, dict(kind=kind, EI=EI, phiI=phiI, phiO=phiO, EX=EX, labels=labels, target=target), max(dims)


def _operands(name, mode):
    o, B0, ops, maxm = _case(name)
    ops = dict(ops)
    NT = ops["EI"].shape[0]
    L = NL if (ops["kind"] == 2 and ops["target"] is None) else 1
    if mode != "f64":
        ops["per"] = rp.bgemm_cut(mode, ops["EI"].shape[1], ops["EX"].shape[1], L, -(-NT // rp.NTPAD) * rp.NTPAD, maxm)["per"]
        ops["fwd"] = "once" if (mode != "f32" and ops["kind"] != 2) else "staged"
    return o, B0, ops


@functools.lru_cache(maxsize=None)
def _sparse_oracle(NT, b, mode):
    """the oracle at bond b of rp.SCALE_DIMS with every image outside the probe set of `mode`'s slab cut stripped of its features"""
    from oracle import pyoracle
    from test_gpu_parity import _mps_with_dims
    dims = rp.SCALE_DIMS
    N = len(dims) - 1
    kind, mI, mO, L = next((k, a, c, LL) for bb, k, a, c, LL in rp.bonds_of(dims) if bb == b)
    cut = rp.bgemm_cut(mode, mI, mO, L, NT, max(dims))
    S, chain = rp.probe_set(cut, NT)
    _, labels, full, _ = make_problem(N, NT, 2, 5, pixel_boost=200.0)
    sub = pyoracle.Oracle(np.ascontiguousarray(full[S]), labels[S], _mps_with_dims(dims, 11))      # the environments of the probes are their own
    sub.init()
    for bb in range(1, b):
        sub.shiftE(bb, True)
    sub.set_bond(b)
    B = sub.bond_tensor(b)
    B0 = B + 0.1 * np.abs(B).max() * np.random.default_rng(2).standard_normal(B.shape)
    one = np.ones((len(S), 1))
    EL = sub.env(b - 1) if b > 1 else one
    ER = sub.env(b + 2) if b + 2 <= N else one
    assert rp.kind_of(B0, EL, ER) == kind
    EI, phiI, phiO, EX = rp.plan(kind, EL, full[S][:, b - 1], ER, full[S][:, b])
    return B0, dict(kind=kind, EI=EI, phiI=phiI, phiO=phiO, EX=EX, labels=labels, target=None, rows=S, chain=chain, per=cut["per"],
                    fwd="once" if (mode != "f32" and kind != 2) else "staged")


def _paths(name):
    return ("folded", "fast_conj") if name.startswith("single") else ("folded", "literal", "merged")


def _all_ratios(mode, path, ops, B0, lam, runs):
    worst = dict(cg.check_start(mode, path, runs[1], B0, ops, lam))
    for k in range(1, len(runs) - 1):
        for key, v in cg.check_pass(mode, path, runs[k], runs[k + 1], k, ops, lam).items():
            worst["pass %s" % key] = max(worst.get("pass %s" % key, 0.), v)
    return worst


# ---- 1. the emulation passes its own checker -----------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
@pytest.mark.parametrize("mode", MODES)
def test_emulated_prefix_runs_pass_every_relation(mode, name, capsys):
    lines = []
    for path in _paths(name):
        for lam in (1e-3, 0.):
            if name == "grad0-b3" and (lam == 0. or path != "folded"):
                continue                                              # the big bond once: the relations are those of the small ones
            _, B0, ops = _operands(name, mode)
            runs = [None] + [emulate(mode, path, ops, B0, k, lam) for k in range(1, K_PASSES + 1)]
            res = _all_ratios(mode, path, ops, B0, lam, runs)
            lines.append("  %-9s %-6s %-9s lambda %-6g worst %.3g (%s)" % (name, mode, path, lam, max(res.values()), max(res, key=res.get)))
            bad = {k: v for k, v in res.items() if not v <= 1.}
            assert not bad, (name, mode, path, lam, bad)
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")


@pytest.mark.parametrize("name", [s[0] for s in SPARSE])
@pytest.mark.parametrize("mode", rp.MODES)
def test_emulated_prefix_runs_on_sparse_probes_pass_every_relation(mode, name):
    """the sparse cases at real image counts: the model runs on the probes, cost and pAp on every image"""
    B0, ops = _sparse_oracle(*next(s[1:] for s in SPARSE if s[0] == name), mode)
    runs = [None] + [emulate(mode, "folded", ops, B0, k, 1e-3) for k in range(1, 4)]
    res = _all_ratios(mode, "folded", ops, B0, 1e-3, runs)
    assert "pAp Pp zero off the probes" in res and "pass pAp Pp zero off the probes" in res
    bad = {k: v for k, v in res.items() if not v <= 1.}
    assert not bad, (name, mode, bad)


# ---- 2. exact operands: the oracle's CG ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scale-b3", "scale-b4", "scale-b6", "single-b3"])
def test_emulation_with_exact_operands_follows_the_oracle(name, capsys):
    """every path computes the reference's CG in exact arithmetic: the trace (pAp, alpha, |r|, cost of every pass) to 1e-8 relative.  What is
    left is fp64 rounding in another summation order, amplified by the passes: 1e-13 in the literal forms at these bonds, 1e-11 at the
    Label-on-B bond, 1e-9 in the fourth pass of the residual recurrence of fast_conj (printed).  B itself is not compared: at the
    Label-on-B bond it moves by 5e-8 where its cost moves by 1e-15.  The suite's tolerance for the device's alpha is 1e-5."""
    o, B0, ops = _operands(name, "f64")
    lam = 1e-3
    for path in _paths(name):
        fastc = path == "fast_conj"
        Bo, to = (o.fast_cgrad if fastc else o.cgrad)(B0, K_PASSES, lam, 0.)
        st = emulate("f64", path, ops, B0, K_PASSES, lam)
        te = st["trace"]
        err = 0.
        for f in ("pAp", "alpha", "rnorm") + (() if fastc else ("cost",)):
            n = K_PASSES if f in ("pAp", "alpha") else K_PASSES - 1
            assert len(to[f]) >= n, (f, to)
            err = max(err, max(abs(te[f][j] - to[f][j]) / abs(to[f][j]) for j in range(n)))
        with capsys.disabled():
            print("\n  %-9s %-9s emulation vs oracle: %.1e" % (name, path, err), end="")
        assert te["npass_done"] == to["npass_done"] == K_PASSES and err < 1e-8, (name, path, err)


# ---- 3. planted defects ---------------------------------------------------------------------------------
# defect -> (the path it lives on, the modes; None: all)
DEFECTS = {"previous alpha": ("folded", None), "alpha not rounded": ("folded", rp.MODES), "skip last unit": ("folded", None), "padded dP": ("folded", None),
           "beta slot": ("folded", None), "cost one pass late": ("folded", None), "lambda p missing": ("merged", None), "lambda B missing": ("literal", None)}


@pytest.mark.parametrize("mode,name", [(m, s[0]) for m in MODES for s in SHAPES] + [(m, s[0]) for m in rp.MODES for s in SPARSE])
def test_every_planted_defect_shows_at_least_ten_bounds(mode, name, capsys):
    """every defect on the path it lives on, at every bond test_cg_model_gpu.py runs (the per-label variant and the sparse cases at real image
    counts run the folded form alone there; fp64 is not run at real image counts, and 24 320 and 24 576 images have no padded rows)"""
    sparse = name.startswith("sparse")
    if sparse:
        B0, ops = _sparse_oracle(*next(s[1:] for s in SPARSE if s[0] == name), mode)
    else:
        _, B0, ops = _operands(name, mode)
    lam, lines = 1e-3, []
    for defect, (path, modes) in DEFECTS.items():
        if (modes is not None and mode not in modes) or (path != "folded" and (sparse or name.startswith("single"))):
            continue
        if defect == "padded dP" and len(ops["labels"]) % rp.NTPAD == 0:
            continue
        runs = [None] + [emulate(mode, path, ops, B0, k, lam, defect=defect) for k in range(1, (3 if sparse else K_PASSES) + 1)]
        res = _all_ratios(mode, path, ops, B0, lam, runs)
        worst = max(res.values())
        lines.append("  %-9s %-6s %-22s %.3g (%s)" % (name, mode, defect, worst, max(res, key=res.get)))
        assert worst >= 10., "%s %s: '%s' shows only %.3g x bound" % (name, mode, defect, worst)
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")


def _converging(name, mode, path, lam=1e-3):
    """cconv: the geometric mean of |r_j| and |r_{j+1}| of the first pass j of the oracle's CG with |r_j| / |r_{j+1}| >= 2"""
    o, B0, ops = _operands(name, mode)
    _, to = o.cgrad(B0, 8, lam, 0.)
    rn = to["rnorm"]
    js = [i for i in range(len(rn) - 1) if rn[i] / rn[i + 1] >= 2.]
    assert js, "no pass of the oracle's CG halves |r| at %s: %s" % (name, rn)
    i = js[0]                                                          # rn[i] is |r| after pass i + 1: pass i + 2 is the first below cconv
    return math.sqrt(rn[i] * rn[i + 1]), B0, ops


@pytest.mark.parametrize("path", ["folded", "merged"])
@pytest.mark.parametrize("mode", MODES)
def test_convergence_defects_break_the_identity_of_the_runs(mode, path):
    """the convergence case of the GPU tests on the emulation: the runs of npass = j + 1, j + 2, j + 3 and 8 are identical, B is that of the
    unconstrained run of j passes, p that run's and r the next one's; a flag read from the wrong parity slot and a direction updated in
    the converging pass each break it"""
    name, lam = "scale-b4", 1e-3
    cconv, B0, ops = _converging(name, mode, path)
    rn = emulate(mode, path, ops, B0, 8, lam)["trace"]["rnorm"][:7]
    j = 1 + next(i for i in range(7) if rn[i] < cconv)                  # the converging pass in this mode's own arithmetic (bf16 operands move |r|)
    assert j + 3 <= 8
    for defect in (None, "flag parity", "p updated on convergence"):
        runs = [emulate(mode, path, ops, B0, n, lam, cconv, defect) for n in (j + 1, j + 2, j + 3, 8)]
        free = [emulate(mode, path, ops, B0, n, lam, 0., defect) for n in (j, j + 1)]
        bad = cg.check_converged(runs, j, free[0], free[1])
        if defect is None:
            assert bad is None, (mode, path, bad)
            assert runs[0]["trace"]["converged"] == 1 and runs[0]["trace"]["npass_done"] == j
        else:
            assert bad is not None, "%s %s: '%s' leaves the converged runs identical" % (mode, path, defect)


# ---- 4. the weights= extension of gradient_model ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["scale-b3", "scale-b4", "scale-b6", "single-b3"])
def test_gradient_model_with_given_weights(name):
    o, B0, ops = _operands(name, "f64")
    ex = rp.ExactModel()
    NT = ops["EI"].shape[0]
    p = np.abs(B0).max() * np.random.default_rng(9).standard_normal(B0.shape)
    args = (ops["kind"], ops["EI"], ops["phiI"], ops["phiO"], ops["EX"])
    Pp = np.asarray(o.forward(p)).reshape(NT, -1)
    Ap, _ = ex.gradient_model("f32", *args, None, ops["labels"], 32, B0.ndim, target=ops["target"], weights=Pp)
    want = o.gradient(B0) - o.gradient(B0 + p)                       # sum_n (tgt - P) v - sum_n (tgt - P - Pp) v
    assert np.abs(Ap - want).max() <= 1e-11 * np.abs(want).max()
    for mode in rp.MODES:                                               # weights = fl32(tgt - P): the unextended model, bit for bit
        P = rp.to_f32(np.asarray(o.forward(B0)).reshape(NT, -1))
        K = cg.Kernels(mode, dict(ops, per=64))
        G0, b0 = rp.gradient_model(mode, *args, P, ops["labels"], 64, B0.ndim, target=ops["target"])
        G1, b1 = rp.gradient_model(mode, *args, None, ops["labels"], 64, B0.ndim, target=ops["target"], weights=rp.to_f32(K.tgt - P))
        assert np.array_equal(G0, G1) and np.array_equal(b0, b1)
