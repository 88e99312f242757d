"""The CG at a bond on the device, held pass by pass to the bounds of its own kernels (tests/cg_model.py).

The parity tests compare a whole CG with the oracle, at tolerances that have to admit the rounding the CG amplifies (1e-5 on alpha in fp64,
the operand precision in the reduced modes).  Here every pass is checked from the DEVICE's own state before it: cgrad(B0, k) and
cgrad(B0, k + 1) from the same B0 are two prefix runs of one computation, TrainStates.cg_state copies out what each left, and
cg_model.check_start / check_pass hold every relation between the two states to the bound of the one launch that made it -- the forward and
gradient bounds of rp_model.py in the f32 / bf16 / bf16x3 modes, (terms + 4) 2^-52 sum |terms| in fp64, a few fp64 ulps for the vector kernels,
and bit for bit for the output update P = fma((T) alpha, Pp, P), dP = tgt - P and the zero padded rows.  test_cg_model_host.py shows that the
defects this is after lie at least 10 bounds away at every shape used here.

Every case prints a line `rp_ratio cg ...` with the largest |device - model| / bound over the passes of each group of relations -- start, pAp,
step, trace, outputs, cost, residual, direction; the bit-for-bit relations count 0 or inf (profiles/rp_model_ratios.txt)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cg_model as cg
import rp_model as rp
from test_rp_model_gpu import BF, Chain, _problem

pytestmark = pytest.mark.gpu

NL = rp.NL
MODES = ("f64",) + rp.MODES
K_PASSES = 4
# one bond per Label position on rp.SCALE_DIMS: 3 (16 x 16, Label on the right environment), 4 (40 x 40, on B), 6 (17 x 40, on the left environment)
SMALL_BONDS = {3: (16, 16), **rp.SCALE_THRESHOLD_BONDS}
OPTION_SETS = {"folded": (), "literal": (("fast_cg", 0),), "merged": (("merged_cg", 2),)}
DEFAULTS = {"fast_cg": 1, "merged_cg": 1, "ldot_cfg": 0, "bf16_grad": 1, "bf16_once": 1}


class CgChain(Chain):
    """Chain with the features at the context's precision, the raw CG trace and the CG state"""

    def __init__(self, dims, NT, dtype, case, single=None, options=(), keep=None):
        super().__init__(dims, NT, dtype, case, single, options, keep)
        if dtype == "f64":                                       # an fp64 context holds the features as given
            if single is None:
                phi = _problem(self.N, NT)[1]
                if keep is not None:
                    full, phi = phi, np.zeros_like(phi)
                    phi[keep] = full[keep]
            else:
                from oracle import pyoracle
                from tnml_amd import synth
                phi = pyoracle.features_single(synth.synthetic_images(self.N, self.labels, seed=5), True).copy()
                phi[..., 1] *= 300.0
            self.phi = np.array(phi, dtype=np.float64)
        self.keep = keep

    def run(self, B0, npass, lam, cconv=0.):
        """cgrad(B0, npass): B, the CG vectors and outputs the run left, and the raw trace (zeros behind what the run wrote)"""
        from tnml_amd import lib
        ts = self.ts
        buf, tr = lib.flat(B0), lib.CgTrace()
        ts._ck(ts._L.tnml_cgrad(ts._h, lib.dptr(buf), npass, lam, cconv, C.byref(tr)))
        st = dict(B=buf.reshape(B0.shape, order="F"),
                  trace=dict(npass_done=tr.npass_done, converged=tr.converged, cost=list(tr.cost[:8]), rnorm=list(tr.rnorm[:8]),
                             pAp=list(tr.pAp[:8]), alpha=list(tr.alpha[:8])))
        for w in ("R", "Pv", "G"):
            st[w] = ts.cg_state(w, B0.shape)
        for w in ("P", "Pp", "dP"):
            st[w] = ts.cg_state(w)
        return st

    def cg_operands(self, b, B, once=1, grad=1, chain=None):
        kind, (EI, phiI, phiO, EX) = self.operands(b, B)
        mI, mO = EI.shape[1], EX.shape[1]
        ops = dict(kind=kind, EI=EI, phiI=phiI, phiO=phiO, EX=EX, labels=self.labels, target=self.single)
        if self.keep is not None:
            ops.update(rows=self.keep, EI=EI[self.keep], phiI=phiI[self.keep], phiO=phiO[self.keep], EX=EX[self.keep], chain=chain)
        if self.dtype != "f64":
            L = NL if (kind == 2 and self.single is None) else 1
            ops["per"] = rp.bgemm_cut(self.dtype, mI, mO, L, self.NTp, max(self.dims))["per"]
            ops["fwd"] = "once" if (self.dtype in BF and once == 1 and kind != 2) else "staged"
            ops["bf16_grad"] = grad != 0
        return ops, (mI, mO)

    def set(self, options):
        for k, v in {**DEFAULTS, **dict(options)}.items():
            if k.startswith("bf16") and self.dtype not in BF:
                continue
            self.ts.set_option(k, v)

    def check_cg(self, b, B0, path, lam, ops, dims, npass=K_PASSES, extra=""):
        """the prefix runs of 1 .. npass passes from B0, every relation of every pass; returns the runs"""
        runs = [None] + [self.run(B0, k, lam) for k in range(1, npass + 1)]
        worst = dict(cg.check_start(self.dtype, path, runs[1], B0, ops, lam))
        for k in range(1, npass):
            for key, v in cg.check_pass(self.dtype, path, runs[k], runs[k + 1], k, ops, lam).items():
                worst[key] = max(worst.get(key, 0.), v)
        tag = "%s lam %g%s" % (path, lam, extra)
        groups = {}
        for key, v in worst.items():                             # one line per case: the largest ratio of each group of relations
            g = key.split()[0]
            groups[g] = max(groups.get(g, 0.), v)
        print("rp_ratio cg %-8s %-6s bond %2d kind %d %3d x %-3d NT %5d %-30s %s" %
              (self.case, self.dtype, b, ops["kind"], dims[0], dims[1], self.NT, tag, "  ".join("%s %.3g" % kv for kv in groups.items())))
        bad = {key: v for key, v in worst.items() if not v <= 1.}
        assert not bad, "%s %s bond %d %s: |device - model| / bound %s" % (self.case, self.dtype, b, tag, bad)
        return runs


def _option_sets(dtype):
    """(path, options, label): every path; in the reduced modes both forced forms of the label dot; in the bf16 modes the fp32 gradient
    kernel and the staged feature GEMM"""
    out = [(path, opts, "") for path, opts in OPTION_SETS.items()]
    if dtype != "f64":
        out += [("folded", (("ldot_cfg", f),), " ldot %d" % f) for f in (1, 2)]
    if dtype in BF:
        out += [("folded", (("bf16_grad", 0),), " bf16_grad 0"), ("folded", (("bf16_once", 0),), " bf16_once 0")]
    return out


@pytest.mark.parametrize("b", sorted(SMALL_BONDS))
@pytest.mark.parametrize("dtype", MODES)
def test_every_pass_of_the_cg_on_every_path(dtype, b):
    """rp.SCALE_DIMS at 300 images (512 padded rows: four 128-image units of the output update, 212 padded rows), one bond per Label position,
    lambda = 1e-3 and 0, K = 4 passes: the folded default, fast_cg = 0, merged_cg = 2; both label-dot forms; bf16_grad = 0 and bf16_once = 0"""
    with CgChain(rp.SCALE_DIMS, rp.SCALE_LDOT_NT, dtype, "small") as c:
        assert c.NTp == 512
        B0 = c.goto(b)
        for path, opts, label in _option_sets(dtype):
            c.set(opts)
            o = dict(opts)
            ops, dims = c.cg_operands(b, B0, o.get("bf16_once", 1), o.get("bf16_grad", 1))
            assert dims == SMALL_BONDS[b] and ops["kind"] == {3: 0, 4: 2, 6: 1}[b]
            for lam in (1e-3, 0.):
                c.check_cg(b, B0, path, lam, ops, dims, extra=label)


@pytest.mark.parametrize("dtype", MODES)
def test_every_pass_of_the_cg_at_a_120_x_120_bond(dtype):
    """bond 3 of rp.GRAD_CHAINS[0] (120 x 120, Label on the right environment) at 40 images: the 80 x 80 tile class of the gradient GEMM in
    f32, Kp = Np = 240 in fp64; the folded, the literal and the merged form"""
    dims, bonds = rp.GRAD_CHAINS[0]
    with CgChain(dims, rp.GRAD_NT, dtype, "m120") as c:
        B0 = c.goto(3)
        ops, d = c.cg_operands(3, B0)
        assert d == bonds[3] == (120, 120) and ops["kind"] == 0
        for path, opts in OPTION_SETS.items():
            c.set(opts)
            c.check_cg(3, B0, path, 1e-3, ops, d)


@pytest.mark.parametrize("method", [0, 1], ids=["conj", "fast_conj"])
@pytest.mark.parametrize("dtype", MODES)
def test_per_label_variant(dtype, method):
    """rp.SINGLE_DIMS at 40 images, target label 3, bond 3 (17 x 40): cg_method 0 (the folded form with a label extent of 1) and 1 (fast_conj:
    the residual by recurrence, no output update, no cost -- with lambda = 0 that field stays 0).  The entry check: with cconv above |r_0| no
    pass runs, the flag says so, and B, P and R are bit for bit those before pass 1."""
    b = 3
    with CgChain(rp.SINGLE_DIMS, rp.SINGLE_NT, dtype, "single", single=3) as c:
        B0 = c.goto(b)
        c.ts.set_option("cg_method", method)
        ops, dims = c.cg_operands(b, B0)
        path = "fast_conj" if method else "folded"
        for lam in (1e-3, 0.):
            runs = c.check_cg(b, B0, path, lam, ops, dims)
            if method and lam == 0.:
                assert not any(runs[K_PASSES]["trace"]["cost"]), runs[K_PASSES]["trace"]["cost"]
        one = runs[1]                                             # lambda = 0
        r0 = math.sqrt(float(np.sum(one["R"] ** 2)))
        st = c.run(B0, K_PASSES, 0., 2. * r0)
        assert st["trace"]["npass_done"] == 0 and st["trace"]["converged"] != 0, st["trace"]
        assert np.array_equal(st["B"], B0), "the entry check left a changed B"
        assert np.array_equal(st["P"], one["P"]) and np.array_equal(st["R"], one["R"]) and np.array_equal(st["Pv"], one["R"])


@functools.lru_cache(maxsize=None)
def _oracle_cconv(b, lam):
    """cconv from the oracle's CG at bond b of rp.SCALE_DIMS (300 images, the B0 of CgChain.goto): the geometric mean of |r_j| and |r_{j+1}| of
    the first pass j that at least halves |r|"""
    from oracle import pyoracle
    from test_gpu_parity import _mps_with_dims
    N, NT = len(rp.SCALE_DIMS) - 1, rp.SCALE_LDOT_NT
    labels, phi = _problem(N, NT)
    o = pyoracle.Oracle(phi, labels, _mps_with_dims(rp.SCALE_DIMS, 11))
    o.init()
    for bb in range(1, b):
        o.shiftE(bb, True)
    o.set_bond(b)
    B = o.bond_tensor(b)
    B0 = B + 0.1 * np.abs(B).max() * np.random.default_rng(2).standard_normal(B.shape)
    rn = o.cgrad(B0, 8, lam, 0.)[1]["rnorm"]
    js = [i for i in range(len(rn) - 1) if rn[i] / rn[i + 1] >= 2.]
    assert js, "no pass of the oracle's CG at bond %d halves |r|: %s -- another bond or seed is needed" % (b, rn)
    return math.sqrt(rn[js[0]] * rn[js[0] + 1])


@pytest.mark.parametrize("path", ["folded", "merged"])
@pytest.mark.parametrize("dtype", MODES)
def test_converged_cg_is_frozen_whatever_the_pass_count(dtype, path):
    """cconv between two residual norms of the oracle's CG that lie a factor of two apart (asserted on the oracle's trace), at the Label-on-B
    bond of rp.SCALE_DIMS.  j, the pass whose |r| first falls below it, is read from the device's own unconstrained run (bf16 operands move
    |r|; asserted to leave three passes to spare).  Runs of j + 1, j + 2, j + 3 and 8 passes: converged, npass_done = j, and B, every array of
    the state and the trace identical bit for bit -- later passes read the flag from both parity slots.  B and p are those of the
    unconstrained run of j passes, r that of j + 1 passes: the direction is not updated in the pass that converges."""
    b, lam = 4, 1e-3
    cconv = _oracle_cconv(b, lam)
    with CgChain(rp.SCALE_DIMS, rp.SCALE_LDOT_NT, dtype, "converge") as c:
        B0 = c.goto(b)
        c.set(OPTION_SETS[path])
        rn = c.run(B0, 8, lam)["trace"]["rnorm"][:7]
        below = [i for i in range(7) if rn[i] < cconv]
        assert below and below[0] + 1 + 3 <= 8, "cconv %g against the device's |r| %s" % (cconv, rn)
        j = below[0] + 1
        runs = [c.run(B0, n, lam, cconv) for n in (j + 1, j + 2, j + 3, 8)]
        free = [c.run(B0, n, lam) for n in (j, j + 1)]
        bad = cg.check_converged(runs, j, free[0], free[1])
        print("rp_ratio cg converge  %-6s bond %2d %-7s cconv %.4g converging pass %d: %s" % (dtype, b, path, cconv, j, bad or "identical"))
        assert bad is None, "%s %s: runs of %d, %d, %d and 8 passes with cconv = %g differ in %s" % (dtype, path, j + 1, j + 2, j + 3, cconv, bad)


@pytest.mark.parametrize("NT", sorted(rp.SCALE_THRESHOLD))
@pytest.mark.parametrize("dtype", rp.MODES)
def test_every_pass_of_the_cg_at_real_image_counts(dtype, NT):
    """24 320 and 24 576 images, on either side of the threshold of the streaming label dot, no kernel-selection option set, K = 3 passes at the
    40 x 40 bond with the Label on B and the 17 x 40 bond with the Label on the left environment.  Every image outside rp.probe_set of the
    bond's slab cut has all-zero features: its outputs are exactly zero (asserted by the checker) and it adds exact zeros to the image sums,
    so the model runs on the probes and a lost or doubled chunk of the output update or of the gradient is thousands of bounds away.  The
    label-dot form is recognised by its bits, as in test_rp_model_gpu.py."""
    want = rp.SCALE_THRESHOLD[NT]
    kinds = {bb: (k, LL) for bb, k, _, _, LL in rp.bonds_of(rp.SCALE_DIMS)}
    for b, (mI, mO) in rp.SCALE_THRESHOLD_BONDS.items():
        kind, L = kinds[b]
        cut = rp.bgemm_cut(dtype, mI, mO, L, NT, max(rp.SCALE_DIMS))
        S, chain = rp.probe_set(cut, NT)
        with CgChain(rp.SCALE_DIMS, NT, dtype, "scale", keep=S) as c:
            assert c.NTp == NT
            B0 = c.goto(b)
            ops, dims = c.cg_operands(b, B0, chain=chain)
            assert dims == (mI, mO) and ops["kind"] == kind
            c.check_cg(b, B0, "folded", 1e-3, ops, dims, npass=3, extra=" probes %d chain %d" % (len(S), chain))
            P = c.ts.forward(B0).reshape(NT, -1)
            forced = {}
            for form in (1, 2):
                c.ts.set_option("ldot_cfg", form)
                forced[form] = c.ts.forward(B0).reshape(NT, -1)
            c.ts.set_option("ldot_cfg", 0)
            assert np.array_equal(P, forced[want]), "bond %d at %d images: the default label dot is not form %d" % (b, NT, want)
            if mO >= 17:
                assert not np.array_equal(P[S], forced[3 - want][S]), "bond %d at %d images: both forms return the same bits" % (b, NT)
