"""The kernels of the reduced-precision modes (dtype f32, bf16, bf16x3) against a model of their own rounding (tests/rp_model.py).

The existing gates of these modes are the OPERAND precision against the fp64 oracle (3e-2 for bf16): anything smaller than the operand
rounding passes them.  Here the reference rounds the same operands at the same places as the kernel and sums in fp64, so that what is left
is fp32 accumulation, and the gate is the derived worst-case bound of rp_model.py -- |device - model| <= bound for every element.  The
model takes the device's own inputs (TrainStates.env, the fp32 features, the bond tensor as passed; for the gradient the P the device
returned), so every comparison isolates one launch sequence.  test_rp_model_host.py proves the model and shows that the defects this is
after (truncation instead of rounding, a dropped cross term, a dropped reduction index or image chunk, a stale bf16 copy, a swapped
epilogue index) lie at least 10 bounds away at every shape used here.

Every check prints a line `rp_ratio ...` with the largest |device - model| / bound (profiles/rp_model_ratios.txt is that list).

The last part runs the same gate PER KERNEL at real image counts (up to 25 000) on one short chain with maxm = 40 (rp.SCALE_DIMS): both forms
of the fp32 label dot, forced at 300 images and by the default dispatch on either side of its threshold of 192 blocks, with the scalar epilogue
(cost, per-label costs, #correct, pAp) held to rp.cost_model / rp.pap_model on the device's own P -- lines `rp_gate ...`, |device - model| / gate;
and the gradient GEMM at the slab cuts of 24 576 and 25 000 images, sparse (every image outside a probe set is zero, so that the chain of the
bound is the probes of one slab and a lost or doubled chunk is thousands of bounds away) and dense (the bound with the full slab length)."""
import functools

import numpy as np
import pytest

import rp_model as rp
import tiled_reference as tr
from conftest import make_problem
from test_gpu_parity import _mps_with_dims

pytestmark = pytest.mark.gpu

NL = rp.NL
BF = ("bf16", "bf16x3")


def _ratio(dev, model, bound):
    d = np.abs(np.asarray(dev, dtype=np.float64).reshape(model.shape) - model)
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / bound, 0.)                      # bound == 0 (every product zero): the device must give the model's value
    return float(r.max())


@functools.lru_cache(maxsize=None)
def _problem(N, NT):
    """(labels, features) of make_problem(N, NT, seed 5), made once per image count and left unchanged"""
    _, labels, phi, _ = make_problem(N, NT, 2, 5, pixel_boost=200.0)
    labels.flags.writeable = phi.flags.writeable = False
    return labels, phi


class Chain:
    """a TrainStates context on a chain with prescribed link dimensions, and what the model needs beside the device's environments"""

    def __init__(self, dims, NT, dtype, case, single=None, options=(), keep=None):
        """keep: the images that keep their features (every other image gets all-zero features at every site)"""
        from tnml_amd.fixedl import TrainStates
        self.dims, self.N, self.NT, self.dtype, self.case, self.single = dims, len(dims) - 1, NT, dtype, case, single
        self.NTp = -(-NT // rp.NTPAD) * rp.NTPAD
        if single is None:
            self.labels, phi = _problem(self.N, NT)
            if keep is not None:
                full, phi = phi, np.zeros_like(phi)
                phi[keep] = full[keep]
            self.W = _mps_with_dims(dims, 11)
        else:
            from oracle import pyoracle
            from tnml_amd import synth
            self.labels = synth.synthetic_labels(NT, seed=5, per_label=NT // 10 if NT % 10 == 0 else None)
            phi = pyoracle.features_single(synth.synthetic_images(self.N, self.labels, seed=5), True).copy()
            phi[..., 1] *= 300.0
            self.W = tr.plain_mps_with_dims(dims, 11)
        self.phi = rp.to_f32(phi)                                # the context stores the features in fp32
        self.ts = TrainStates(self.labels, self.N, max(dims), phi=phi, dtype=dtype, single_label=single)
        for k, v in options:
            self.ts.set_option(k, v)
        self.ts.set_mps(self.W)
        self.ts.init()
        self.rng = np.random.default_rng(2)
        self.at = 1
        self.one = np.ones((NT, 1))

    def report(self, what, kernel, b, kind, mI, mO, r, extra=""):
        print("rp_ratio %-9s %-6s %-8s %-14s bond %2d kind %d %3d x %-3d NT %3d%s  ratio %.3f" %
              (self.case, self.dtype, what, kernel, b, kind, mI, mO, self.NT, extra, r))
        assert r <= 1.0, "%s %s %s (%s) at bond %d (kind %d, %d x %d, %d images%s): |device - model| = %.3f x bound" % (
            self.case, self.dtype, what, kernel, b, kind, mI, mO, self.NT, extra, r)

    def operands(self, b, B):
        """(kind, (EI, phiI, phiO, EX)) of bond b from the device's own environments"""
        ts = self.ts
        EL = ts.env(b - 1) if b > 1 else self.one
        ER = ts.env(b + 2) if b + 2 <= self.N else self.one
        kind = rp.kind_of(B, EL, ER)
        return kind, rp.plan(kind, EL, self.phi[:, b - 1], ER, self.phi[:, b])

    def goto(self, b):
        """to bond b by shifts from the left (unchecked: the shift kernels have their cases above); returns a perturbed bond tensor"""
        for bb in range(self.at, b):
            self.ts.shiftE(bb, True)
        self.at = b
        self.ts.setBond(b)
        B = self.ts.bond_tensor(b)
        return B + 0.1 * np.abs(B).max() * self.rng.standard_normal(B.shape)

    def forward_check(self, b, B, once, extra="", ops=None):
        """forward at the bond that is set, with option bf16_once = once (None: not a bf16 mode); returns the device's P"""
        ts = self.ts
        kind, (EI, phiI, phiO, EX) = ops if ops is not None else self.operands(b, B)
        if once is not None:
            ts.set_option("bf16_once", once)
        path = "once" if (once == 1 and kind != 2) else "staged"
        P = ts.forward(B).reshape(self.NT, -1)
        Pm, bound = rp.forward_model(self.dtype, path, kind, EI, phiI, B, phiO, EX)
        kernel = "k_fgemm_bf16e" if path == "once" else ("k_fgemm/f32" if self.dtype == "f32" else "k_fgemm/bf16")
        self.report("forward", kernel, b, kind, EI.shape[1], EX.shape[1], _ratio(P, Pm, bound), extra)
        return P, kind, (EI, phiI, phiO, EX)

    def epilogue_check(self, b, B, P, extra=""):
        """the scalar epilogue of the label dot: quadcost(B) against rp.cost_model on P = forward(B) as the device returned it, and pAp(p)
        against rp.pap_model on forward(p).  #correct exactly, the regulariser and lambda |p|^2 (fp64) to 1e-12, every cost inside its gate"""
        ts, lam = self.ts, 1e-3
        C, lc, cr, nc = ts.quadcost(B, lam)
        cm = rp.cost_model(P, self.labels, self.single)
        assert cr == pytest.approx(lam * float(np.sum(B * B)), rel=1e-12)
        rl = float((np.abs(lc - cm["label_cost"]) / cm["gate"]).max())
        rc = abs(C - (cm["cost"] + cr)) / (cm["cost_gate"] + 1e-12 * cr)
        p = np.abs(B).max() * self.rng.standard_normal(B.shape)
        s, gate = rp.pap_model(ts.forward(p))
        reg = lam * float(np.sum(p * p))
        rp_ = abs(ts.pAp(p, lam) - (s + reg)) / (gate + 1e-12 * reg)
        print("rp_gate  %-9s %-6s bond %2d NT %5d%s  #correct %d (model %d)  cost %.2g per-label %.2g pAp %.2g" %
              (self.case, self.dtype, b, self.NT, extra, nc, cm["ncorrect"], rc, rl, rp_))
        assert nc == cm["ncorrect"], "%s %s bond %d%s: #correct %d, from the device's own P %d" % (self.case, self.dtype, b, extra, nc, cm["ncorrect"])
        assert max(rc, rl, rp_) <= 1.0, "%s %s bond %d%s: cost %.3g, per-label cost %.3g, pAp %.3g x gate" % (self.case, self.dtype, b, extra, rc, rl, rp_)

    def check(self, b, expect=None, gradient=True):
        """forward (both settings of bf16_once) and gradient (both settings of bf16_grad) at bond b against the model"""
        ts, bf = self.ts, self.dtype in BF
        ts.setBond(b)
        B = ts.bond_tensor(b)
        B = B + 0.1 * np.abs(B).max() * self.rng.standard_normal(B.shape)
        kind = None
        for once in ((0, 1) if bf else (None,)):
            if once == 1 and kind == 2:                         # Label on B: bf16_once changes nothing, the staged kernel has run
                ts.set_option("bf16_once", 1)
                continue
            P, kind, (EI, phiI, phiO, EX) = self.forward_check(b, B, once)
        mI, mO, L = EI.shape[1], EX.shape[1], (P.shape[1] if kind == 2 else 1)
        if expect is not None:
            assert (mI, mO) == expect, (b, mI, mO, expect)
        cut = rp.bgemm_cut(self.dtype, mI, mO, L, self.NTp, max(self.dims))
        if gradient:
            for grad in ((1, 0) if bf else (None,)):
                if grad is not None:
                    ts.set_option("bf16_grad", grad)
                G = ts.gradient(B)                              # its weights: the forward pass of the same B with the options as they stand (P above)
                Gm, bound = rp.gradient_model(self.dtype, kind, EI, phiI, phiO, EX, P, self.labels, cut["per"], B.ndim,
                                              target=self.single, bf16_grad=grad != 0)
                self.report("gradient", "k_bgemm/bf16" if grad == 1 else "k_bgemm/f32", b, kind, mI, mO, _ratio(G, Gm, bound),
                            " tile %d slabs %d x %d" % (cut["tile"], cut["nsplit"], cut["per"]))
            if bf:
                ts.set_option("bf16_grad", 1)
        return kind, cut

    def shift(self, b):
        """shiftE(b, from the left) and the new environment against shift_model on the device's previous one"""
        ts = self.ts
        prev = ts.env(b - 1) if b > 1 else None
        ts.shiftE(b, True)
        E = ts.env(b)
        Em, bound = rp.shift_model(self.dtype, prev, self.phi[:, b - 1], self.W[b - 1], True)
        lab = "on the environment" if prev is not None and prev.ndim == 3 else ("on the site" if E.ndim == 3 else "nowhere")
        self.report("shift", "k_fgemm/f32", b, 0, self.dims[b - 1], self.dims[b], _ratio(E, Em, bound), " Label " + lab)
        self.at = b + 1

    def shift_from_right(self, b):
        """shiftE(b, from the right): the environment of site b + 1 from that of site b + 2 (none: the chain end)"""
        ts = self.ts
        prev = ts.env(b + 2) if b + 2 <= self.N else None
        ts.shiftE(b, False)
        E = ts.env(b + 1)
        Em, bound = rp.shift_model(self.dtype, prev, self.phi[:, b], self.W[b], False)
        lab = "on the environment" if prev is not None and prev.ndim == 3 else ("on the site" if E.ndim == 3 else "nowhere")
        self.report("shift<-", "k_fgemm/f32", b, 0, self.dims[b + 1], self.dims[b], _ratio(E, Em, bound), " Label " + lab)

    def walk(self, bonds, gradient=True):
        """visit the bonds in `bonds` (a dict bond -> expected (mI, mO), or an iterable) from the left; every shift on the way is checked"""
        out = {}
        for b in range(self.at, max(bonds) + 1):
            if b in bonds:
                out[b] = self.check(b, bonds[b] if isinstance(bonds, dict) else None, gradient)
                self.shift(b)
            else:
                self.shift(b)
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ts.close()


@pytest.mark.parametrize("dtype", rp.MODES)
def test_forward_tile_classes_and_reduction_padding(dtype):
    """every bond of [1, 2, 16, 17, 33, 64, 65, 120, 40, 2, 1] at 40 images: Np <= 32, <= 64, > 64 and == 240 of k_fgemm on the fp32 pipe, <= 64 and > 64
    on the bf16 pipe, a reduction that fills its last 32-chunk (mI = 16) and one that leaves 30 padded rows (17), KH / QP of k_fgemm_bf16e exact
    (32 / 64) and one past (33, 65), the extent-1 edge bonds; Label on the right environment, on B, on the left environment"""
    with Chain(rp.FORWARD_DIMS, 40, dtype, "forward") as c:
        seen = c.walk(range(1, c.N))
        assert sorted(k for k, _ in seen.values()) == [0, 0, 0, 1, 1, 1, 1, 2, 2]
        for b in range(c.N - 1, 0, -1):                         # and back: the right-to-left form of the shift at every site
            c.shift_from_right(b)


@pytest.mark.parametrize("chain", range(len(rp.GRAD_CHAINS)))
@pytest.mark.parametrize("dtype", rp.MODES)
def test_gradient_tile_classes(dtype, chain):
    """(mI, mO) = (40, 40), (80, 40), (120, 120), (33, 17), (16, 16), (9, 5) with the Label on an environment and on B: launch_bgemm's
    80 x 80 class (whose Kp is ru32(2 mI) in the bf16 modes: (40, 40) leaves it there and (80, 40) enters it), 64 x 64 and 32 x 32.  At 40
    images (256 padded) the cut of the 32 x 32 bonds is one 32-image chunk per slab (120 x 120 with the Label on B: four slabs of two)."""
    dims, bonds = rp.GRAD_CHAINS[chain]
    with Chain(dims, rp.GRAD_NT, dtype, "grad%d" % chain) as c:
        seen = c.walk(bonds)
        NTp = c.NTp
    want = {(40, 40): 80 if dtype == "f32" else 64, (80, 40): 80, (120, 120): 80 if dtype == "f32" else 64, (33, 17): 64, (16, 16): 32, (9, 5): 32}
    for b, (kind, cut) in seen.items():
        assert cut["tile"] == want[bonds[b]], (b, bonds[b], cut)
        if cut["tile"] == 32:                                    # a handful of tiles: 1024 / tiles is more than the 8 chunks there are
            assert cut["per"] == 32 and cut["nsplit"] == NTp // 32, "bond %d: %d tiles -> %d slabs of %d images, expected one chunk per slab" % (b, cut["tiles"], cut["nsplit"], cut["per"])
    assert {k for k, _ in seen.values()} == ({1, 2} if chain == 2 else {0, 1, 2})


@pytest.mark.parametrize("dtype", rp.MODES)
def test_slab_cut_with_a_short_last_slab(dtype):
    """m = 150 with the Label on B at 700 (768 padded) images: 5 x 5 x 10 = 250 tiles of 64 x 64 -> ceil(1024 / 250) = 5 slabs over 24 chunks ->
    ceil(24 / 5) = 5 chunks = 160 images per slab, the last slab holds 128"""
    with Chain(rp.SLAB_DIMS, rp.SLAB_NT, dtype, "slab") as c:
        (kind, cut), = c.walk({rp.SLAB_BOND: (150, 150)}).values()
        assert kind == 2 and c.NTp == 768
    assert (cut["tiles"], cut["nsplit"], cut["per"], cut["last"]) == (250, 5, 160, 128), \
        "the cut computed from %d tiles is %d slabs of %d images (last %d): this case is about five slabs of 160 with a last one of 128" % (cut["tiles"], cut["nsplit"], cut["per"], cut["last"])


@pytest.mark.parametrize("NT", rp.RAGGED_NTS)
@pytest.mark.parametrize("dtype", rp.MODES)
def test_ragged_image_counts(dtype, NT):
    """130 and 257 images at m = 61 (126 and 255 padded ones): the model sums the real images only, so padded images that contributed to
    a real row of P or to G would show"""
    with Chain(rp.RAGGED_DIMS, NT, dtype, "ragged") as c:
        seen = c.walk({b: (61, 61) for b in rp.RAGGED_BONDS})
        assert c.NTp - NT in (126, 255) and {k for k, _ in seen.values()} == {0, 2}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_per_label_variant(dtype):
    """single_label: every bond runs the Label-on-B plan with a label extent of 1"""
    with Chain(rp.SINGLE_DIMS, rp.SINGLE_NT, dtype, "single", single=3) as c:
        seen = c.walk(range(1, c.N))
        assert all(k == 2 for k, _ in seen.values())
        for b in range(c.N - 1, 0, -1):
            c.shift_from_right(b)


@pytest.mark.parametrize("dtype", BF)
def test_bf16_copy_of_the_environment_follows_shifts_and_the_host_tier(dtype):
    """launch_fgemm_bf16e keeps a bf16 copy of its input environment, keyed on pointer, dimension and epoch.  Forward at bond 6 of a
    24-site chain (Label on the right environment: the copy is of the left environment of site 5).  Then site 4 is changed by less than a
    percent and the shifts of sites 4 and 5 are redone: the environment of site 5 is rewritten -- same dimension, the slot it had -- with
    values that moved by less than a percent.  The second forward pass must follow the model on the NEW environment and must differ from
    the first by more than the bound (the bound is far below the movement, so a copy that was kept would show).  Then to bond 21 by shifts
    from the left and back by shifts from the right, and forward at bond 6 a third time: the bits of the second.  Under env_budget_mb = 2
    (four slabs) the slab of the left environments 1 .. 10 is the farthest one while the Label-carrying right environments 12 .. 7 are
    rebuilt from bond 21 and goes to the host: the last setBond(6) has to fetch site 5 back.  Every result of that run equals the run
    without a budget bit for bit."""
    from tnml_amd.fixedl import TrainStates
    N, NT, m, b, far = rp.STALE["N"], rp.STALE["NT"], rp.STALE["m"], rp.STALE["bond"], rp.STALE["far"]
    _, labels, phi, W = make_problem(N, NT, m, 11, pixel_boost=200.0)
    phi32 = rp.to_f32(phi)

    def fwd(ts, B, what):
        ts.setBond(b)
        EL, ER = ts.env(b - 1), ts.env(b + 2)
        kind = rp.kind_of(B, EL, ER)
        EI, phiI, phiO, EX = rp.plan(kind, EL, phi32[:, b - 1], ER, phi32[:, b])
        P = ts.forward(B)
        Pm, bound = rp.forward_model(dtype, "once", kind, EI, phiI, B, phiO, EX)
        r = _ratio(P, Pm, bound)
        print("rp_ratio %-9s %-6s %-8s %-14s bond %2d kind %d %3d x %-3d NT %3d %s  ratio %.3f" % ("stale", dtype, "forward", "k_fgemm_bf16e", b, kind, EI.shape[1], EX.shape[1], NT, what, r))
        assert kind == 0 and r <= 1.0, (what, r)
        return P, bound, EL

    def run(budget):
        ts = TrainStates(labels, N, m, phi=phi, dtype=dtype)
        try:
            if budget:
                ts.set_option("env_budget_mb", budget)
            ts.set_option("bf16_once", 1)
            ts.set_mps(W)
            ts.init()
            for bb in range(1, b):
                ts.shiftE(bb, True)
            ts.setBond(b)
            rng = np.random.default_rng(3)
            B = ts.bond_tensor(b)
            B = B + 0.05 * np.abs(B).max() * rng.standard_normal(B.shape)
            P1, bound1, E1 = fwd(ts, B, "first")
            ts.set_site(b - 2, W[b - 3] * (1.0 - 0.008 * rng.uniform(0.5, 1.0, W[b - 3].shape)))      # site 4 moves by < 1 % ...
            ts.shiftE(b - 2, True)
            ts.shiftE(b - 1, True)                                   # ... and with it the environment of site 5
            P2, bound2, E2 = fwd(ts, B, "input environment moved")
            drift = float(np.abs(E2 - E1).max() / np.abs(E1).max())
            moved = _ratio(P2, P1, np.maximum(bound1, bound2))
            for bb in range(b, far):                                 # to the far bond
                ts.shiftE(bb, True)
            ts.setBond(far)
            for bb in range(far - 1, b - 1, -1):                     # and back: the right environments far .. b + 1 are rebuilt
                ts.shiftE(bb, False)
            f0 = ts.env_stats()["fetches"]
            ts.setBond(b)
            fetched = ts.env_stats()["fetches"] - f0
            P3, _, _ = fwd(ts, B, "after the walk to bond %d and back" % far)
            return P1, P2, P3, fetched, ts.env_stats(), drift, moved
        finally:
            ts.close()
    free = run(0)
    print("stale %s: the input environment moved by %.2e relative, P by %.3g x bound" % (dtype, free[5], free[6]))
    assert free[4]["spills"] == 0
    assert 0 < free[5] < 1e-2
    assert free[6] > 1.0, "P follows an environment that moved by %.1e only within the bound: a stale copy would pass" % free[5]
    assert np.array_equal(free[1], free[2])
    tight = run(2)
    print("host tier: %s, fetches at the last setBond(%d): %d" % (tight[4], b, tight[3]))
    assert tight[4]["slabs"] <= 4 and tight[4]["spills"] > 0
    assert tight[3] >= 1, "the input environment of bond %d was not on the host in between: this case no longer tests the copy cache under the host tier" % b
    for x, y in zip(free[:3], tight[:3]):
        assert np.array_equal(x, y)


# ---- at real image counts, per kernel (rp.SCALE_DIMS: maxm = 40) ---------------------------------------------------------------------
def _both_forms(c, b, B, once, ops):
    """forward under ldot_cfg = 1 (k_labeldot<8, 2>: 128-image blocks, non-temporal loads) and 2 (<16, 1>: 64-image blocks), each against the
    model and each twice with the same bits; {form: P}"""
    out = {}
    for form in (1, 2):
        c.ts.set_option("ldot_cfg", form)
        out[form] = c.forward_check(b, B, once, " ldot %d" % form, ops)[0]
        assert np.array_equal(out[form], c.ts.forward(B).reshape(c.NT, -1)), "bond %d, label-dot form %d: forward twice, different bits" % (b, form)
    return out


@pytest.mark.parametrize("dtype,single", [(d, None) for d in rp.MODES] + [("f32", 3), ("bf16", 3)], ids=lambda v: "per-label" if v == 3 else (v or "ten-labels"))
def test_both_forms_of_the_fp32_label_dot_and_their_scalar_epilogue(dtype, single):
    """300 images, every bond of rp.SCALE_DIMS, ldot_cfg = 1 and 2 (NLT = 10; NLT = 1 in the per-label variant): P inside the bound of
    forward_model, cost / per-label costs / #correct / pAp from the device's own P inside the gates of cost_model and pap_model.  The two forms
    sum the label dot in different orders wherever a wave of either holds more than one row: their P must differ in some bit at every
    bond with mO >= 17, or this case no longer tells them apart."""
    bf = dtype in BF
    with Chain(rp.SCALE_DIMS, rp.SCALE_LDOT_NT, dtype, "ldot", single=single) as c:
        for b in range(1, c.N):
            B = c.goto(b)
            ops = c.operands(b, B)
            for once in ((0, 1) if bf and ops[0] != 2 else (0,) if bf else (None,)):
                P = _both_forms(c, b, B, once, ops)
                for form in (1, 2):
                    c.ts.set_option("ldot_cfg", form)
                    c.epilogue_check(b, B, P[form], " ldot %d" % form)
                if ops[1][3].shape[1] >= 17:
                    assert not np.array_equal(P[1], P[2]), "bond %d (mO = %d): the 128-image and the 64-image form of the label dot return the same bits: " \
                        "this case no longer tells them apart" % (b, ops[1][3].shape[1])
            c.ts.set_option("ldot_cfg", 0)


@pytest.mark.parametrize("NT", sorted(rp.SCALE_THRESHOLD))
@pytest.mark.parametrize("dtype", rp.MODES)
def test_default_label_dot_dispatch_on_either_side_of_its_threshold(dtype, NT):
    """24 320 images (190 blocks of 128: the 64-image form) and 24 576 (192: the streaming form k_labeldot<8, 2, 10, float, float, float>), no
    kernel-selection option set, at the 40 x 40 bond with the Label on B and the 17 x 40 bond with the Label on the left environment.  P is dense
    and every image is held to forward_model's per-image bound; cost, per-label costs, #correct and pAp to cost_model / pap_model on that P.
    The form is recognised by its bits: P under ldot_cfg = 0 equals P under the form the threshold predicts and differs from the other."""
    bf = dtype in BF
    want = rp.SCALE_THRESHOLD[NT]
    with Chain(rp.SCALE_DIMS, NT, dtype, "dispatch") as c:
        assert c.NTp == NT
        for b, expect in rp.SCALE_THRESHOLD_BONDS.items():
            B = c.goto(b)
            ops = c.operands(b, B)
            assert (ops[1][0].shape[1], ops[1][3].shape[1]) == expect
            for once in ((0, 1) if bf and ops[0] != 2 else (0,) if bf else (None,)):
                P = c.forward_check(b, B, once, " default", ops)[0]
                c.epilogue_check(b, B, P, " default")
            forced = {}
            for form in (1, 2):
                c.ts.set_option("ldot_cfg", form)
                forced[form] = c.ts.forward(B).reshape(NT, -1)
            c.ts.set_option("ldot_cfg", 0)
            assert np.array_equal(P, forced[want]), "bond %d at %d images: the default label dot is not form %d" % (b, NT, want)
            assert not np.array_equal(P, forced[3 - want]), "bond %d at %d images: both forms return the same bits" % (b, NT)


def _grad_options(bf):
    return (1, 0) if bf else (None,)


@pytest.mark.parametrize("NT", rp.SCALE_NTS)
@pytest.mark.parametrize("dtype", rp.MODES)
def test_gradient_with_long_slabs_on_sparse_probes(dtype, NT):
    """24 576 and 25 000 images: 12 slabs of 2 048 / 2 112 images (f32, 40 x 40 with the Label on B; the last of 1 856 at 25 000), 79 slabs of
    320 with a last one of 128 (16 x 16 at 25 000), hundreds of 32-image chunks per workgroup.  Every image outside rp.probe_set of the bond's
    cut has all-zero features: its environments and outputs are zero on the device (asserted) and it adds exact zeros to G, so the model is
    gradient_model on the probes alone (test_rp_model_host.py: the same bits) and the chain of its bound is the probes of one slab --
    a chunk lost, summed twice, or a lost slab lies thousands of bounds away.  Both settings of bf16_grad in the bf16 modes."""
    bf = dtype in BF
    cuts = {}
    for b, (mI, mO) in rp.SCALE_GRAD_BONDS.items():
        kind, L = {bb: (k, LL) for bb, k, _, _, LL in rp.bonds_of(rp.SCALE_DIMS)}[b]
        cut = cuts[b] = rp.bgemm_cut(dtype, mI, mO, L, -(-NT // rp.NTPAD) * rp.NTPAD, max(rp.SCALE_DIMS))
        S, chain = rp.probe_set(cut, NT)
        rest = np.setdiff1d(np.arange(NT), S)
        with Chain(rp.SCALE_DIMS, NT, dtype, "sparse", keep=S) as c:
            B = c.goto(b)
            k, (EI, phiI, phiO, EX) = c.operands(b, B)
            assert k == kind and (EI.shape[1], EX.shape[1]) == (mI, mO)
            if bf:
                c.ts.set_option("bf16_once", 0)
            P = c.ts.forward(B).reshape(NT, -1)
            assert not EI[rest].any() and not EX[rest].any() and not P[rest].any(), "bond %d: an image without features has a non-zero environment or output" % b
            assert EI[S].any(axis=1).all() and EX[S].reshape(len(S), -1).any(axis=1).all() and P[S].any(axis=1).all()
            for grad in _grad_options(bf):
                if grad is not None:
                    c.ts.set_option("bf16_grad", grad)
                G = c.ts.gradient(B)
                Gm, bound = rp.gradient_model(dtype, kind, EI[S], phiI[S], phiO[S], EX[S], P[S], c.labels[S], cut["per"], B.ndim, bf16_grad=grad != 0, chain=chain)
                c.report("gradient", "k_bgemm/bf16" if grad == 1 else "k_bgemm/f32", b, kind, mI, mO, _ratio(G, Gm, bound),
                         " tile %d slabs %d x %d last %d probes %d chain %d" % (cut["tile"], cut["nsplit"], cut["per"], cut["last"], len(S), chain))
    if dtype == "f32":                                                  # the cuts this case is about
        assert cuts[4]["per"] >= 2048 and cuts[4]["tile"] == 80
        if NT == 25000:
            assert 0 < cuts[4]["last"] < cuts[4]["per"] and cuts[5]["nsplit"] >= 79 and cuts[5]["last"] < cuts[5]["per"]
    else:
        assert cuts[4]["per"] >= 1664 and cuts[4]["last"] < cuts[4]["per"] and cuts[4]["tile"] == 64
    assert cuts[5]["tile"] == 32 and cuts[6]["tile"] == 64


@pytest.mark.parametrize("dtype", rp.MODES)
def test_gradient_with_long_slabs_dense(dtype):
    """the same bonds at 24 576 images with ordinary features against gradient_model with the full slab length (up to 2 048 images summed
    in fp32 by one workgroup): the derived bound, ratio <= 1 -- the measured figure of these modes at a real image count.  On an MI355X
    the largest ratio at per = 2 048 is quoted in DESIGN.md (tolerance study) from profiles/rp_model_ratios.txt."""
    with Chain(rp.SCALE_DIMS, rp.SCALE_NTS[0], dtype, "dense") as c:
        for b, expect in rp.SCALE_GRAD_BONDS.items():
            c.goto(b)
            kind, cut = c.check(b, expect)
            if b == 4:
                assert kind == 2 and cut["per"] >= (2048 if dtype == "f32" else 1664), cut
