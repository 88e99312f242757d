"""The per-label variant (TNML_MODE_SINGLE: single.cc / single.h) at real bond dimensions against its oracle (oracle/single_oracle.c).

Every bond of the variant runs the "Label on B" plan (kind 2) with a label extent of 1: the forward pass takes the label dot with A = U,
Bv = EX and NLT = 1, the gradient the weighted (w / Zq32) branch of the four unfused k_bgemm64 instantiations with a slab cut computed for
L = 1, the split with noise its own rocBLAS + k_noise_weights + k_noise_add path -- none of which the fixedL tests reach, and the per-label
tests of test_gpu_parity.py stay at bond dimension <= 8.  Here: chains with unequal and odd bond dimensions up to 300 (part 1), every tile
class of the gradient / forward kernels on m x m bonds with forced variants and the launch table (2), the noise split with mL != mR (3),
whole bond updates in lockstep (4), the unforced dispatch at 30 720 images against the tiled ground truth (5), two ranks at m = 64 (6).

Chains are plain MPS with prescribed link dimensions (tiled_reference.plain_mps_with_dims).  The "uniform" chains are [1, 2, m, ..., m, 2, 1]:
synth.random_mps caps a link at 2^min(j, N - j), 64 on 12 sites, and would never give the 120 x 120 bonds these tests are about.
Tolerances are those of test_gpu_parity.py (TOL; the f32 row of test_bonds_with_unequal_and_odd_dimensions) and of the existing per-label
tests (1e-7 / 1e-6 for fast_conj and sweep costs, 1e-8 in lockstep).  Every truncation below is decided by maxm / minm, or by the cutoff
with a margin: the oracle's new bond dimension is the same at ten times and at a tenth of the cutoff (checked when the seeds were chosen;
test_single_oracle.py pins the ground truth itself at unequal dimensions)."""
import os
import threading

import numpy as np
import pytest

import tiled_reference as tr
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

LAM, CCONV, NPASS = 1e-3, 1e-10, 4
TARGET = 3
_NTH = min(8, os.cpu_count() or 1)
F32 = dict(E=2e-5, P=2e-5, G=5e-4, C=2e-4)        # the f32 row of test_bonds_with_unequal_and_odd_dimensions (ftol, gtol; costs at 10 ftol)

CHAINS = [[1, 2, 3, 5, 9, 17, 33, 65, 120, 2, 1],
          [1, 2, 120, 97, 64, 60, 61, 128, 33, 2, 1],
          [1, 2, 4, 150, 129, 200, 300, 257, 16, 2, 1]]
SMALL_UNEQUAL = [1, 2, 4, 7, 13, 24, 31, 17, 8, 4, 2, 1]


def uniform_dims(N, m):
    """every interior link of dimension m: bonds 2 ... N - 2 are m x m"""
    return [1, 2] + [m] * (N - 3) + [2, 1]


def single_problem(dims, NT, seed=5, boost=300.0):
    """(labels, phi, W): synthetic images under the per-label feature map with the second component boosted, a plain MPS with link dimensions
    `dims`; labels evenly filled where 10 divides NT, after the MNIST histogram otherwise"""
    from oracle import pyoracle
    from tnml_amd import synth
    N = len(dims) - 1
    labels = synth.synthetic_labels(NT, seed=seed, per_label=NT // 10 if NT % 10 == 0 else None)
    pixels = synth.synthetic_images(N, labels, seed=seed)
    phi = pyoracle.features_single(pixels, True).copy()
    phi[..., 1] *= boost
    return labels, phi, tr.plain_mps_with_dims(dims, seed + 6)


def _pair(dims, NT, seed=5, dtype="f64", maxm=None, target=TARGET, options=()):
    """TrainStates(..., single_label=target) beside pyoracle.SingleOracle on the same problem, environments of init built on both"""
    from oracle import pyoracle
    from tnml_amd.fixedl import TrainStates
    labels, phi, W = single_problem(dims, NT, seed)
    ts = TrainStates(labels, len(dims) - 1, max(max(dims), maxm or 0), phi=phi, dtype=dtype, single_label=target)
    for k, v in options:
        ts.set_option(k, v)
    o = pyoracle.SingleOracle(phi, labels, target, W, nthread=_NTH)
    ts.set_mps(W)
    o.init()
    ts.init()
    return ts, o


def _perturbed(B, scale, seed):
    return B + scale * np.abs(B).max() * np.random.default_rng(seed).standard_normal(B.shape)


def _walk_to(ts, o, at, b):
    for bb in range(at, b):
        ts.shiftE(bb, True); o.shiftE(bb, True)
    ts.setBond(b); o.set_bond(b)


def _launches(ts):
    return {k: v[0] for k, v in ts.profile_read().items() if v[0]}


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. single evaluations on unequal and odd bonds
def _evaluate_every_bond(dims, NT, dtype):
    ts, o = _pair(dims, NT, dtype=dtype)
    N = len(dims) - 1
    T = TOL.get(dtype, F32)
    exact = dtype == "f64"
    y = np.asarray(o.labels) == o.target
    f = np.array([o.output(i) for i in range(NT)])
    w = ts.classify()[0]                                         # the decision function of separate_fulltest.cc (tnml_classify)
    assert w.shape == (NT, 1)
    print("  %s NT %d %s: decision function %.1e" % (dims, NT, dtype, tr.relmax(w[:, 0], f)))
    assert tr.relmax(w[:, 0], f) < (T["P"] if dtype in TOL else 10 * T["P"])
    for j in range(3, N + 1):
        assert tr.relmax(ts.env(j), o.env(j)) < T["E"], j
    rng = np.random.default_rng(2)
    for b in range(1, N):
        ts.setBond(b); o.set_bond(b)
        B = o.bond_tensor(b)
        assert B.shape == (dims[b - 1], 2, 2, dims[b + 1]) == ts.bond_shape(b)
        B = B + 0.1 * np.abs(B).max() * rng.standard_normal(B.shape)
        Po, Pg = o.forward(B), ts.forward(B)
        Go, Gg = o.gradient(B), ts.gradient(B)
        Cg, lg, crg, ng = ts.quadcost(B, LAM)
        Co, cro = o.quadcost(B, LAM)
        ts.shiftE(b, True); o.shiftE(b, True)
        eE = tr.relmax(ts.env(b), o.env(b))
        print("  bond %2d (%3d x %3d): P %.1e G %.1e cost %.1e env %.1e" % (b, B.shape[0], B.shape[3], tr.relmax(Pg, Po), tr.relmax(Gg, Go), abs(Cg / Co - 1), eE))
        assert tr.relmax(Pg, Po) < T["P"], b
        assert tr.relmax(Gg, Go) < T["G"], b
        assert Cg == pytest.approx(Co, rel=T["C"]), b
        assert lg.sum() + crg == pytest.approx(Cg, rel=1e-12) and crg == pytest.approx(cro, rel=1e-12), b
        hit_o = (Po > 0.5) == y                                   # evaluated in fp64 by the oracle
        if exact:
            assert ng == int(hit_o.sum()), b
        else:
            # reduced storage may move an output across 1/2, but only one that lies within the output tolerance of it: the count is that of the
            # kernel's own outputs, and every image decided differently from the oracle is such an image
            hit_g = (Pg > 0.5) == y
            assert ng == int(hit_g.sum()), b
            assert (np.abs(Po - 0.5)[hit_g != hit_o] <= T["P"] * np.abs(Po).max()).all(), b
        assert eE < T["E"], b
    ts.close()


@pytest.mark.parametrize("dtype", ["f64", "f64_e32", "f32"])
@pytest.mark.parametrize("dims", CHAINS, ids=["grow-to-120", "unequal-60-128", "above-120"])
def test_every_bond_of_chains_with_unequal_and_odd_dimensions(dims, dtype):
    """The three chains of test_bonds_with_unequal_and_odd_dimensions without the Label index, 40 images: the decision function, then at every
    bond, left to right, forward, gradient, cost / regulariser / #correct (against (f > 1/2) == (label == target) of the oracle's fp64
    outputs) and the environment the shift leaves -- every (Kp, Np) class of the kind-2 plan at label extent 1, mL != mR, odd sizes."""
    _evaluate_every_bond(dims, 40, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f64_e32", "f32"])
@pytest.mark.parametrize("NT", [1, 37, 257])
def test_ragged_image_counts_on_an_unequal_chain(NT, dtype):
    """the second chain again at 1 image (the target label is absent: y = 0 throughout), 37 and 257 (labels after the MNIST histogram,
    unevenly filled; 257 is one image past two 128-image blocks): padding images must contribute nothing"""
    _evaluate_every_bond(CHAINS[1], NT, dtype)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. tile classes of the gradient and forward kernels at label extent 1
N_UNI = 12
BONDS_UNI = (4, 8)                                               # one bond left of the middle, one right of it


def _compare_cg(ts, o, B, tag):
    """four passes of conj (cg_method 0) and of fast_conj (cg_method 1) from B against the oracle's cgrad / fast_cgrad"""
    F = TOL["f64"]
    ts.set_option("cg_method", 0)
    Bg, tg = ts.cgrad(B, NPASS, LAM, CCONV)
    Bo, to = o.cgrad(B, NPASS, LAM, CCONV)
    assert not tg["skipped"] and not to["skipped"] and tg["npass_done"] == to["npass_done"] == NPASS, tag
    print("   conj: cost %.1e alpha %.1e B %.1e" % (tr.relmax(tg["cost"], to["cost"]), max(abs(a / b - 1) for a, b in zip(tg["alpha"], to["alpha"])), tr.relmax(Bg, Bo)))
    np.testing.assert_allclose(tg["cost"], to["cost"], rtol=F["cgc"], err_msg=str(tag))
    np.testing.assert_allclose(tg["alpha"], to["alpha"], rtol=F["cga"], err_msg=str(tag))
    assert tr.relmax(Bg, Bo) < F["cga"], tag
    ts.set_option("cg_method", 1)
    Bf, tf = ts.cgrad(B, NPASS, LAM, CCONV)
    ts.set_option("cg_method", 0)
    Bfo, tfo = o.fast_cgrad(B, NPASS, LAM, CCONV)
    assert not tf["skipped"] and tf["npass_done"] == NPASS, tag
    print("   fast_conj: alpha %.1e |r| %.1e B %.1e" % (max(abs(a / b - 1) for a, b in zip(tf["alpha"], tfo["alpha"])), tr.relmax(tf["rnorm"], tfo["rnorm"]), tr.relmax(Bf, Bfo)))
    np.testing.assert_allclose(tf["alpha"], tfo["alpha"], rtol=1e-7, err_msg=str(tag))
    np.testing.assert_allclose(tf["rnorm"], tfo["rnorm"], rtol=1e-6, err_msg=str(tag))
    assert tr.relmax(Bf, Bfo) < 1e-6, tag
    return Bg, tg


@pytest.mark.parametrize("m,NT", [(12, 300), (40, 300), (61, 300), (120, 300), (150, 300), (120, 1100), (40, 256), (120, 512)])
def test_gradient_and_forward_tile_classes_at_label_extent_one(m, NT):
    """m x m bonds on 12 sites: 2m pads to 32 (the 32 x 32 gradient tiles <1,1,2,2>), 80 (<1,5,5,1>), 128 and 304 (<2,2,2,2>), 240 (<5,1,3,5>);
    300 images, and 1 100 at m = 120 (more slabs, a ragged last one).  256 and 512 images fill the padded count (a multiple of 256) exactly: only
    there are the last images of the last slab real ones -- at every other count a slab cut that loses its tail loses padding.  At a bond on either side of the middle: gradient and forward (each
    repeated: the same bits), four passes of conj and of fast_conj against the oracle."""
    F = TOL["f64"]
    ts, o = _pair(uniform_dims(N_UNI, m), NT)
    at = 1
    for b in BONDS_UNI:
        _walk_to(ts, o, at, b)
        at = b
        B0 = o.bond_tensor(b)
        assert B0.shape == (m, 2, 2, m)
        B = _perturbed(B0, 0.05, b)
        G, P = ts.gradient(B), ts.forward(B)
        print("  m %d NT %d bond %d: G %.1e P %.1e" % (m, NT, b, tr.relmax(G, o.gradient(B)), tr.relmax(P, o.forward(B))))
        assert tr.relmax(G, o.gradient(B)) < F["G"], b
        assert tr.relmax(P, o.forward(B)) < F["P"], b
        assert np.array_equal(G, ts.gradient(B)) and np.array_equal(P, ts.forward(B)), b
        _compare_cg(ts, o, B, (m, NT, b))
    ts.close()


def test_forced_kernel_variants_at_m120_agree_with_the_unforced_result():
    """m = 120, 300 images: the 128 x 240 forward tile (fg64_cfg = 2), both NLT = 1 label dots (ldot_cfg = 1: 128-image blocks, 2: 64-image
    blocks), other slab cuts of the gradient GEMM (bgemm_wgs = 8, back to 0, bgemm_per = 2: 64 images per slab).  Each changes a tile or the
    summation order only: within 1e-13 (relative) of the unforced result, within the parity tolerances of the oracle, and the same bits when
    the call is repeated."""
    F = TOL["f64"]
    ts, o = _pair(uniform_dims(N_UNI, 120), 300)
    at = 1
    for b in BONDS_UNI:
        _walk_to(ts, o, at, b)
        at = b
        B = _perturbed(o.bond_tensor(b), 0.05, b)
        Po, Go, Co = o.forward(B), o.gradient(B), o.quadcost(B, LAM)[0]
        P0, G0, C0 = ts.forward(B), ts.gradient(B), ts.quadcost(B, LAM)
        for name, value in (("fg64_cfg", 2), ("ldot_cfg", 1), ("ldot_cfg", 2), ("bgemm_wgs", 8), ("bgemm_wgs", 0), ("bgemm_per", 2)):
            ts.set_option(name, value)
            P, G, C = ts.forward(B), ts.gradient(B), ts.quadcost(B, LAM)
            print("  bond %d %s = %d: P %.1e G %.1e cost %.1e against the unforced result" % (b, name, value, tr.relmax(P, P0), tr.relmax(G, G0), abs(C[0] / C0[0] - 1)))
            assert tr.relmax(P, P0) < 1e-13 and tr.relmax(G, G0) < 1e-13, (b, name, value)
            assert C[0] == pytest.approx(C0[0], rel=1e-13) and C[3] == C0[3], (b, name, value)
            assert tr.relmax(P, Po) < F["P"] and tr.relmax(G, Go) < F["G"] and C[0] == pytest.approx(Co, rel=F["C"]), (b, name, value)
            assert np.array_equal(P, ts.forward(B)) and np.array_equal(G, ts.gradient(B)), (b, name, value)
            if name != "bgemm_wgs" or value == 0:                       # bgemm_wgs = 8 stays on until it is set back to 0
                ts.set_option(name, 0)
        assert np.array_equal(P0, ts.forward(B)) and np.array_equal(G0, ts.gradient(B)), b        # every option is back at its default
    ts.close()


@pytest.mark.parametrize("forced", [False, True], ids=["default", "ten-label-kernels-requested"])
def test_launch_table_of_the_variant(forced):
    """One gradient and one forward evaluation on a 120 x 120 bond launch the feature GEMM, ONE label dot and the unfused gradient GEMM -- and
    none of the kernels that assume ten labels (k_grad_quad, k_fwd_res, k_fwd_fused, k_zprime), also when grad_quad = 2, fwd_res = 2 and
    fused_fwd = 2 ask for them: the variant must ignore those options.  The results are those of the oracle either way."""
    F = TOL["f64"]
    opts = (("grad_quad", 2), ("fwd_res", 2), ("fused_fwd", 2)) if forced else ()
    ts, o = _pair(uniform_dims(N_UNI, 120), 300, options=opts)
    classes = "bgemm,labeldot,fgemm_fwd,grad_quad,fwd_res,fwd_fused,zprime"
    at = 1
    for b in BONDS_UNI:
        _walk_to(ts, o, at, b)
        at = b
        B = _perturbed(o.bond_tensor(b), 0.05, b)
        ts.profile(True, only=classes)
        ts.profile_reset()
        P = ts.forward(B)
        lf = _launches(ts)
        ts.profile_reset()
        G = ts.gradient(B)
        lg = _launches(ts)
        ts.profile(False)
        assert lf == {"fgemm_fwd": 1, "labeldot": 1}, (b, lf)
        assert lg.pop("bgemm", 0) >= 1 and lg == {"fgemm_fwd": 1, "labeldot": 1}, (b, lg)      # (the gradient evaluates the outputs first)
        assert tr.relmax(P, o.forward(B)) < F["P"] and tr.relmax(G, o.gradient(B)) < F["G"], b
    ts.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. the noise split at shape
def _noise_splits(dims, NT, noise, ha, bonds=None):
    """test_single_noise_split_matches_the_oracle's recipe along the whole chain: B perturbed deterministically, split with keep =
    max(2, min(mL, mR)) and cutoff 1e-12, then both sides back to the original sites (a split to min(mL, mR) would otherwise shrink every link
    that follows, and the walk is about the prescribed dimensions).  `bonds`: where to split (default: everywhere)."""
    N = len(dims) - 1
    ts, o = _pair(dims, NT, maxm=max(dims))
    ts.set_option_real("noise", noise)
    W0 = o.get_mps()
    if ha == 2:
        for b in range(1, N):
            ts.shiftE(b, True); o.shiftE(b, True)
    for b in (range(1, N) if ha == 1 else range(N - 1, 0, -1)):
        if bonds is None or b in bonds:
            ts.setBond(b); o.set_bond(b)
            B0 = o.bond_tensor(b)
            B = B0 * (1.0 + 0.2 * np.cos(1.0 + np.arange(B0.size)).reshape(B0.shape))
            keep = max(2, min(B.shape[0], B.shape[3]))
            mg, teg, _ = ts.svd_split(B, b, ha, 1e-12, keep, 1)
            mo, teo = o.noise_split(B, b, ha, noise, 1e-12, keep, 1)
            Bg, Bo = ts.bond_tensor(b), o.bond_tensor(b)
            A = ts.get_site(b if ha == 1 else b + 1)
            G = np.einsum('asg,ash->gh', A, A) if ha == 1 else np.einsum('gtr,htr->gh', A, A)
            print("  noise %g half %d bond %2d (%3d x %3d): new m %d (oracle %d), truncation error %.3e (oracle %.3e), product of the sites %.1e, basis %.1e"
                  % (noise, ha, b, B.shape[0], B.shape[3], mg, mo, teg, teo, tr.relmax(Bg, Bo), np.abs(G - np.eye(G.shape[0])).max()))
            assert mg == mo, (ha, b)
            assert teg == pytest.approx(teo, rel=1e-5, abs=1e-13), (ha, b)
            assert tr.relmax(Bg, Bo) < 1e-7, (ha, b)
            assert np.abs(G - np.eye(G.shape[0])).max() < 1e-10, (ha, b)
            for j in (b, b + 1):                                 # lockstep, from the original sites: the walk keeps the prescribed dimensions
                ts.set_site(j, W0[j - 1]); o.set_site(j, W0[j - 1])
        ts.shiftE(b, ha == 1); o.shiftE(b, ha == 1)
    ts.close()


@pytest.mark.parametrize("ha", [1, 2])
@pytest.mark.parametrize("noise", [1e-6, 1e-3])
@pytest.mark.parametrize("dims,NT", [(SMALL_UNEQUAL, 37), (SMALL_UNEQUAL, 257), (CHAINS[1], 37), (CHAINS[1], 257)],
                         ids=["to-31-NT37", "to-31-NT257", "to-128-NT37", "to-128-NT257"])
def test_noise_split_with_unequal_left_and_right_dimensions(dims, NT, noise, ha):
    """rho + noise drho (single.h:648-672) where mL != mR at every interior bond -- the strides 2 mL / 4 mL of the weights kernel, the row
    index e + mE s against s + 2 e, the carve-up of the workspace by maxm -- in both half sweeps, chain ends included (no environment
    there: drho = NT rho): kept dimension, truncation error, the product of the two new sites, orthonormality of the basis."""
    _noise_splits(dims, NT, noise, ha)


@pytest.mark.parametrize("ha", [1, 2])
@pytest.mark.parametrize("noise", [1e-6, 1e-3])
def test_noise_split_on_the_uniform_m120_chain(noise, ha):
    """the same on the uniform chain, 300 images: rho is 240 x 240, the images' GEMMs run at their real size.  Splits at both chain ends, at
    the 2 x 120 and 120 x 2 bonds next to them, and at 120 x 120 bonds 3, 6 and 9 (the oracle's Jacobi sweeps over 240 x 240 take 0.4 s
    each); the bonds between are only shifted over."""
    _noise_splits(uniform_dims(N_UNI, 120), 300, noise, ha, bonds=(1, 2, 3, 6, 9, 10, 11))


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. bond updates in lockstep
def oracle_bond_update(o, b, ha, method, noise, maxm, minm, cutoff, npass, lam, cconv):
    """one bond update of single.h:523-728 from the oracle's entry points, as sorc_mldmrg strings them together"""
    o.set_bond(b)
    oB = o.bond_tensor(b)
    B, trc = (o.fast_cgrad if method == "fast_conj" else o.cgrad)(oB, npass, lam, cconv)
    rep = dict(norm_oB=float(np.sqrt(np.sum(oB * oB))), cost_old=o.quadcost(oB, lam)[0], cost_cg=o.quadcost(B, lam)[0], cg=trc)
    if noise:
        rep["newm"], rep["truncerr"] = o.noise_split(B, b, ha, noise, cutoff, maxm, minm)
    else:
        rep["newm"], rep["truncerr"], _ = o.svd_split(B, b, ha, cutoff, maxm, minm)
    rep["cost"] = o.quadcost(o.bond_tensor(b), lam)[0]
    o.shiftE(b, ha == 1)
    return rep


# The cutoffs: on the uniform chain every new dimension is set by the rank (2 mL) or by maxm = 48 at 1e-9, 1e-10 and 1e-11 alike.  On the third
# chain the spectrum of rho + noise drho falls smoothly: between 1e-4 and 1e-12 the cutoff itself picks 62 ... 97 states and a factor of 10
# moves that by up to 20, which no two fp64 codes need agree on; at 1e-14 (and at 1e-13, 1e-15) every split keeps maxm = 101 or its full rank.
LOCKSTEP = [pytest.param(uniform_dims(10, 64), 48, 24, "conj", 0.0, 1e-10, id="m64-conj"),
            pytest.param(uniform_dims(10, 64), 48, 24, "fast_conj", 1e-5, 1e-10, id="m64-fast_conj-noise"),
            pytest.param([1, 2, 4, 8, 16, 97, 120, 64, 33, 2, 1], 101, 60, "conj", 1e-6, 1e-14, id="to-120-conj-noise")]
CUTOFF_BIG = 1e-10


@pytest.mark.parametrize("dims,maxm,minm,method,noise,cutoff", LOCKSTEP)
def test_a_sweep_of_bond_updates_in_lockstep(dims, maxm, minm, method, noise, cutoff):
    """One full sweep through tnml_bond_update (report_costs) on 300 images, every update starting from the oracle's sites: the CG (conj or
    fast_conj), the split (SVD or density matrix with noise) truncating to maxm < m, the costs before the CG, after it and after the split,
    |B|, the truncation error and the CG trace against the oracle's cgrad / fast_cgrad + svd_split / noise_split + quadcost + shiftE."""
    from tnml_amd import lib
    N = len(dims) - 1
    ts, o = _pair(dims, 300, maxm=maxm)
    if method == "fast_conj":
        ts.set_option("cg_method", 1)
    if noise:
        ts.set_option_real("noise", noise)
    b, ha, n = 1, 1, 0
    while ha <= 2:
        r = ts.bond_update(b, ha, maxm, minm, cutoff, 3, LAM, CCONV, report_costs=True)
        q = oracle_bond_update(o, b, ha, method, noise, maxm, minm, cutoff, 3, LAM, CCONV)
        print("  half %d bond %2d (%3d x %3d): new m %d (oracle %d), cost %.1e, cost after the CG %.1e, truncation error %.3e (oracle %.3e)"
              % (ha, b, r["mL"], r["mR"], r["newm"], q["newm"], abs(r["cost"] / q["cost"] - 1), abs(r["cost_cg"] / q["cost_cg"] - 1), r["truncerr"], q["truncerr"]))
        assert r["newm"] == q["newm"], (b, ha)
        for k in ("cost_old", "cost_cg", "cost", "norm_oB"):
            assert r[k] == pytest.approx(q[k], rel=1e-8), (k, b, ha)
        assert r["truncerr"] == pytest.approx(q["truncerr"], rel=1e-3, abs=1e-12), (b, ha)
        assert r["cg"]["npass_done"] == q["cg"]["npass_done"] and r["cg"]["skipped"] == q["cg"]["skipped"], (b, ha)
        if method == "conj":
            np.testing.assert_allclose(r["cg"]["cost"], q["cg"]["cost"], rtol=1e-8, err_msg=str((b, ha)))
            np.testing.assert_allclose(r["cg"]["alpha"], q["cg"]["alpha"], rtol=TOL["f64"]["cga"], err_msg=str((b, ha)))
        else:
            np.testing.assert_allclose(r["cg"]["alpha"], q["cg"]["alpha"], rtol=1e-7, err_msg=str((b, ha)))
            np.testing.assert_allclose(r["cg"]["rnorm"], q["cg"]["rnorm"], rtol=1e-6, err_msg=str((b, ha)))
        ts.set_site(b, o.get_site(b)); ts.set_site(b + 1, o.get_site(b + 1))
        ts.shiftE(b, ha == 1)
        n += 1
        b, ha = lib.sweepnext(b, ha, N)
    assert n == 2 * (N - 1)
    ts.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
# 5. the unforced dispatch above the image-count thresholds
NT_BIG, K_BIG, NOISE_BIG = 30720, 256, 1e-8


def big_problem():
    """256 base images x 120 through tiled_problem's seeded permutation on the uniform m = 120 chain of 12 sites, its Label index dropped"""
    tp = tr.tiled_problem(N_UNI, K_BIG, NT_BIG, 120, 7, pixel_boost=200.0, dims=uniform_dims(N_UNI, 120))
    tp.W = tr.without_label(tp.W)
    return tp


def test_default_dispatch_at_30720_images_against_the_tiled_ground_truth():
    """30 720 images per rank with no option forced: above 24 576 padded images the label dot takes its streaming form <4, 2, NLT = 1> and the
    slab cut of the gradient GEMM is that of a real shard.  Against the oracle on the 256 base images through the per-label identities of
    tiled_reference.py (R = 120): forward, gradient (repeated: the same bits), cost and #correct at a bond on either side of the middle, three
    CG passes at lambda / R, cconv / R, the split with noise in both half sweeps and one bond update with noise (the base split at noise R).  The streaming form is recognised by its
    bits: outputs and cost are those of ldot_cfg = 1 (128-image blocks) and not those of ldot_cfg = 2 (64-image blocks, sixteen waves)."""
    from oracle import pyoracle
    from tnml_amd.fixedl import TrainStates
    F = TOL["f64"]
    tp = big_problem()
    R = tp.R
    assert R == NT_BIG // K_BIG == 120
    ts = TrainStates(tp.labels, N_UNI, 120, phi=tp.phi, single_label=TARGET)                # NO kernel-selection option
    ts.set_mps(tp.W)
    ts.init()
    ob = pyoracle.SingleOracle(tp.phi0, tp.labels0, TARGET, tp.W, nthread=_NTH)
    ob.init()
    at = 1
    for b in BONDS_UNI:
        _walk_to(ts, ob, at, b)
        at = b
        B = _perturbed(ob.bond_tensor(b), 0.05, b)
        want = tr.single_tiled(tp, TARGET, ob.forward(B), ob.gradient(B), ob.quadcost(B, LAM / R)[0])
        ts.profile(True, only="bgemm,labeldot,fgemm_fwd,grad_quad,fwd_res,fwd_fused,zprime")
        ts.profile_reset()
        P = ts.forward(B)
        lf = _launches(ts)
        ts.profile_reset()
        G = ts.gradient(B)
        lg = _launches(ts)
        ts.profile(False)
        C = ts.quadcost(B, LAM)
        print("  bond %d: P %.1e G %.1e cost %.1e | forward %s | gradient %s" % (b, tr.relmax(P, want["P"]), tr.relmax(G, want["G"]), abs(C[0] / want["cost"] - 1), lf, lg))
        assert lf == {"fgemm_fwd": 1, "labeldot": 1} and lg.pop("bgemm", 0) >= 1 and lg == {"fgemm_fwd": 1, "labeldot": 1}, (b, lf, lg)
        assert tr.relmax(P, want["P"]) < F["P"], b
        assert tr.relmax(G, want["G"]) < F["G"], b
        assert C[0] == pytest.approx(want["cost"], rel=F["C"]) and C[3] == want["ncorrect"], b
        assert np.array_equal(G, ts.gradient(B)), b
        ts.set_option("ldot_cfg", 1)
        P1, C1 = ts.forward(B), ts.quadcost(B, LAM)
        ts.set_option("ldot_cfg", 2)
        P2, C2 = ts.forward(B), ts.quadcost(B, LAM)
        ts.set_option("ldot_cfg", 0)
        assert np.array_equal(P, P1) and C[0] == C1[0], b                       # the unforced label dot IS the streaming form
        assert not (np.array_equal(P, P2) and C[0] == C2[0]), b                 # ... whose sums differ in order from the small-shard form's
        assert tr.relmax(P2, want["P"]) < F["P"] and C2[0] == pytest.approx(want["cost"], rel=F["C"]) and C2[3] == want["ncorrect"], b
        Bg, tg = ts.cgrad(B, 3, LAM, CCONV)
        Bo, to = ob.cgrad(B, 3, LAM / R, CCONV / R)
        sc = tr.scaled_trace(to, R)
        np.testing.assert_allclose(tg["cost"], sc["cost"], rtol=F["cgc"], err_msg=str(b))
        np.testing.assert_allclose(tg["alpha"], sc["alpha"], rtol=F["cga"], err_msg=str(b))
        assert tr.relmax(Bg, Bo) < F["cga"], b
    b = BONDS_UNI[1]
    ts.set_option_real("noise", NOISE_BIG)
    # the split with noise in both half sweeps: 120 x 30 720 entries of the weighted environment are seven times what a capped grid of
    # 2048 x 256 threads covers in one pass
    B0 = ob.bond_tensor(b)
    B = B0 * (1.0 + 0.2 * np.cos(1.0 + np.arange(B0.size)).reshape(B0.shape))
    sites = [ob.get_site(b), ob.get_site(b + 1)]
    for ha in (1, 2):
        mg, teg, _ = ts.svd_split(B, b, ha, 1e-12, 120, 1)
        mo, teo = ob.noise_split(B, b, ha, NOISE_BIG * R, 1e-12, 120, 1)
        print("  noise split half %d: new m %d (oracle %d), truncation error %.3e (oracle %.3e), product of the sites %.1e" % (ha, mg, mo, teg, teo, tr.relmax(ts.bond_tensor(b), ob.bond_tensor(b))))
        assert mg == mo == 120, ha
        assert teg == pytest.approx(teo, rel=1e-5, abs=1e-13), ha
        assert tr.relmax(ts.bond_tensor(b), ob.bond_tensor(b)) < 1e-7, ha
        for j in (0, 1):
            ts.set_site(b + j, sites[j]); ob.set_site(b + j, sites[j])
    r = ts.bond_update(b, 1, 100, 60, CUTOFF_BIG, 3, LAM, CCONV, report_costs=True)
    q = oracle_bond_update(ob, b, 1, "conj", NOISE_BIG * R, 100, 60, CUTOFF_BIG, 3, LAM / R, CCONV / R)
    print("  bond update %d: new m %d (oracle %d), cost %.1e, truncation error %.3e (oracle %.3e)" % (b, r["newm"], q["newm"], abs(r["cost"] / (R * q["cost"]) - 1), r["truncerr"], q["truncerr"]))
    assert r["newm"] == q["newm"]
    for k in ("cost_old", "cost_cg", "cost"):
        assert r[k] == pytest.approx(R * q[k], rel=1e-8), k
    assert r["truncerr"] == pytest.approx(q["truncerr"], rel=1e-3, abs=1e-12)
    np.testing.assert_allclose(r["cg"]["cost"], [R * x for x in q["cg"]["cost"]], rtol=1e-8)
    ts.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
# 6. two ranks
RANKS_CASE = dict(dims=uniform_dims(10, 64), NT=301, noise=1e-5, sweep=(1, 48, 24, 1e-10, 3, LAM, CCONV))


def test_two_ranks_at_m64_with_noise():
    """test_per_label_variant_on_two_ranks_with_and_without_noise at m = 64: 301 images split 150 / 151, noise 1e-5, one sweep truncating to
    48.  noise_add's all-reduce of the three weighted Gram matrices of the environment carries 3 * 64^2 doubles here (75 in that test).  Both
    ranks report the one-rank values, which are the oracle's, and keep bit-identical replicas."""
    from oracle import pyoracle
    from tnml_amd import lib
    from tnml_amd.fixedl import TrainStates, mldmrg
    dims, NT, noise, sweep = (RANKS_CASE[k] for k in ("dims", "NT", "noise", "sweep"))
    N = len(dims) - 1
    labels, phi, W = single_problem(dims, NT)
    o = pyoracle.SingleOracle(phi, labels, TARGET, W, nthread=_NTH)
    o.set_noise(noise)
    o.init()
    ro = o.mldmrg(*sweep)

    def run(nranks):
        states = []
        for r in range(nranks):
            lo, hi = lib.shard_bounds(NT, nranks, r)
            states.append(TrainStates(labels[lo:hi], N, max(dims), phi=phi[lo:hi], rank=r, nranks=nranks, NT_total=NT, single_label=TARGET))
        if nranks > 1:
            assert len({s.NT for s in states}) == nranks                       # an uneven split
            TrainStates.comm_init_local(states)
        out, err = [None] * nranks, [None] * nranks

        def work(r):
            try:
                ts = states[r]
                ts.set_mps(W)
                ts.set_option_real("noise", noise)
                ts.init()
                reps = mldmrg(ts, *sweep)
                ts.replica_check()
                out[r] = (reps, [ts.get_site(j) for j in range(1, N + 1)])
            except Exception as e:                               # noqa: BLE001
                err[r] = e
        th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=600)
        assert not any(t.is_alive() for t in th), "a rank hung"
        for e in err:
            if e is not None:
                raise e
        for ts in states:
            ts.close()
        return out
    one, two = run(1), run(2)
    assert len(two[0][0]) == len(one[0][0]) == len(ro) == 2 * (N - 1)
    for a, a1, b, c in zip(two[0][0], two[1][0], one[0][0], ro):
        assert a["newm"] == a1["newm"] == b["newm"] == c["newm"], (a["c"], a["half"])
        assert a["cost"] == a1["cost"]
        assert a["cost"] == pytest.approx(b["cost"], rel=1e-9) and a["cost"] == pytest.approx(c["cost"], rel=1e-7), (a["c"], a["half"])
        assert a["cost_cg"] == pytest.approx(b["cost_cg"], rel=1e-9) and a["cost_cg"] == pytest.approx(c["cost_cg"], rel=1e-7), (a["c"], a["half"])
        assert a["truncerr"] == pytest.approx(c["truncerr"], rel=1e-3, abs=1e-12), (a["c"], a["half"])
    for A0, A1 in zip(two[0][1], two[1][1]):
        assert np.array_equal(A0, A1)                              # replicas bit-identical
