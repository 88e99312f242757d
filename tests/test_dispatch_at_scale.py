"""The DEFAULT kernel dispatch at the image counts where it changes, against ground truth -- and the selectable paths no parity test reached.

Every kernel a real run executes is chosen by the padded image count per rank (k_fwd_res / k_shift_res from 7 680, k_grad_quad from 4 096 and
its pair form from 15 360, k_fwd_fused from 14 336, the k_fgemm64 tile families and the streaming label dot from 192 tiles of 64 / 128 images,
the slab count of the gradient GEMM), while the oracle handles a few thousand images at m = 120.  The tests of test_configs_at_shape.py
therefore FORCE those kernels at oracle-sized counts; here no kernel-selection option is set and the image count is real.

Ground truth at scale comes from tiled_reference.py: the large set repeats a base set of a few hundred images through a seeded permutation,
so outputs, environments, gradient, costs, the CG and the bond update of the large set follow from the base set (count-weighted sums; for a
uniform repeat count R the base problem at lambda/R, cconv/R).  test_tiled_identity_with_the_oracle_on_both_sides proves that identity on
the CPU with the C oracle on both sides -- the GPU tests below then measure the kernels, not the harness.  The tolerances are the fp64
figures of test_gpu_parity.py (TOL) and of the forced-kernel tests; the reference's own scatter under the identity is four orders below them.

f32, bf16 and bf16x3 are covered PER KERNEL up to 25 000 images, not here: tests/rp_model.py models their rounding and test_rp_model_gpu.py
holds every kernel of theirs inside its derived bound -- at up to 700 images every tile class, and at 24 320 / 24 576 / 25 000 images the
default dispatch of the label dot on either side of its threshold (the streaming form k_labeldot<8, 2, NLT, float, float, float> included),
cost / per-label costs / #correct / pAp as exact functions of the device's own outputs, and the gradient GEMM at its real slab cuts (12 slabs
of 2 048 images, a short last slab, 79 slabs) on sparse probes and on dense data.  The CG is closed pass by pass: test_cg_model_gpu.py
holds every pass of it, from the device's own state before the pass, to the bounds of those kernels and its fast output update P = fma(alpha, Pp, P)
bit for bit -- every path at 300 images (fp64 included, at 1e-13 where the parity tolerance is 1e-5) and the default dispatch at 24 320 / 24 576
images on sparse probes (tests/cg_model.py).  Still open in these modes at scale: whole bond updates (the split and the shift after the CG), and
image counts above 25 000 (the slab grows to 5 024 images at 60 000).  Only
f64_e32 (fp32 storage, fp64 accumulation: its rounding does not depend on the image count) gets a case at scale in this file."""
import os

import numpy as np
import pytest

import tiled_reference as tr
from test_gpu_parity import TOL

F64 = TOL["f64"]
LAM, CCONV, NPASS = 1e-3, 1e-10, 3
_NTH = min(8, os.cpu_count() or 1)


def _oracle(phi, labels, W):
    from oracle import pyoracle
    o = pyoracle.Oracle(phi, labels, W, nthread=_NTH)
    o.init()
    return o


def _perturbed(B, scale, seed):
    return B + scale * np.random.default_rng(seed).standard_normal(B.shape)


# ------------------------------------------------------------------------------------------------------------------------------------------
# A. the identity itself, oracle on both sides (no GPU)
@pytest.mark.parametrize("NT", [420, 437], ids=["uniform-R7", "ragged"])
def test_tiled_identity_with_the_oracle_on_both_sides(NT):
    """The C oracle on the MATERIALISED tiled set (420 = 7 x 60 images, and 437: ragged counts of 7 and 8) against the weighted base references
    of tiled_reference.py (extended precision, from the numpy restatement's environments of the 60 base images): environments, P, gradient,
    cost, per-label costs, #correct and pAp at bonds 1 / 3 (Label on the right environment), 5 / 6 (on B) and 9 (on the left environment);
    with uniform counts also the CG at lambda/R, cconv/R (four passes) and one split after it.  Where np.longdouble is not an extended type
    the references are evaluated in fp64 instead of skipping: they stay an independent evaluation (numpy restatement, factorised t.v, weighted
    base set) and the fp64 tolerances hold for two fp64 codes."""
    N, K, m = 12, 60, 6
    tp = tr.tiled_problem(N, K, NT, m, 3)
    assert tp.counts.sum() == NT and (tp.R == 7 if NT == 420 else tp.R is None and set(tp.counts) == {7, 8})
    assert not np.array_equal(tp.idx, np.arange(NT) % K)                      # permuted: copies do not sit at a fixed stride
    big = _oracle(tp.phi, tp.labels, tp.W)
    base = _oracle(tp.phi0, tp.labels0, tp.W)
    n = tr.extended_environments(tp, 1)
    for j in range(3, N + 1):
        assert tr.relmax(big.env(j), np.asarray(n.E[j], dtype=np.float64)[tp.idx]) < F64["E"], j
    at = 1
    for b in (1, 3, 5, 6, 9):
        for bb in range(at, b):
            big.shiftE(bb, True); base.shiftE(bb, True); n.shiftE(bb, True)
            if bb >= 3:
                assert tr.relmax(big.env(bb), np.asarray(n.E[bb], dtype=np.float64)[tp.idx]) < F64["E"], bb
        at = b
        big.set_bond(b); base.set_bond(b)
        ref = tr.BondReference.at_bond(n, b, tp.labels0)
        assert ref.kind == {1: "RE", 3: "RE", 5: "B", 6: "B", 9: "LE"}[b]
        B = _perturbed(big.bond_tensor(b), 0.1, b)
        ev = ref.evaluate(B)
        w = ref.weighted(ev, tp.counts, B, LAM)
        assert tr.relmax(big.forward(B), ev["P"][tp.idx]) < F64["P"], b
        assert tr.relmax(big.gradient(B), w["G"]) < F64["G"], b
        C, lc, cr, nc = big.quadcost(B, LAM)
        assert C == pytest.approx(w["cost"], rel=F64["C"]) and nc == w["ncorrect"], b
        np.testing.assert_allclose(lc, w["label_cost"], rtol=5 * F64["C"], atol=0.05 * F64["C"] * C)
        assert cr == pytest.approx(w["reg_cost"], rel=1e-12)
        p = np.random.default_rng(100 + b).standard_normal(B.shape)
        assert float(np.sum(big.forward(p) ** 2) + LAM * np.sum(p ** 2)) == pytest.approx(ref.pAp(p, LAM, tp.counts), rel=F64["C"]), b
        if tp.R is None:
            continue
        R = tp.R
        B0 = big.bond_tensor(b)
        Bb, tb = big.cgrad(B0, 4, LAM, CCONV)
        Bs, ts_ = base.cgrad(B0, 4, LAM / R, CCONV / R)
        sc = tr.scaled_trace(ts_, R)
        assert tb["npass_done"] == ts_["npass_done"] == 4
        np.testing.assert_allclose(tb["cost"], sc["cost"], rtol=F64["cgc"], err_msg=str(b))
        for k in ("alpha", "rnorm", "pAp"):
            np.testing.assert_allclose(tb[k], sc[k], rtol=F64["cga"], err_msg="%s bond %d" % (k, b))
        assert tr.relmax(Bb, Bs) < F64["cga"], b
    if tp.R is not None:                                                    # one split after the CG of bond 9, the same on both sides
        mb, teb, svb = big.svd_split(Bb, 9, 1, 1e-4, 5, 2)
        ms, tes, svs = base.svd_split(Bs, 9, 1, 1e-4, 5, 2)
        assert mb == ms and teb == pytest.approx(tes, rel=1e-6, abs=1e-18)
        np.testing.assert_allclose(svb, svs, rtol=1e-8, atol=1e-10 * svs[0])
        Cb = big.quadcost(big.bond_tensor(9), LAM)
        Cs = base.quadcost(base.bond_tensor(9), LAM / tp.R)
        assert Cb[0] == pytest.approx(tp.R * Cs[0], rel=1e-8) and Cb[3] == tp.R * Cs[3]


# ------------------------------------------------------------------------------------------------------------------------------------------
# B / E. the default dispatch at real image counts
N_CHAIN, BOOST = 20, 200.0
BONDS = ((7, "Label on RE, 64 x m"), (8, "Label on RE"), (9, "Label on B"), (12, "Label on LE"), (13, "Label on LE, m x 64"))
ENV_SITES_RIGHT, ENV_SITES_LEFT = (7, 9), (11, 12)          # Label-carrying environments fetched whole: two per direction (NT x 1200 doubles each)
STRETCH = (8, 9, 10, 11, 12)                                 # bond updates in lockstep: Label on RE, on B twice, on LE twice
NT_M120 = [3840, 4096, 7424, 7680, 7681, 12032, 12288, 14080, 14336, 15104, 15360, 24320, 24576, 60000]
NT_M48 = [15104, 15360, 24320, 24576]
_BASE = {}          # (N, K, m, seed, dims) -> the base set's references: a memo only (they do not depend on the image count, and cost ~8 s at m = 120)


def _base_size(NT):
    return 256 if NT % 256 == 0 else 300


def _base_references(N, K, m, seed, bonds, dims=None, env_left=(), env_right=()):
    key = (N, K, m, seed, tuple(dims) if dims else None)
    if key not in _BASE:
        tp = tr.tiled_problem(N, K, K, m, seed, pixel_boost=BOOST, dims=dims)
        n = tr.extended_environments(tp, 1)
        out = dict(bonds={}, env={})
        for j in env_right:
            out["env"][("R", j)] = np.asarray(n.E[j], dtype=np.float64)
        at = 1
        for b in bonds:
            for bb in range(at, b):
                n.shiftE(bb, True)
                if bb in env_left:
                    out["env"][("L", bb)] = np.asarray(n.E[bb], dtype=np.float64)
            at = b
            ref = tr.BondReference.at_bond(n, b, tp.labels0)
            B0 = np.asarray(n.bond_tensor(b), dtype=np.float64)
            B = _perturbed(B0, 0.05 * np.abs(B0).max(), b)
            p = np.random.default_rng(100 + b).standard_normal(B.shape)
            out["bonds"][b] = dict(ref=ref, B=B, ev=ref.evaluate(B), p=p)
        _BASE[key] = out
    return _BASE[key]


def _launches(ts):
    return {k: v[0] for k, v in ts.profile_read().items() if v[0]}


def _env_deviation(Eg, Eb, idx, chunk=8192):
    """max |Eg[n] - Eb[idx[n]]| / max |Eb|, in slices of images (an environment of 60 000 images is 576 MB)"""
    worst, scale = 0.0, float(np.abs(Eb).max())
    for s in range(0, len(idx), chunk):
        worst = max(worst, float(np.abs(Eg[s:s + chunk] - Eb[idx[s:s + chunk]]).max()))
    return worst / scale


def _single_evaluations(ts, tp, base, bonds, tol, table, worst, shifted=None):
    """walk ts left to right over `bonds`; at each: forward, gradient (twice: the same bits), quadcost and pAp against the weighted references"""
    at = 1
    for b, kind in bonds:
        for bb in range(at, b):
            ts.profile_reset()
            ts.shiftE(bb, True)
            if shifted is not None:
                shifted(bb, _launches(ts))
        at = b
        ts.setBond(b)
        d = base["bonds"][b]
        ref, B, ev = d["ref"], d["B"], d["ev"]
        assert ts.bond_shape(b) == B.shape, (b, ts.bond_shape(b), B.shape)
        w = ref.weighted(ev, tp.counts, B, LAM)
        ts.profile_reset()
        P = ts.forward(B)
        lf = _launches(ts)
        ts.profile_reset()
        G = ts.gradient(B)
        lg = _launches(ts)
        table[b] = dict(kind=kind, forward=lf, gradient=lg)
        eP = tr.relmax(P, np.asarray(ev["P"], dtype=np.float64)[tp.idx])
        eG = tr.relmax(G, w["G"])
        Cg, lcg, crg, ncg = ts.quadcost(B, LAM)
        eC = abs(Cg / w["cost"] - 1.0)
        pg = ts.pAp(d["p"], LAM)
        eA = abs(pg / ref.pAp(d["p"], LAM, tp.counts) - 1.0)
        print("  NT %6d bond %2d (%-19s) rel. dev. P %.1e G %.1e cost %.1e pAp %.1e | forward %s | gradient %s" % (tp.NT, b, kind, eP, eG, eC, eA, lf, lg))
        for k, v in (("P", eP), ("G", eG), ("cost", eC)):
            worst[k] = max(worst.get(k, 0.0), v)
        assert eP < tol["P"], (b, kind)
        assert eG < tol["G"], (b, kind)
        assert eC < tol["C"] and eA < tol["C"], (b, kind)
        np.testing.assert_allclose(lcg, w["label_cost"], rtol=5 * tol["C"], atol=0.05 * tol["C"] * w["cost"])
        assert crg == pytest.approx(w["reg_cost"], rel=1e-12)
        if tol is F64:
            assert ncg == w["ncorrect"], (b, kind)
        else:
            # fp32-stored environments may move an image across the decision boundary, but only one whose two largest |P_l| lie within the
            # storage tolerance of each other (each may move by tol P of max |P|): the count is the one of the kernel's own outputs, and every
            # image it decides differently from the reference is a copy of such a base image
            Px = np.abs(np.asarray(ev["P"], dtype=np.float64))
            top = np.sort(Px, axis=1)
            near = (top[:, -1] - top[:, -2]) < 2 * tol["P"] * Px.max()
            hit = np.argmax(np.abs(P), axis=1) == tp.labels
            assert ncg == int(hit.sum()), (b, kind)
            differs = hit != ev["hit"][tp.idx]
            assert near[tp.idx[differs]].all(), (b, kind, int(differs.sum()))
        assert np.array_equal(G, ts.gradient(B)), (b, kind)                     # fixed summation order: the same bits every time


def _default_dispatch(m, NT, dtype="f64", with_cg=True):
    from tnml_amd.fixedl import TrainStates
    tol = TOL[dtype]
    K = _base_size(NT)
    tp = tr.tiled_problem(N_CHAIN, K, NT, m, 7, pixel_boost=BOOST)
    base = _base_references(N_CHAIN, K, m, 7, [b for b, _ in BONDS], env_left=ENV_SITES_LEFT, env_right=ENV_SITES_RIGHT)
    ts = TrainStates(tp.labels, N_CHAIN, m, phi=tp.phi, dtype=dtype)            # NO kernel-selection option
    ts.set_mps(tp.W)
    ts.profile(True)
    ts.profile_reset()
    ts.init()
    table, worst = {"init": _launches(ts)}, {}
    for j in ENV_SITES_RIGHT:                                                   # built by init
        assert _env_deviation(ts.env(j), base["env"][("R", j)], tp.idx) < tol["E"], j
    shifts = {}

    def shifted(bb, launches):
        shifts[bb] = launches
        if bb in ENV_SITES_LEFT:                                                # built by shiftE
            assert _env_deviation(ts.env(bb), base["env"][("L", bb)], tp.idx) < tol["E"], bb
    _single_evaluations(ts, tp, base, BONDS, tol, table, worst, shifted)
    table["shift"] = shifts
    if with_cg and tp.R is not None:
        R = tp.R
        ob = _oracle(tp.phi0, tp.labels0, tp.W)
        # the CG on the large set against the base set's at lambda / R, cconv / R
        ts.init()
        at = 1
        for b, kind in BONDS:
            for bb in range(at, b):
                ts.shiftE(bb, True); ob.shiftE(bb, True)
            at = b
            ts.setBond(b); ob.set_bond(b)
            B = base["bonds"][b]["B"]
            Bg, tg = ts.cgrad(B, NPASS, LAM, CCONV)
            Bo, to = ob.cgrad(B, NPASS, LAM / R, CCONV / R)
            sc = tr.scaled_trace(to, R)
            np.testing.assert_allclose(tg["cost"], sc["cost"], rtol=tol["cgc"], err_msg=kind)
            np.testing.assert_allclose(tg["alpha"], sc["alpha"], rtol=tol["cga"], err_msg=kind)
            assert tr.relmax(Bg, Bo) < tol["cga"], kind
        # bond updates in lockstep: every one starts from the oracle's sites
        ts.init(); ob.init()
        for bb in range(1, STRETCH[0]):
            ts.shiftE(bb, True); ob.shiftE(bb, True)
        cutoff, maxm, minm = 3e-4, m - m // 6, m // 2          # the split truncates: the bonds that follow have unequal dimensions (100 x 120, ...)
        for b in STRETCH:
            r = ts.bond_update(b, 1, maxm, minm, cutoff, NPASS, LAM, CCONV)
            ob.set_bond(b)
            Bo, to = ob.cgrad(ob.bond_tensor(b), NPASS, LAM / R, CCONV / R)
            newm, te, _ = ob.svd_split(Bo, b, 1, cutoff, maxm, minm)
            C, lc, cr, nc = ob.quadcost(ob.bond_tensor(b), LAM / R)
            ob.shiftE(b, True)
            print("  NT %6d bond update %2d: %d x %d -> new m %d (oracle %d), rel. dev. of the cost %.1e" % (NT, b, r["mL"], r["mR"], r["newm"], newm, abs(r["cost"] / (R * C) - 1)))
            assert r["newm"] == newm, (b, r["newm"], newm)
            assert r["cost"] == pytest.approx(R * C, rel=1e-8), b
            assert r["ncorrect"] == R * nc, b
            np.testing.assert_allclose(r["cg"]["cost"], [R * x for x in to["cost"]], rtol=1e-8, err_msg="bond %d" % b)
            ts.set_site(b, ob.get_site(b))
            ts.set_site(b + 1, ob.get_site(b + 1))
            ts.shiftE(b, True)
    ts.profile(False)
    ts.close()
    print("  NT %6d m %d %s: largest rel. dev. P %.1e G %.1e cost %.1e" % (NT, m, dtype, worst["P"], worst["G"], worst["cost"]))
    return table


@pytest.mark.gpu
@pytest.mark.parametrize("NT", NT_M120)
def test_default_dispatch_at_m120_against_the_tiled_ground_truth(NT):
    """The N = 20, m = 120, pixel_boost = 200 chain of test_configs_at_shape.py at real image counts, either side of every dispatch threshold
    (stated in padded images: 4 096, 7 680, 12 288, 14 336, 15 360, 24 576), one ragged count whose PADDED count is past a threshold (7 681)
    and 60 000; no kernel-selection option.  Bonds 7 / 8 (Label on the right environment; 64 x 120 and 120 x 120), 9 (on B), 12 / 13 (on the
    left environment): forward, gradient (repeats bit for bit), cost / label costs / #correct and pAp against the count-weighted references
    of the base set; Label-carrying environments of init and shiftE against the tiled base environments.  Where the base size divides the
    count: the CG (three passes) at every one of those bonds and five bond updates in lockstep (Label on RE, on B, on LE) against the oracle
    on the base set at lambda / R.  At 60 000 images the kernel classes are asserted; elsewhere they are printed and compared across the
    thresholds by test_launches_change_across_the_dispatch_thresholds."""
    table = _default_dispatch(120, NT)
    if NT == 60000:
        assert table["init"].get("fgemm_shift", 0) > 0
        for b, kind in BONDS:
            if kind == "Label on B":
                continue
            f, g = table[b]["forward"], table[b]["gradient"]
            assert f.get("fwd_res", 0) == 1 and not f.get("fgemm_fwd") and not f.get("labeldot"), (kind, f)
            assert g.get("grad_quad", 0) == 1 and g.get("fwd_res", 0) >= 1 and not g.get("bgemm") and not g.get("fgemm_fwd"), (kind, g)
        assert all(v.get("fgemm_shift", 0) > 0 for v in table["shift"].values()), table["shift"]


@pytest.mark.gpu
@pytest.mark.parametrize("NT", NT_M48)
def test_default_dispatch_at_m48_against_the_tiled_ground_truth(NT):
    """the same chain at m = 48, either side of the two thresholds that apply to bonds up to 64 only: the pair form of k_grad_quad (15 360)
    and the 128 x 128 feature-GEMM tiles (128 * 192 = 24 576)"""
    _default_dispatch(48, NT)


@pytest.mark.gpu
def test_reduced_storage_at_60000_images():
    """dtype f64_e32 (fp32-stored environments, fp64 accumulation) at 60 000 images with no forced option: single evaluations as above at
    TOL["f64_e32"] -- the storage rounding does not depend on the image count."""
    _default_dispatch(120, 60000, dtype="f64_e32", with_cg=False)


def _launch_table(m, NT):
    """the kernel classes one forward / one gradient evaluation launches at bonds 8 and 12 (Label on the right / left environment)"""
    from tnml_amd.fixedl import TrainStates
    tp = tr.tiled_problem(N_CHAIN, _base_size(NT), NT, m, 7, pixel_boost=BOOST)
    ts = TrainStates(tp.labels, N_CHAIN, m, phi=tp.phi)
    ts.set_mps(tp.W)
    ts.profile(True)
    ts.init()
    table, at = {}, 1
    for b in (8, 12):
        for bb in range(at, b):
            ts.shiftE(bb, True)
        at = b
        ts.setBond(b)
        B = ts.bond_tensor(b)
        ts.profile_reset(); ts.forward(B); lf = _launches(ts)
        ts.profile_reset(); ts.gradient(B); lg = _launches(ts)
        table[b] = dict(forward=lf, gradient=lg)
    ts.close()
    return table


@pytest.mark.gpu
def test_launches_change_across_the_dispatch_thresholds():
    """Not a second copy of the dispatch table: only THAT the launched kernel classes differ between the two sides of a threshold where the
    threshold moves work to another class -- k_grad_quad (4 096; pair form 15 360 at m = 48) and k_fwd_res (7 680) -- measured here at those
    seven counts.  The thresholds at 12 288 and 24 576 choose another tile instantiation or label-dot form of the SAME class (fgemm_fwd,
    labeldot: one launch either way): launch counts cannot see them, the parity checks on either side are what covers them.  The
    k_fwd_fused threshold (14 336) is NOT exercised by the 14 080 / 14 336 pair: k_fwd_res takes the forward pass on both sides; the default
    dispatch reaches k_fwd_fused only above the 32-bit guard of k_fwd_res (asserted by the 460 800-image case below)."""
    t = {(m, NT): _launch_table(m, NT) for m, NT in ((120, 3840), (120, 4096), (120, 7424), (120, 7680), (120, 7681), (48, 15104), (48, 15360))}
    for b in (8, 12):
        g_lo, g_hi = t[120, 3840][b]["gradient"], t[120, 4096][b]["gradient"]
        f_lo, f_hi = t[120, 7424][b]["forward"], t[120, 7680][b]["forward"]
        p_lo, p_hi = t[48, 15104][b]["gradient"], t[48, 15360][b]["gradient"]
        assert g_lo.get("grad_quad", 0) != g_hi.get("grad_quad", 0) and g_lo.get("bgemm", 0) != g_hi.get("bgemm", 0), (b, g_lo, g_hi)
        assert f_lo.get("fwd_res", 0) != f_hi.get("fwd_res", 0) and f_lo.get("fgemm_fwd", 0) != f_hi.get("fgemm_fwd", 0), (b, f_lo, f_hi)
        assert p_lo.get("grad_quad", 0) != p_hi.get("grad_quad", 0), (b, p_lo, p_hi)
        assert t[120, 7681][b]["forward"] == f_hi                              # the decision is made on the PADDED count (7 681 -> 7 936)


# ------------------------------------------------------------------------------------------------------------------------------------------
# C. large shards: both sides of the 32-bit lane-offset guards
# the shortest chain with a 120 x 120 bond on either side of the Label site (N / 2 = 5): bond 3 (sites 3, 4; Label on the right environment),
# bond 6 (sites 6, 7; on the left environment); bond 4 carries the Label index itself (8 x 120).  The inner links are 8 wide to keep the footprint down.
# The 120-link environments of bonds 3 and 6 come from the shift of the Label SITE (generic kernel).  The shifts that READ them -- 120 -> 8 links,
# k_shift_res below its guard, k_fgemm64 above -- build the right environment of bond 2 (by init) and the left one of bond 7 (by shiftE): those
# two small bonds (2 x 2 x 2 x 8, 8 x 2 x 2 x 4) are what checks the output of a Label-carrying shift over a > 2 GiB / > 4 GiB source.
DIMS_SHARD = [1, 2, 120, 8, 120, 120, 8, 120, 4, 2, 1]
BONDS_SHARD = ((2, "Label on RE, shifted"), (3, "Label on RE"), (4, "Label on B"), (6, "Label on LE"), (7, "Label on LE, shifted"))


@pytest.mark.gpu
@pytest.mark.parametrize("NT,resident", [(230400, True), (460800, False)])
def test_large_shards_on_both_sides_of_the_32_bit_offset_guards(NT, resident):
    """A Label-carrying environment of 120 links is 10 * 120 * NTp * 8 bytes: 2.2 GB at 230 400 images -- byte offsets past 2^31, the resident
    kernels (k_fwd_res, k_shift_res, k_grad_quad) still apply -- and 4.4 GB at 460 800, above their guard (2^32): the kernels with 64-bit
    offsets (k_fwd_fused -- the one place the default dispatch reaches it, asserted --, k_fgemm64, k_bgemm64) must take over without an error.
    forward (all images), gradient, cost, label costs, #correct and pAp against the weighted references of 256 base images at bonds 3 / 6
    (120 x 120), 4 (Label on B) and 2 / 7, whose Label-carrying environments are the outputs of the shifts over the large environments; no
    environment is fetched."""
    import torch
    from tnml_amd.fixedl import TrainStates
    N, m, K = len(DIMS_SHARD) - 1, 120, 256
    tp = tr.tiled_problem(N, K, NT, m, 17, pixel_boost=BOOST, dims=DIMS_SHARD)
    base = _base_references(N, K, m, 17, [b for b, _ in BONDS_SHARD], dims=DIMS_SHARD)
    ts = TrainStates(tp.labels, N, m, phi=tp.phi)
    need, free = ts.estimate_bytes(), torch.cuda.mem_get_info(0)[0]
    if need > free:
        ts.close()
        pytest.skip("the device has %.1f GB free, tnml_estimate_bytes asks for %.1f GB (an MI355X runs this case)" % (free / 1e9, need / 1e9))
    ts.set_mps(tp.W)
    ts.profile(True)
    ts.profile_reset()
    ts.init()
    table, worst, shifts = {"init": _launches(ts)}, {}, {}
    _single_evaluations(ts, tp, base, BONDS_SHARD, F64, table, worst, shifts.__setitem__)
    assert table["init"].get("fgemm_shift", 0) > 0 and shifts[6].get("fgemm_shift", 0) == 1, (table["init"], shifts)
    print("  NT %d: %.1f GB on the device; init %s; largest rel. dev. P %.1e G %.1e cost %.1e" % (NT, ts.device_bytes() / 1e9, table["init"], worst["P"], worst["G"], worst["cost"]))
    for b in (3, 6):
        f, g = table[b]["forward"], table[b]["gradient"]
        if resident:
            assert f.get("fwd_res", 0) == 1 and not f.get("fgemm_fwd"), (b, f)
        else:
            assert not f.get("fwd_res") and not f.get("fgemm_fwd") and f.get("fwd_fused", 0) == 1, (b, f)      # (k_fwd_fused: 64-bit offsets, from 14 336 images on)
            assert not g.get("fwd_res") and not g.get("grad_quad") and g.get("bgemm", 0) >= 1, (b, g)
    assert ts.env_stats()["fetches"] == 0
    ts.profile(False)
    ts.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
# D. selectable paths no parity test reached, at oracle size
def _walk_pair(ts, o, at, b):
    for bb in range(at, b):
        ts.shiftE(bb, True); o.shiftE(bb, True)
    ts.setBond(b); o.set_bond(b)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [120, 40, 61, 12])
def test_unfused_gradient_tiles_match_the_oracle(m):
    """fuse_z = 0: k_zprime forms Z' = sum_l dP_l E_l first and the gradient GEMM runs its unfused fp64 tiles -- 240 x 80 at m = 120, 80 x 80 at
    m = 40, the generic tiles at m = 61, 32 x 32 at m = 12 -- for both bond kinds with the Label index on an environment: gradient, the CG and
    one bond update against the oracle; the same sums as the fused form (fuse_z = 1) to 1e-13."""
    from conftest import make_problem
    from tnml_amd.fixedl import TrainStates
    N, NT = 20, 300
    pixels, labels, phi, W = make_problem(N, NT, m, 7, pixel_boost=BOOST)
    ts = TrainStates(labels, N, m, phi=phi)
    ts.set_option("fuse_z", 0)
    ts.set_mps(W)
    ts.init()
    o = _oracle(phi, labels, W)
    rng = np.random.default_rng(1)
    at = 1
    for b, kind in ((8, "Label on RE"), (12, "Label on LE")):
        _walk_pair(ts, o, at, b)
        at = b
        B = o.bond_tensor(b)
        B = B + 0.05 * rng.standard_normal(B.shape)
        ts.profile(True, only="zprime,bgemm,grad_quad")
        ts.profile_reset()
        G = ts.gradient(B)
        ts.profile(False)
        pr = ts.profile_read()
        assert pr["zprime"][0] == 1 and pr["bgemm"][0] >= 1 and pr.get("grad_quad", (0, 0))[0] == 0, (kind, pr)
        assert tr.relmax(G, o.gradient(B)) < F64["G"], kind
        assert np.array_equal(G, ts.gradient(B)), kind
        ts.set_option("fuse_z", 1)
        ts.profile(True, only="zprime")
        ts.profile_reset()
        Gf = ts.gradient(B)
        ts.profile(False)
        assert ts.profile_read().get("zprime", (0, 0))[0] == 0, kind
        ts.set_option("fuse_z", 0)
        assert tr.relmax(G, Gf) < 1e-13, kind
        Bg, tg = ts.cgrad(B, NPASS, LAM, CCONV)
        Bo, to = o.cgrad(B, NPASS, LAM, CCONV)
        np.testing.assert_allclose(tg["cost"], to["cost"], rtol=F64["cgc"], err_msg=kind)
        np.testing.assert_allclose(tg["alpha"], to["alpha"], rtol=F64["cga"], err_msg=kind)
        assert tr.relmax(Bg, Bo) < F64["cga"], kind
    r = ts.bond_update(12, 1, m, m // 2, 1e-10, NPASS, LAM, CCONV)
    o.set_bond(12)
    B, _ = o.cgrad(o.bond_tensor(12), NPASS, LAM, CCONV)
    newm, te, _ = o.svd_split(B, 12, 1, 1e-10, m, m // 2)
    C, lc, cr, nc = o.quadcost(o.bond_tensor(12), LAM)
    assert r["newm"] == newm and r["ncorrect"] == nc and r["cost"] == pytest.approx(C, rel=1e-8)
    ts.close()


@pytest.mark.gpu
@pytest.mark.parametrize("NT,grid", [(300, 0), (2100, 16)])
def test_pacing_variants_of_the_resident_forward_kernel_are_bit_identical(NT, grid):
    """res_pace 1..4 are four more instantiations of k_fwd_res on 120 x 120 bonds: pauses of the GEMM waves between groups of MFMAs.  A pause
    changes when an instruction issues, not what it computes or in which order the sums are formed, so the outputs must be the SAME BITS as
    res_pace = 0 -- and within 1e-11 of the oracle.  300 images: two rounds per pair of workgroups; 2 100 images on 16 workgroups: nine."""
    from conftest import make_problem
    from tnml_amd.fixedl import TrainStates
    N, m = 20, 120
    pixels, labels, phi, W = make_problem(N, NT, m, 7, pixel_boost=BOOST)
    ts = TrainStates(labels, N, m, phi=phi)
    ts.set_option("fwd_res", 2)
    if grid:
        ts.set_option("res_grid", grid)
    ts.set_mps(W)
    ts.init()
    o = _oracle(phi, labels, W)
    rng = np.random.default_rng(1)
    at = 1
    for b, kind in ((8, "Label on RE"), (12, "Label on LE")):
        _walk_pair(ts, o, at, b)
        at = b
        B = o.bond_tensor(b)
        B = B + 0.05 * rng.standard_normal(B.shape)
        Po = o.forward(B)
        ts.set_option("res_pace", 0)
        P0 = ts.forward(B)
        assert tr.relmax(P0, Po) < F64["P"], kind
        for pace in (1, 2, 3, 4):
            ts.set_option("res_pace", pace)
            ts.profile(True, only="fwd_res,fgemm_fwd")
            ts.profile_reset()
            P = ts.forward(B)
            ts.profile(False)
            pr = ts.profile_read()
            assert pr["fwd_res"][0] == 1 and pr.get("fgemm_fwd", (0, 0))[0] == 0, (kind, pace, pr)
            assert np.array_equal(P, P0), (kind, pace, tr.relmax(P, P0))
            assert tr.relmax(P, Po) < F64["P"], (kind, pace)
            C0, Co = ts.quadcost(B, LAM), o.quadcost(B, LAM)
            assert C0[0] == pytest.approx(Co[0], rel=F64["C"]) and C0[3] == Co[3], (kind, pace)
    ts.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fast_cg,reuse_p", [(0, 1), (1, 0), (0, 0)])
def test_sweep_in_the_literal_evaluation_order_matches_the_oracle(fast_cg, reuse_p):
    """fast_cg = 0 (every CG pass re-evaluates B*t.v instead of updating P), reuse_p = 0 (the after-SVD cost from a fresh forward pass) and both
    -- "the reference's literal evaluation order": a full sweep of the test_full_sweep_reports_match_oracle problem against the oracle's at
    that test's tolerances, and against the default (fast_cg = reuse_p = 1) sweep to the same sweep_rtol."""
    from conftest import make_problem
    from tnml_amd.fixedl import TrainStates, mldmrg
    N, NT, m, sweep_rtol = 10, 40, 4, 1e-8
    pixels, labels, phi, W = make_problem(N, NT, m, 3, pixel_boost=BOOST)
    runs = []
    for opts in ({"fast_cg": fast_cg, "reuse_p": reuse_p}, {"fast_cg": 1, "reuse_p": 1}):
        ts = TrainStates(labels, N, m, phi=phi)
        for k, v in opts.items():
            ts.set_option(k, v)
        ts.set_mps(W)
        ts.init()
        runs.append(mldmrg(ts, 1, 4, 2, 1e-10, 3, LAM, CCONV))
        ts.close()
    o = _oracle(phi, labels, W)
    ro = o.mldmrg(1, 4, 2, 1e-10, 3, LAM, CCONV)
    rg, rd = runs
    assert len(rg) == len(rd) == len(ro) == 2 * (N - 1)
    for a, d, b in zip(rg, rd, ro):
        assert (a["bond"], a["half"], a["origm"], a["newm"]) == (b["bond"], b["half"], b["origm"], b["newm"])
        assert a["cost"] == pytest.approx(b["cost"], rel=sweep_rtol)
        assert a["ncorrect"] == b["ncorrect"]
        np.testing.assert_allclose(a["label_cost"], b["label_cost"], rtol=10 * sweep_rtol, atol=sweep_rtol * b["cost"])
        assert a["newm"] == d["newm"] and a["ncorrect"] == d["ncorrect"]
        assert a["cost"] == pytest.approx(d["cost"], rel=sweep_rtol)
    assert rg[0]["cost"] == pytest.approx(ro[0]["cost"], rel=F64["cgc"])
    assert rg[0]["truncerr"] == pytest.approx(ro[0]["truncerr"], rel=1e-3, abs=1e-12)
    np.testing.assert_allclose(rg[0]["cg"]["cost"], ro[0]["cg"]["cost"][:len(rg[0]["cg"]["cost"])], rtol=F64["cgc"])
