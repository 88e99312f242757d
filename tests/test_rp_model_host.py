"""The reference of the reduced-precision gate (tests/rp_model.py) proved before it judges a kernel -- no GPU.

1. the rounding helpers against torch's float32 -> bfloat16 conversion, bit for bit;
2. with the rounding helpers replaced by the identity the three models equal the fp64 oracle to 1e-12: their index maps are the oracle's;
3. the gate has teeth: at every shape test_rp_model_gpu.py runs, each planted defect moves the model's result by at least 10 x bound
   somewhere.  The inputs of part 3 are made for that: positive operands (non-cancelling sums) whose bf16 rounding error has one sign
   (x = c (1 +- 3 * 2^-11) with c a bf16 number), because a worst-case bound grows with n and a sum of random-sign errors with sqrt(n);
4. the scalar epilogue of the fp32 label dot (cost_model, pap_model; with exact operands they equal the oracle's quadcost in part 2): a dropped
   image, an image under the wrong label, a padded image that counts and the last maximum on a tie each miss the gate;
5. the gradient at the slab cuts of 24 576 / 25 000 images on sparse probes: the whole set and its probes give the same bits, and a lost or
   doubled chunk and a lost slab are thousands of the short-chain bounds away."""
import numpy as np
import pytest

import rp_model as rp
from conftest import make_problem

NL = rp.NL


# ---- 1. rounding helpers ----------------------------------------------------------------------------
def _f32_inputs():
    rng = np.random.default_rng(0)
    bits = [rng.integers(0, 0x7F800000, 200000, dtype=np.uint32)]                                   # dense: every exponent, random mantissas
    base = rng.integers(0x00010000, 0x7F000000, 20000, dtype=np.uint32) & np.uint32(0xFFFF0000)
    bits += [base | np.uint32(0x8000),                                                              # exact ties: to even, down (even hi) and up (odd hi)
             base | np.uint32(0x7FFF), base | np.uint32(0x8001)]                                    # one below / above a tie
    bits += [np.array([0x3F7FFFFF, 0x3FFFFFFF, 0x3F7F8000, 0x3F7F7FFF, 0x7F7F7FFF], dtype=np.uint32)]   # carry into the exponent
    bits += [rng.integers(1, 0x00800000, 20000, dtype=np.uint32),                                   # below 2^-126
             np.array([0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00800000], dtype=np.uint32)]
    bits += [np.array([0], dtype=np.uint32)]                                                        # zero
    u = np.concatenate(bits)
    u = np.concatenate([u, u | np.uint32(0x80000000)])                                              # both signs
    return u.view(np.float32)


def test_rounding_helpers_equal_torch_bit_for_bit():
    """to_bf16 / to_f32 against torch on every input of _f32_inputs, bit for bit.  hi + lo reproduces x to 2^-16 relative for every
    input that bf16 can hold that well: not from 0x7F7F8000 on, where the kernels' bit formula rounds hi to infinity (asserted to be
    exactly those inputs), and below 2^-100 only to the absolute floor 2^-133 of the format, because lo underflows there."""
    import torch
    x = _f32_inputs()
    ref = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).to(torch.float32).numpy()
    got = rp.to_bf16(x.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    tie = x.view(np.uint32) & np.uint32(0xFFFF) == np.uint32(0x8000)
    odd = (x.view(np.uint32) >> np.uint32(16)) & np.uint32(1) == 1
    assert (tie & odd).sum() > 1000 and (tie & ~odd).sum() > 1000                                   # ties in both directions are in the set
    assert np.array_equal(rp.to_f32(x.astype(np.float64)).astype(np.float32).view(np.uint32), x.view(np.uint32))
    d = np.random.default_rng(1).standard_normal(100000) * 1e3                                      # float64 inputs: fp32 rounding first
    assert np.array_equal(rp.to_f32(d), torch.tensor(d, dtype=torch.float64).to(torch.float32).to(torch.float64).numpy())
    assert np.array_equal(rp.to_bf16(d), torch.tensor(d, dtype=torch.float64).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy())
    # hi + lo reproduces x to 2^-16 relative (normal numbers whose lo part is not below the subnormal range)
    xx = x.astype(np.float64)
    hi, lo = rp.split_bf16(xx)
    fin = np.isfinite(hi)                                                                           # from 0x7F7F8000 on the bit formula rounds to infinity
    assert np.array_equal(~fin, (x.view(np.uint32) & np.uint32(0x7FFFFFFF)) >= np.uint32(0x7F7F8000))
    ok = fin & (np.abs(xx) >= 2.0 ** -100)
    err = np.abs(np.where(fin, hi, 0.) + np.where(fin, lo, 0.) - xx)
    assert np.all(err[ok] <= 2.0 ** -16 * np.abs(xx)[ok])
    assert np.all(err[fin] <= np.maximum(2.0 ** -16 * np.abs(xx), 2.0 ** -133)[fin])                   # below: the absolute floor of bf16


def test_slab_cut_of_the_issue_shapes():
    """bgemm_cut restates launch_bgemm: m = 150 with the Label on B at 700 (768 padded) images is five slabs of 160, the last of 128; a
    small bond at 40 images is one 32-image chunk per slab"""
    for mode in rp.MODES:
        c = rp.bgemm_cut(mode, 150, 150, NL, 768, 150)
        assert (c["tile"], c["nsplit"], c["per"], c["last"]) == (64, 5, 160, 128), (mode, c)
        c = rp.bgemm_cut(mode, 16, 16, 1, 256, 33)
        assert (c["tile"], c["nsplit"], c["per"]) == (32, 8, 32), (mode, c)
    assert rp.bgemm_cut("f32", 40, 40, 1, 256, 120)["tile"] == 80 and rp.bgemm_cut("bf16", 40, 40, 1, 256, 120)["tile"] == 64
    assert rp.bgemm_cut("f32", 80, 40, 1, 256, 120)["tile"] == 80 and rp.bgemm_cut("bf16", 80, 40, 1, 256, 120)["tile"] == 80
    assert rp.bgemm_cut("f32", 120, 120, NL, 256, 120)["tile"] == 80 and rp.bgemm_cut("bf16x3", 120, 120, NL, 256, 120)["tile"] == 64
    assert rp.bgemm_cut("f32", 33, 17, 1, 256, 33)["tile"] == 64 and rp.bgemm_cut("f32", 9, 5, 1, 256, 80)["tile"] == 32
    # at real image counts with maxm = 40 (test_rp_model_gpu.py, the long-slab cases): (tile, slabs, images per slab, images of the last slab)
    for (mode, NTp, m), want in {("f32", 24576, 40): (80, 12, 2048, 2048), ("f32", 25088, 40): (80, 12, 2112, 1856), ("f32", 25088, 16): (32, 79, 320, 128),
                                 ("bf16", 24576, 40): (64, 15, 1664, 1280), ("bf16x3", 24576, 40): (64, 15, 1664, 1280)}.items():
        c = rp.bgemm_cut(mode, m, m, NL, NTp, 40)
        assert (c["tile"], c["nsplit"], c["per"], c["last"]) == want, (mode, NTp, m, c)
    dims = {b: (mI, mO) for b, _, mI, mO, _ in rp.bonds_of(rp.SCALE_DIMS)}
    kinds = {b: kind for b, kind, _, _, _ in rp.bonds_of(rp.SCALE_DIMS)}
    assert max(rp.SCALE_DIMS) == 40 and all(dims[b] == v for b, v in {**rp.SCALE_GRAD_BONDS, **rp.SCALE_THRESHOLD_BONDS}.items())
    assert (kinds[3], kinds[4], kinds[5], kinds[6]) == (0, 2, 2, 1)
    assert all(NT % rp.NTPAD == 0 for NT in rp.SCALE_THRESHOLD)                                   # labeldot_streaming: NTp / 128 >= 192
    assert {NT: (1 if NT // 128 >= 192 else 2) for NT in rp.SCALE_THRESHOLD} == rp.SCALE_THRESHOLD and sorted(NT // 128 for NT in rp.SCALE_THRESHOLD) == [190, 192]


# ---- 2. exact operands equal the oracle -------------------------------------------------------------
def _relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _exact_walk(o, phi, labels, N, single, target, capsys):
    ex = rp.ExactModel()
    NT = phi.shape[0]
    one = np.ones((NT, 1))
    rng = np.random.default_rng(4)
    worst = 0.
    for j in range(N, 2, -1):                                           # the environments of init: shifts from the right
        got, _ = ex.shift_model("f32", o.env(j + 1) if j < N else None, phi[:, j - 1], o.get_site(j), False)
        worst = max(worst, _relmax(got, o.env(j)))
    for b in range(1, N):
        o.set_bond(b)
        B = o.bond_tensor(b)
        B = B + 0.1 * np.abs(B).max() * rng.standard_normal(B.shape)
        EL = o.env(b - 1) if b > 1 else one
        ER = o.env(b + 2) if b + 2 <= N else one
        kind = rp.kind_of(B, EL, ER)
        assert (kind == 2) == (B.ndim == 5 or single)
        EI, phiI, phiO, EX = rp.plan(kind, EL, phi[:, b - 1], ER, phi[:, b])
        Po = o.forward(B)
        P, _ = ex.forward_model("f32", "staged", kind, EI, phiI, B, phiO, EX)
        eP = _relmax(P.reshape(Po.shape), Po)
        eP1 = eP
        if kind != 2:
            P1, _ = ex.forward_model("bf16x3", "once", kind, EI, phiI, B, phiO, EX)
            eP1 = _relmax(P1, Po)
        G, _ = ex.gradient_model("f32", kind, EI, phiI, phiO, EX, Po, labels, 32, B.ndim, target=target)
        eG = _relmax(G, o.gradient(B))
        lam = 1e-3                                                     # the scalar epilogue: cost_model / pap_model on the oracle's own outputs
        cm, q = ex.cost_model(Po, labels, target), o.quadcost(B, lam)
        reg = lam * float(np.sum(B * B))
        eC = abs(cm["cost"] + reg - q[0]) / q[0]
        assert (q[1] if single else q[2]) == pytest.approx(reg, rel=1e-12)
        if not single:
            assert cm["ncorrect"] == q[3], b
            eC = max(eC, _relmax(cm["label_cost"], q[1]))
        p = rng.standard_normal(B.shape)
        Pp = o.forward(p)
        eC = max(eC, abs(ex.pap_model(Pp)[0] / float(np.sum(Pp * Pp)) - 1.0))
        o.shiftE(b, True)
        E, _ = ex.shift_model("f32", o.env(b - 1) if b > 1 else None, phi[:, b - 1], o.get_site(b), True)
        eE = _relmax(E, o.env(b))
        with capsys.disabled():
            print("\n  exact-operand model vs oracle%s, bond %d (kind %d, %s): P %.1e (converted-once path %.1e)  G %.1e  shifted E %.1e  cost, pAp %.1e"
                  % (" (per-label)" if single else "", b, kind, "x".join(map(str, B.shape)), eP, eP1, eG, eE, eC), end="")
        worst = max(worst, eP, eP1, eG, eE, eC)
    return worst


def test_exact_operands_equal_the_oracle(capsys):
    """rounding helpers replaced by the identity: forward, gradient and shift models against oracle.pyoracle on a chain with unequal, odd
    bond dimensions -- every bond kind"""
    from oracle import pyoracle
    from test_gpu_parity import _mps_with_dims
    dims = [1, 2, 3, 5, 9, 7, 5, 3, 4, 2, 1]
    N, NT = len(dims) - 1, 30
    _, labels, phi, _ = make_problem(N, NT, 2, 5, pixel_boost=200.0)
    o = pyoracle.Oracle(phi, labels, _mps_with_dims(dims, 11))
    o.init()
    assert _exact_walk(o, phi, labels, N, False, None, capsys) < 1e-12


def test_exact_operands_equal_the_per_label_oracle(capsys):
    from oracle import pyoracle
    from tnml_amd import synth
    import tiled_reference as tr
    dims = [1, 2, 3, 7, 5, 4, 3, 2, 1]
    N, NT, target = len(dims) - 1, 30, 3
    labels = synth.synthetic_labels(NT, seed=5, per_label=NT // 10)
    phi = pyoracle.features_single(synth.synthetic_images(N, labels, seed=5), True).copy()
    phi[..., 1] *= 300.0
    o = pyoracle.SingleOracle(phi, labels, target, tr.plain_mps_with_dims(dims, 11))
    o.init()
    assert _exact_walk(o, phi, labels, N, True, target, capsys) < 1e-12


# ---- 3. the gate has teeth ----------------------------------------------------------------------------
class DropLastK(rp.Model):
    def klen(self, K):
        return K - 1


class DropLastChunk(rp.Model):
    def nimg(self, NT):
        return 32 * ((NT - 1) // 32)                 # the last 32-image chunk that holds a real image (chunks of padding alone sum zeros)


class DropCross(rp.Model):
    def __init__(self, which):
        self.which = which

    def terms(self, nplanes):
        return [t for t in rp.Model.terms(self, nplanes) if t != self.which]


class Truncate(rp.Model):
    def bf(self, x):
        return rp.trunc_bf16(x)


class SwapT(rp.Model):
    def epilogue_phi(self, phiO):
        return phiO[:, ::-1]


def _shapes():
    """(name, kind, mI, mO, L, NT) of every bond the GPU gate checks, once each"""
    out, seen = [], set()

    def add(name, dims, NT, bonds=None, single=False):
        for b, kind, mI, mO, L in rp.bonds_of(dims, single):
            if bonds is not None and b not in bonds:
                continue
            key = (kind, mI, mO, L, NT)
            if key not in seen:
                seen.add(key)
                out.append(("%s-b%d" % (name, b),) + key)
    add("forward", rp.FORWARD_DIMS, 40)
    for i, (dims, bonds) in enumerate(rp.GRAD_CHAINS):
        add("grad%d" % i, dims, rp.GRAD_NT, bonds)
    add("slab", rp.SLAB_DIMS, rp.SLAB_NT, (rp.SLAB_BOND,))
    for NT in rp.RAGGED_NTS:
        add("ragged%d" % NT, rp.RAGGED_DIMS, NT, rp.RAGGED_BONDS)
    add("single", rp.SINGLE_DIMS, rp.SINGLE_NT, None, True)
    out.append(("stale-b%d" % rp.STALE["bond"], 0, rp.STALE["m"], rp.STALE["m"], 1, rp.STALE["NT"]))
    return out


def _shift_shapes():
    """(m_in, m_out, where the Label index is: 0 nowhere, 1 on the site, 2 on the incoming environment) of the shifts the GPU gate checks"""
    seen = []
    for dims, single in [(rp.FORWARD_DIMS, False)] + [(d, False) for d, _ in rp.GRAD_CHAINS] + [(rp.SLAB_DIMS, False), (rp.RAGGED_DIMS, False), (rp.SINGLE_DIMS, True)]:
        N = len(dims) - 1
        for b in range(1, N):
            lab = 0 if single or b < N // 2 else (1 if b == N // 2 else 2)
            key = (dims[b - 1], dims[b], lab)
            if key not in seen:
                seen.append(key)
    return seen


def _teeth_inputs(kind, mI, mO, L, NT, sign, seed):
    rng = np.random.default_rng(seed)

    def sysv(shape):                                 # bf16 numbers moved by +-3 * 2^-11 relative: exact in fp32, rounding error of one sign
        return rp.to_f32(rp.to_bf16(rng.uniform(0.5, 2.0, shape)) * (1.0 + sign * 3 * 2.0 ** -11))

    def feat():
        return np.stack([np.ones(NT), rp.to_f32(rng.uniform(0.3, 1.0, NT))], axis=1)
    EI = sysv((NT, mI))
    EX = sysv((NT, mO)) if kind == 2 else sysv((NT, mO, NL))
    Bshape = (mO, 2, 2, mI) if kind == 1 else (mI, 2, 2, mO) + ((NL,) if L == NL else ())
    P = -rp.to_f32(rng.uniform(0.1, 1.0, (NT, NL if (kind != 2 or L == NL) else 1)))        # residuals of one sign: non-cancelling weights
    drift = 1.0 - 0.008 * rng.uniform(0.5, 1.0, (NT, 1))                                    # the environment before a shift that moved it by < 1 %
    return dict(EI=EI, phiI=feat(), B=sysv(Bshape), phiO=feat(), EX=EX, P=P, labels=rng.integers(0, NL, NT), stale=rp.to_f32(EI * drift))


def _factor(a, b, bound):
    d = np.abs(np.asarray(a) - np.asarray(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / bound, 0.)
    return float(r.max())


@pytest.mark.parametrize("name,kind,mI,mO,L,NT", _shapes(), ids=[s[0] for s in _shapes()])
def test_every_planted_defect_is_at_least_ten_bounds_away(name, kind, mI, mO, L, NT, capsys):
    NTp = -(-NT // rp.NTPAD) * rp.NTPAD
    single = kind == 2 and L == 1
    lines, worst = [], np.inf
    for mode in rp.MODES:
        d = _teeth_inputs(kind, mI, mO, L, NT, +1 if mode == "bf16x3" else -1, 7)
        per = rp.bgemm_cut(mode, mI, mO, L, NTp, max(mI, mO))["per"]
        fw = lambda m, path, EI=None: m.forward_model(mode, path, kind, d["EI"] if EI is None else EI, d["phiI"], d["B"], d["phiO"], d["EX"])
        gr = lambda m: m.gradient_model(mode, kind, d["EI"], d["phiI"], d["phiO"], d["EX"], d["P"], d["labels"], per, d["B"].ndim,
                                        target=3 if single else None)
        res = {}
        for path in ["staged"] + (["once"] if mode != "f32" and kind != 2 else []):
            P, bound = fw(rp.Model(), path)
            res["fwd/%s: last reduction index dropped" % path] = _factor(fw(DropLastK(), path)[0], P, bound)
            res["fwd/%s: output site index swapped" % path] = _factor(fw(SwapT(), path)[0], P, bound)
            if mode == "bf16x3":
                res["fwd/%s: cross term dropped" % path] = _factor(fw(DropCross((0, 1)), path)[0], P, bound)
            if mode == "bf16":
                res["fwd/%s: truncation" % path] = _factor(fw(Truncate(), path)[0], P, bound)
            if path == "once":
                res["fwd/once: stale environment"] = _factor(fw(rp.Model(), path, d["stale"])[0], P, bound)
        G, bound = gr(rp.Model())
        res["grad: last image chunk dropped"] = _factor(gr(DropLastChunk())[0], G, bound)
        if mode == "bf16x3":
            res["grad: cross term dropped"] = _factor(gr(DropCross((1, 0)))[0], G, bound)
        if mode == "bf16":
            res["grad: truncation"] = _factor(gr(Truncate())[0], G, bound)
        lines.append("  %-14s %-6s " % (name, mode) + "; ".join("%s %.3g" % kv for kv in res.items()))
        for k, v in res.items():
            assert v >= 10., "%s (%s, kind %d, %d x %d, %d images): '%s' moves the model by only %.3g x bound" % (name, mode, kind, mI, mO, NT, k, v)
            worst = min(worst, v)
    with capsys.disabled():
        print("\n" + "\n".join(lines) + "\n  %-14s smallest defect / bound: %.3g" % (name, worst), end="")


@pytest.mark.parametrize("m_in,m_out,lab", _shift_shapes())
def test_a_dropped_reduction_index_in_the_shift_is_at_least_ten_bounds_away(m_in, m_out, lab, capsys):
    rng = np.random.default_rng(9)
    NT = 40
    E = rp.to_f32(rng.uniform(0.5, 2.0, (NT, m_in) + ((NL,) if lab == 2 else ())))
    A = rng.uniform(0.5, 2.0, (m_in, 2, m_out) + ((NL,) if lab == 1 else ()))
    phi = np.stack([np.ones(NT), rp.to_f32(rng.uniform(0.3, 1.0, NT))], axis=1)
    out, bound = rp.Model().shift_model("f32", E, phi, A, True)
    f = _factor(DropLastK().shift_model("f32", E, phi, A, True)[0], out, bound)
    with capsys.disabled():
        print("\n  shift %d -> %d (Label %s): last reduction index dropped %.3g x bound" % (m_in, m_out, ("nowhere", "on the site", "on the environment")[lab], f), end="")
    assert f >= 10.


# ---- 4. the scalar epilogue of the fp32 label dot -----------------------------------------------------
class DropOneImage(rp.Model):
    def __init__(self, n):
        self.n = n

    def cost_images(self, NT):
        return np.delete(np.arange(NT), self.n)


class WrongBucket(rp.Model):
    def __init__(self, n):
        self.n = n

    def bucket(self, labels):
        out = np.array(labels)
        out[self.n] = (out[self.n] + 1) % NL
        return out


class LastMaximum(rp.Model):
    def argmax(self, a):
        return a.shape[1] - 1 - np.argmax(a[:, ::-1], axis=1)


def _cost_miss(bad, good):
    """(largest |defect - model| / gate over the cost and the per-label costs, difference of #correct)"""
    r = abs(bad["cost"] - good["cost"]) / good["cost_gate"]
    r = max(r, float((np.abs(bad["label_cost"] - good["label_cost"]) / good["gate"]).max()))
    return r, bad["ncorrect"] - good["ncorrect"]


@pytest.mark.parametrize("target", [None, 3], ids=["ten-labels", "per-label"])
@pytest.mark.parametrize("NT", [rp.SCALE_LDOT_NT] + sorted(rp.SCALE_THRESHOLD))
def test_every_planted_defect_of_the_cost_epilogue_misses_its_gate_ten_times(NT, target, capsys):
    """cost_model / pap_model at the image counts of the GPU cases, on outputs of the size the kernels produce: one image dropped, one image
    summed under the wrong label, a padded image that counts (as label 0 with outputs 0: one unit of cost for the ten labels, a 'correct'
    image in the per-label variant), the LAST maximum on a planted tie of |P|.  The cost defects move a gated figure by at least 10 gates;
    the two that move #correct move it by one, and its gate is equality."""
    rng = np.random.default_rng(NT)
    L = NL if target is None else 1
    labels = rng.integers(0, NL, NT)
    P = rp.to_f32(0.3 * rng.standard_normal((NT, L)) + (labels[:, None] == (np.arange(L)[None, :] if target is None else target)))
    n = NT // 3
    if target is None:                                               # the tie: the image's own label and a later one share the largest |P|
        a = int(labels[n]) if labels[n] < NL - 1 else 0
        labels[n] = a
        P[n] = rp.to_f32(0.1 * rng.uniform(-1, 1, L))
        P[n, a], P[n, NL - 1] = 0.75, -0.75
    good = rp.cost_model(P, labels, target)
    res = {"one image dropped": _cost_miss(DropOneImage(n).cost_model(P, labels, target), good),
           "one image under the wrong label": _cost_miss(WrongBucket(n).cost_model(P, labels, target), good),
           "a padded image counted": _cost_miss(rp.cost_model(np.vstack([P, np.zeros((1, L))]), np.append(labels, 0), target), good)}
    assert res["one image dropped"][0] >= 10. and res["one image under the wrong label"][0] >= 10.
    assert res["a padded image counted"][1] == 1 and (target is not None or res["a padded image counted"][0] >= 10.)
    if target is None:
        res["the last maximum on a tie"] = _cost_miss(LastMaximum().cost_model(P, labels, target), good)
        assert res["the last maximum on a tie"] == (0., -1)
    s, gate = rp.pap_model(P)
    res["pAp: one image dropped"] = (abs(DropOneImage(n).pap_model(P)[0] - s) / gate, 0)
    assert res["pAp: one image dropped"][0] >= 10.
    assert gate < 1e-6 * s and np.all(good["gate"] < 1e-6 * good["label_cost"])              # the gates themselves: far below the f32 tolerances
    with capsys.disabled():
        print("\n  %5d images, %s: " % (NT, "ten labels" if target is None else "per-label") +
              "; ".join("%s %.3g gates, #correct %+d" % ((k,) + v) for k, v in res.items()), end="")


# ---- 5. the gradient with long slabs: sparse probes ----------------------------------------------------
class Images(rp.Model):
    """the gradient over the images `idx` (indices into the WHOLE set; repeats allowed) of arguments that hold the rows `rows` of it"""

    def __init__(self, idx, rows):
        self.idx, self.rows = np.asarray(idx), np.asarray(rows)

    def images(self, NT):
        i = self.idx[np.isin(self.idx, self.rows)]                   # every other image is zero and adds nothing
        return np.searchsorted(self.rows, i)


def _sparse_cases():
    """(name, mode, NT, bond, kind, mI, mO, L) of the sparse GPU cases"""
    out = []
    for NT in rp.SCALE_NTS:
        for b, kind, mI, mO, L in rp.bonds_of(rp.SCALE_DIMS):
            if b in rp.SCALE_GRAD_BONDS:
                out += [("%s-%d-b%d" % (mode, NT, b), mode, NT, b, kind, mI, mO, L) for mode in rp.MODES]
    return out


@pytest.mark.parametrize("name,mode,NT,b,kind,mI,mO,L", _sparse_cases(), ids=[c[0] for c in _sparse_cases()])
def test_sparse_probes_identity_and_planted_slab_defects(name, mode, NT, b, kind, mI, mO, L, capsys):
    """A set in which every image outside the probe set S (rp.probe_set of the bond's slab cut) has all-zero environments: gradient_model
    on the whole set equals gradient_model on the rows of S BIT FOR BIT (bonds 4 and 5: kind 2, bond 6: kind 1; kind 0 with the roles of
    bond 6 exchanged), and the bound with the chain length of S is the whole-set bound times (chain nt + 4) / (per nt + 4).  Planted at
    that layout, each of these is at least 10 of the short bounds away: a 32-image chunk that holds a probe dropped, a slab boundary
    moved by one chunk (the first chunk of the next slab summed twice / not at all), the last slab dropped."""
    NTp = -(-NT // rp.NTPAD) * rp.NTPAD
    cut = rp.bgemm_cut(mode, mI, mO, L, NTp, max(rp.SCALE_DIMS))
    S, chain = rp.probe_set(cut, NT)
    per, ns = cut["per"], cut["nsplit"]
    last = (NT - 1) // per                                           # the last slab that holds a real image
    assert chain <= 4 and len(S) >= 2 * (last + 1) and {0, NT - 1, per - 1, per, last * per} <= set(S)
    lines = []
    for kd in ((kind,) if kind == 2 else (0, 1)):
        d = _teeth_inputs(kd, mI, mO, L, len(S), +1 if mode == "bf16x3" else -1, 11)
        whole = {k: np.zeros((NT,) + d[k].shape[1:]) for k in ("EI", "EX", "P")}
        for k in whole:
            whole[k][S] = d[k]
        labels = np.random.default_rng(5).integers(0, NL, NT)
        phiI, phiO = (np.stack([np.ones(NT), np.linspace(0.3, 1.0, NT)], axis=1) for _ in range(2))
        args = lambda rows: (mode, kd, whole["EI"][rows], phiI[rows], phiO[rows], whole["EX"][rows], whole["P"][rows], labels[rows], per, d["B"].ndim)
        Gw, bw = rp.gradient_model(*args(slice(None)))
        Gs, bs = rp.gradient_model(*args(S), chain=chain)
        assert np.array_equal(Gw, Gs), "the whole set and its probes differ"
        nt = 3 if mode == "bf16x3" else 1
        np.testing.assert_allclose(bs * (per * nt + 4), bw * (chain * nt + 4), rtol=1e-14)
        chunk = lambda c: np.arange(32 * c, min(32 * c + 32, NT))
        k = ns // 2                                                  # the slab boundary k per: its first chunk holds the probe k per
        keep = np.arange(NT)
        res = {"the chunk of probe %d dropped" % S[len(S) // 2]: np.setdiff1d(keep, chunk(S[len(S) // 2] // 32)),
               "boundary %d one chunk late: a chunk twice" % k: np.concatenate([keep, chunk(k * per // 32)]),
               "boundary %d one chunk late: a chunk not at all" % k: np.setdiff1d(keep, chunk(k * per // 32)),
               "the last slab dropped": keep[keep < last * per]}
        for what, idx in res.items():
            f = _factor(Images(idx, S).gradient_model(*args(S), chain=chain)[0], Gs, bs)
            assert f >= 10., "%s kind %d: '%s' moves the model by only %.3g x bound" % (name, kd, what, f)
            res[what] = f
        lines.append("  %-16s kind %d %2d slabs x %4d (last %4d), %3d probes, chain %d, bound %.0f x tighter: " % (name, kd, ns, per, cut["last"], len(S), chain, (per * nt + 4) / (chain * nt + 4))
                     + "; ".join("%s %.3g" % kv for kv in res.items()))
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")
