"""Well-conditioned long chains: the inputs tests/test_long_chain_host.py proves and tests/test_long_chain_gpu.py runs, N = 784, 197
and 196 sites -- the lengths the streamed calls (predict, evaluate, site_response, site_gradient, gradient_step) are used at.

sitegrad_model.mps_with_dims keeps a chain vector's scale over ten sites only: its noise is signed and of size 1 / sqrt(m) per site, so
over hundreds of sites the contraction on absolute values, which every rounding bound here is a multiple of, leaves the contraction
itself behind by tens of orders of magnitude and the bound sees nothing.  The generator here keeps the two together: the noise is mostly
of one sign (a fraction PNEG of it flipped) and O(1 / N) per site around the identity,

    site j != c:         E = |normal|, flipped with probability PNEG;  A = 8 E / (N max(ml, mr));  A[:, 1] *= 5;  A[:, 0] += eye(ml, mr)
    Label site c = N/2:  A = E / (2 max(ml, mr));  A[:, 0] += eye(ml, mr)[:, :, None] (0.5 + uniform(0, 1)[l])

(the factor per label separates the labels), on the bond dimensions [1, 2] + integers(3 .. top, N - 3) + [2, 1].  What these inputs must
satisfy before a GPU test may lean on them is asserted by tests/test_long_chain_host.py on the models alone.

The cases: the smallest at which each path that only a long chain reaches is taken.
    A     N = 784, bonds 3..24,  37 images   even N, one block per site, a 64-wide tile with a ragged end
    B     N = 197, bonds 3..40,  37 images   odd N (98 sites left of the Label site, 99 right of it), sites of 1, 2 and 4 blocks
    C     N = 784, bonds 3..130, 20 images   the 32-wide tile class (a bond above 128), up to 25 blocks per site, a tape of 50 000 rows
    D     N = 784, bonds 3..24,  37 images   the per-label variant (single_label = 3): no left chain, 783 right steps
    E196, E784   bonds 3..24, 20 images      raw 28 x 28 bytes through the device input map (from_imglen(28, 14 / 28, "normal"))
Every model is computed once per process and shared (model(), response_model(), f32_model())."""
import numpy as np

import chain32_model as cm
import response_model as rm
import sitegrad_model as sm
from conftest import make_problem

PNEG = 0.1
U = sm.U

#            N,   top bond, images, seed, tile (option predict_tile; 0: the dispatch's own), single_label, (side, imglen) of the map
CASES = {"A": dict(N=784, top=24, n=37, seed=101, tile=64),
         "B": dict(N=197, top=40, n=37, seed=112, tile=0),
         "C": dict(N=784, top=130, n=20, seed=243, tile=32),
         "D": dict(N=784, top=24, n=37, seed=114, tile=0, single=3),
         "E196": dict(N=196, top=24, n=20, seed=105, tile=0, imglen=(28, 14)),
         "E784": dict(N=784, top=24, n=20, seed=106, tile=0, imglen=(28, 28))}
_CACHE = {}


def forms(name):
    """the input forms of a case: given features and bytes, or raw bytes under the case's input map"""
    return ("map",) if "imglen" in CASES[name] else ("phi", "u8")


CASE_FORMS = [(name, form) for name in CASES for form in forms(name)]
MODES = ("labels", "coef")


def bond_dims(N, top, seed):
    """d_0 = 1, d_1, ..., d_N = 1"""
    rng = np.random.default_rng(seed)
    return [1, 2] + rng.integers(3, top + 1, N - 3).tolist() + [2, 1]


def long_mps(dims, seed):
    """the generator of the module's header on the bond dimensions dims; the Label index on site N // 2 (1-based)"""
    rng = np.random.default_rng([seed, 1])
    N = len(dims) - 1
    c = N // 2
    W = []
    for j in range(1, N + 1):
        ml, mr = dims[j - 1], dims[j]
        shape = (ml, 2, mr, 10) if j == c else (ml, 2, mr)
        E = np.abs(rng.standard_normal(shape))
        E = np.where(rng.random(shape) < PNEG, -E, E)
        if j == c:
            A = E / (2. * max(ml, mr))
            A[:, 0] += np.eye(ml, mr)[:, :, None] * (0.5 + rng.random(10))
        else:
            A = E * 8. / (N * max(ml, mr))
            A[:, 1] *= 5.
            A[:, 0] += np.eye(ml, mr)
        W.append(A)
    return W


def plain(W):
    """the per-label variant's W: no Label index"""
    return [A if A.ndim == 3 else A[..., 0] * 3.0 for A in W]


def dims_of(name):
    p = CASES[name]
    return bond_dims(p["N"], p["top"], p["seed"])


def case(name):
    """dict(W, labels, coef, target (the per-label variant's label or None), dims) and the images: pixels, phi (boosted features) and
    phi8 (the bytes' features), or under a map raw (the 28 x 28 bytes), imap and phi (the features the map defines)"""
    if ("case", name) not in _CACHE:
        from oracle import pyoracle
        p = CASES[name]
        N, n = p["N"], p["n"]
        dims = dims_of(name)
        W = long_mps(dims, p["seed"])
        d = dict(name=name, dims=dims, target=p.get("single"), W=plain(W) if "single" in p else W)
        nl = 1 if "single" in p else 10
        d["coef"] = np.random.default_rng(p["seed"] + n).standard_normal((n, nl))
        if "imglen" in p:
            from tnml_amd.input_map import InputMap
            d["imap"] = InputMap.from_imglen(p["imglen"][0], p["imglen"][1], "normal")
            assert d["imap"].N == N
            raw, labels, _, _ = make_problem(d["imap"].S, n, 2, 5, pixel_boost=200.0)     # the synthetic 28 x 28 images as raw bytes
            d.update(raw=np.ascontiguousarray(raw, dtype=np.uint8), phi=d["imap"].features(raw))
        else:
            pixels, labels, phi, _ = make_problem(N, n, 2, 5, pixel_boost=200.0)
            d.update(pixels=pixels, phi=phi, phi8=pyoracle.features_series(pixels))
        d["labels"] = np.asarray(labels, dtype=np.int32)
        _CACHE[("case", name)] = d
    return _CACHE[("case", name)]


def feats(name, form):
    """the fp64 features the device forms or is given in this form"""
    return case(name)["phi8" if form == "u8" else "phi"]


def coefs(name, mode):
    """the keyword that selects the mode in site_gradient() / gradient_step() and in the model"""
    d = case(name)
    return dict(labels=d["labels"]) if mode == "labels" else dict(coef=d["coef"])


def weight_count(N, m):
    """K_w of sitegrad_model's header: the roundings of one fp64 evaluation of a weight"""
    return N * (4 * m + 1) + 2 * m + 1


def model(name, form, mode):
    """dict(g, w, bound, w_abs, w_bound) of tests/sitegrad_model.py: the gradient with its elementwise bound, the weights [n, nl], their
    contraction on absolute values and the bound 2 K_w 2^-53 w_abs between two fp64 evaluations of them"""
    key = ("model", name, form, mode)
    if key not in _CACHE:
        d, f = case(name), feats(name, form)
        kw = dict(coefs(name, mode), target_label=d["target"]) if mode == "labels" else coefs(name, mode)
        g, w = sm.site_gradient(d["W"], f, **kw)
        if ("wabs", name, form) not in _CACHE:
            _CACHE[("wabs", name, form)] = sm._contract([np.abs(A) for A in d["W"]], np.abs(f), lambda x: np.zeros_like(x))[1]
        w_abs = _CACHE[("wabs", name, form)]
        m = max(d["dims"])
        _CACHE[key] = dict(g=g, w=w, bound=sm.bound(d["W"], f, **kw), w_abs=w_abs, w_bound=2 * weight_count(len(d["W"]), m) * U * w_abs)
    return _CACHE[key]


def pred_of(name, w):
    """the decision of tnml_classify on weights [n, nl]"""
    return (w[:, 0] > 0.5).astype(np.int32) if CASES[name].get("single") is not None else np.abs(w).argmax(axis=1).astype(np.int32)


def decision_gap(name, w):
    """per image, how far the weights are from another decision: the top-two gap of |W_l|, per-label variant |w - 1/2|"""
    if CASES[name].get("single") is not None:
        return np.abs(w[:, 0] - 0.5)
    s = np.sort(np.abs(w), axis=1)
    return s[:, -1] - s[:, -2]


def given_labels(name):
    """the labels of site_response(which=...): any, the per-label variant's all zero"""
    n = CASES[name]["n"]
    if CASES[name].get("single") is not None:
        return np.zeros(n, dtype=np.int32)
    return np.random.default_rng(17).integers(0, 10, size=n).astype(np.int32)


def response_model(name, form, chosen):
    """dict(resp, w, label, bound) of tests/response_model.py; chosen "own" (which = None: every image's prediction) or "given" """
    key = ("resp", name, form, chosen)
    if key not in _CACHE:
        d, f = case(name), feats(name, form)
        resp, w, label = rm.response(d["W"], f, None if chosen == "own" else given_labels(name))
        _CACHE[key] = dict(resp=resp, w=w, label=label, bound=rm.bound(d["W"], f, label))
    return _CACHE[key]


def f32_model(name, form):
    """(weights, pred) of tests/chain32_model.py"""
    key = ("f32", name, form)
    if key not in _CACHE:
        _CACHE[key] = cm.predict32(case(name)["W"], feats(name, form), single=CASES[name].get("single") is not None)
    return _CACHE[key]


def worst(err, bnd):
    """max |err| / bound over an array (0 / 0 counts as 0)"""
    err = np.abs(err)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0., err / bnd).max())
