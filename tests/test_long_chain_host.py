"""The long-chain cases (tests/long_chain_cases.py) and their yardsticks proved on the CPU before tests/test_long_chain_gpu.py leans on
them, at N = 784, 197 and 196:
  * the conditions on the inputs -- the gradient's bound is at most 1e-8 of every site's largest |G|, the weights are O(1), every
    decision is 1e4 weight bounds away from the next one, the fp32 model is finite.  These are no tolerances: a seed that misses one is
    changed, not the threshold;
  * the models against something independent of them: the Euler identity, the tie of the responses to the weights, the two fp64
    models' weights against each other, the fp32 model inside half of every image's decision gap;
  * seven planted defects, four of which only a long chain can carry, each at least 10 bounds away."""
import numpy as np
import pytest

import long_chain_cases as lc
import response_model as rm
import sitegrad_model as sm

SHORT = ["swap_s", "drop_image", "no_factor2"]            # sitegrad_model's own
LONG = ["swapped_neighbours_5_6", "swapped_neighbours_near_the_end", "skipped_site", "shifted_gradient"]


@pytest.mark.parametrize("name,form", lc.CASE_FORMS)
def test_the_inputs_give_the_bounds_teeth(name, form):
    d = lc.case(name)
    for mode in lc.MODES:
        m = lc.model(name, form, mode)
        assert [g.shape for g in m["g"]] == [A.shape for A in d["W"]]
        rel = max(float(b.max() / np.abs(g).max()) for g, b in zip(m["g"], m["bound"]))
        print(name, form, mode, "worst bound / max|G_j| over the sites %.3e" % rel)
        assert rel <= 1e-8
    w, w_bound = m["w"], m["w_bound"]
    gap = lc.decision_gap(name, w)
    print(name, form, "|w| %.3g .. %.3g, smallest decision gap %.3e, smallest gap / weight bound %.3e"
          % (np.abs(w).min(), np.abs(w).max(), gap.min(), (gap / w_bound.max(axis=1)).min()))
    assert np.abs(w).min() >= 0.05 and np.abs(w).max() <= 20.
    assert (gap >= 1e4 * w_bound.max(axis=1)).all()
    assert np.isfinite(lc.f32_model(name, form)[0]).all()


@pytest.mark.parametrize("name", list(lc.CASES))
def test_the_chosen_tile_is_within_the_class_of_the_largest_bond(name):
    """kernels_chain.hip (chain_tile): fp64 tiles of 64 images up to bond 128, of 32 up to 256, halved while workgroups are fewer than
    compute units -- 16 for these image counts -- unless option predict_tile asks for a width, which the class of the largest bond
    caps.  Case A asks for 64 and may have it, case C asks for 32 and its largest bond is in the 32 class"""
    top = max(lc.dims_of(name))
    assert top <= lc.CASES[name]["top"]
    assert lc.CASES[name]["tile"] <= (64 if top <= 128 else 32)
    if name == "C":
        assert top > 128


@pytest.mark.parametrize("mode", lc.MODES)
@pytest.mark.parametrize("name,form", lc.CASE_FORMS)
def test_euler_identity_at_the_first_the_label_and_the_last_site(name, form, mode):
    """W is linear in every site: sum A_j G_j = sum_n sum_l c_nl W_l(x_n), within the bound of G_j against |A_j| and the roundings of the
    right-hand side"""
    d, m = lc.case(name), lc.model(name, form, mode)
    N = len(d["W"])
    coef = d["coef"] if mode == "coef" else 2. * (m["w"] - sm.targets(d["labels"], m["w"].shape[1], d["target"]))
    K, _ = sm.rounding_counts(N, max(d["dims"]), len(coef), coef.shape[1])
    want = (coef * m["w"]).sum()
    rhs = K * sm.U * (np.abs(coef) * m["w_abs"]).sum()
    c = 0 if d["target"] is not None else N // 2 - 1
    for j in (0, c, N - 1):
        A, G = d["W"][j], m["g"][j]
        allowed = (np.abs(A) * m["bound"][j]).sum() + rhs
        dev = abs((A * G).sum() - want)
        print(name, form, mode, "site", j + 1, "sum A G", (A * G).sum(), "sum c W", want, "difference / allowed %.3e" % (dev / allowed))
        assert dev <= allowed
        assert allowed <= 1e-7 * abs(want)                       # (the identity, not its allowance, decides)


@pytest.mark.parametrize("chosen", ["own", "given"])
@pytest.mark.parametrize("name,form", lc.CASE_FORMS)
def test_responses_give_back_the_weight_at_every_site(name, form, chosen):
    """multilinearity: the image's own feature at site j on resp[n, j] is the weight of the chosen label, at every j; and the response
    model's weights are the gradient model's within the weight bound"""
    r, m = lc.response_model(name, form, chosen), lc.model(name, form, "coef")
    f = lc.feats(name, form)
    rows = np.arange(len(f))
    ratio_w = lc.worst(r["w"] - m["w"], m["w_bound"])
    assert ratio_w <= 1.
    if chosen == "own":
        assert np.array_equal(r["label"], lc.pred_of(name, m["w"]) if lc.case(name)["target"] is None else np.zeros(len(f), dtype=np.int32))
    tie = (f * r["resp"]).sum(axis=2)                                               # [n, N]
    allowed = (np.abs(f) * r["bound"]).sum(axis=2) + 2 * rm.U * np.abs(f * r["resp"]).sum(axis=2) + m["w_bound"][rows, r["label"]][:, None]
    ratio = lc.worst(tie - r["w"][rows, r["label"]][:, None], allowed)
    rel = float((r["bound"].max(axis=(0, 2)) / np.abs(r["resp"]).max(axis=(0, 2))).max())
    print(name, form, chosen, "weights of the two models: worst / bound %.3e; tie: worst / allowed %.3e; worst bound / max|resp_j| %.3e" % (ratio_w, ratio, rel))
    assert ratio <= 1.
    assert rel <= 1e-8                                                              # the response bound has teeth as well


@pytest.mark.parametrize("name,form", lc.CASE_FORMS)
def test_fp32_model_stays_inside_half_the_decision_gap(name, form):
    """the bound of tests/test_chain32_model_host.py at these lengths: every image's fp32 weights are closer to the fp64 ones than half
    its decision gap, so the predictions agree"""
    w = lc.model(name, form, "coef")["w"]
    w32, p32 = lc.f32_model(name, form)
    dist = np.abs(w32 - w).max(axis=1)
    gap = lc.decision_gap(name, w)
    print(name, form, "relmax(fp32 model, fp64 model) %.3e, largest distance / half gap %.3e" % (dist.max() / np.abs(w).max(), (dist / (0.5 * gap)).max()))
    assert (dist < 0.5 * gap).all()
    assert np.array_equal(p32, lc.pred_of(name, w))
    assert np.array_equal(w32, w32.astype(np.float32).astype(np.float64)) and not np.array_equal(w32, w)


def _square_site(dims):
    """the first site (0-based) whose two bonds are equal, at least ten sites right of the middle of the chain, or None"""
    N = len(dims) - 1
    return next((j for j in range(N // 2 + 10, N - 10) if dims[j] == dims[j + 1]), None)


def _twin_sites(dims):
    """the first site j (0-based, away from the Label site) whose right neighbour has its shape, or None"""
    c = (len(dims) - 1) // 2 - 1
    return next((j for j in range(2, len(dims) - 4) if dims[j] == dims[j + 1] == dims[j + 2] and c not in (j, j + 1)), None)


def _planted(name, form, defect):
    """the labels-mode gradient with the defect planted -> (list of gradients, the sites to compare)"""
    d, f = lc.case(name), lc.feats(name, form)
    N = len(d["W"])
    every = range(N)
    kw = dict(labels=d["labels"], target_label=d["target"])
    if defect in SHORT:
        return sm.site_gradient(d["W"], f, defect=defect, **kw)[0], every
    if defect.startswith("swapped_neighbours"):             # the features of sites 5 / 6, or of N - 6 / N - 5 (1-based), change places
        g = f.copy()
        a = 4 if defect.endswith("5_6") else N - 7
        g[:, [a, a + 1]] = f[:, [a + 1, a]]
        return sm.site_gradient(d["W"], g, **kw)[0], every
    if defect == "skipped_site":                            # the walk passes a site with ml = mr by: its matrix is the identity
        j = _square_site(d["dims"])
        W = list(d["W"])
        W[j] = np.stack([np.eye(d["dims"][j]), np.zeros((d["dims"][j],) * 2)], axis=1)
        g = f.copy()
        g[:, j] = (1., 0.)
        return sm.site_gradient(W, g, **kw)[0], [k for k in every if k != j]
    assert defect == "shifted_gradient"                     # G_j lands on site j + 1 and the other way round
    j = _twin_sites(d["dims"])
    g = list(lc.model(name, form, "labels")["g"])
    g[j], g[j + 1] = g[j + 1], g[j]
    return g, every


def test_every_case_can_carry_every_defect():
    """two sites of one shape side by side need three equal bonds in a row, a site the walk can skip two: the seeds of the cases are
    chosen so that every list of bonds has them (bonds 3..130 seldom do)"""
    for name in lc.CASES:
        dims = lc.dims_of(name)
        assert _twin_sites(dims) is not None, name
        assert _square_site(dims) is not None, name


@pytest.mark.parametrize("defect", SHORT + LONG)
@pytest.mark.parametrize("name,form", lc.CASE_FORMS)
def test_planted_defects_land_ten_bounds_away(name, form, defect):
    m = lc.model(name, form, "labels")
    got, sites = _planted(name, form, defect)
    ratio = sm.worst_ratio([got[j] for j in sites], [m["g"][j] for j in sites], [m["bound"][j] for j in sites])
    print(name, form, defect, "worst error / bound %.3e" % ratio)
    assert ratio >= 10.
