"""tests/grad32_model.py proved on the host: its weights and pred are chain32_model.predict32's bit for bit, its G and dphi lie within the
derived fp32 bound of the fp64 models (sitegrad_model.py, inputgrad_model.py) on the same inputs, the Euler identity and the tie
sum_s phi dphi = sum_l c W hold within the same bound, and each planted defect changes bits (the structural one leaves the bound by
more than a factor of 10).  No GPU."""
import numpy as np
import pytest

import chain32_cases as cases
import chain32_model as cm
import grad32_model as gm
import inputgrad_model as im
import sitegrad_model as sm

# (kind, key, form, mode): the three small problems in both modes, one (form, mode) pair per list of bond dimensions
SMALL = [("small", k, form, mode) for k in cases.SMALL for form, mode in (("phi", "labels"), ("u8", "coef"))]
LISTS = [("dims", 0, "phi", "labels"), ("dims", 1, "u8", "coef"), ("dims", 2, "u8", "labels"), ("dims", 3, "phi", "coef"), ("1024", 0, "phi", "labels")]


def _kw(d, mode):
    return dict(labels=d["labels"]) if mode == "labels" else dict(coef=d["coef"])


@pytest.mark.parametrize("kind,key,form,mode", SMALL + LISTS)
def test_model_against_the_fp64_models(kind, key, form, mode):
    d = gm.case(kind, key)
    W, f = d["W"], d["forms"][form]
    r = gm.model(kind, key, form, mode)
    wm, pm = cm.predict32(W, f)
    assert np.array_equal(r["weights"], wm) and np.array_equal(r["pred"], pm)        # phase A is the chain model, bit for bit
    assert np.array_equal(r["coef"], cm.fl32(r["coef"]))
    kw = _kw(d, mode)
    g64, w64 = sm.site_gradient(W, f, **kw)
    d64, _ = im.input_gradient(W, f, **kw)
    bg, bd, bw = gm.bound_grads(W, f, **kw), gm.bound_dphi(W, f, **kw), gm.weight_bound(W, f)
    rg, rd = sm.worst_ratio(r["grads"], g64, bg), im.worst_ratio(r["dphi"], d64, bd)
    scale = max(np.abs(g).max() for g in g64)
    relg = max(np.abs(a - b).max() for a, b in zip(r["grads"], g64)) / scale
    print("G: worst deviation / bound %.3g, relmax %.3g; dphi: %.3g, relmax %.3g" % (rg, relg, rd, np.abs(r["dphi"] - d64).max() / np.abs(d64).max()))
    assert rg <= 1. and rd <= 1.
    assert any((a != b).any() for a, b in zip(r["grads"], g64)) and (r["dphi"] != d64).any()      # fp32 it is
    assert np.array_equal(r["dphi"], cm.fl32(r["dphi"]))                                          # every dphi value is an fp32
    # Euler: W is linear in every site tensor; the tie: and in every site's feature
    c = r["coef"]
    want = (c * r["weights"]).sum()
    slack = (np.abs(c) * bw).sum()
    for j in range(len(W)):
        got = (W[j] * r["grads"][j]).sum()
        allowed = (np.abs(W[j]) * bg[j]).sum() + slack
        assert abs(got - want) <= allowed, (j, got, want, allowed)
    tie = (f * r["dphi"]).sum(axis=2)                                                             # [n, N]
    per_image = (c * r["weights"]).sum(axis=1)
    allowed = (np.abs(f) * bd).sum(axis=2) + (np.abs(c) * bw).sum(axis=1)[:, None]
    assert (np.abs(tie - per_image[:, None]) <= allowed).all()
    if mode == "coef":       # the checks have teeth (labels: c carries the weight's error on absolute values, which the boosted features make large)
        assert (allowed < 0.2 * (np.abs(c) * sm.abs_gradient(W, f, coef=np.abs(c))[1]).sum(axis=1)[:, None]).all()


@pytest.mark.parametrize("defect", gm.DEFECTS)
def test_planted_defects_change_bits(defect):
    """on the first small problem, 70 images in chunks of 64 and 6 as the GPU test runs them"""
    kind, key = "small", cases.SMALL[0]
    d = gm.case(kind, key)
    W, f = d["W"], d["forms"]["phi"]
    good = gm.model(kind, key, "phi", "labels", 64)
    bad = gm.backward32(W, f, labels=d["labels"], chunk=64, defect=defect)
    changed = sum(int((a != b).sum()) for a, b in zip(good["grads"], bad["grads"])) + int((good["dphi"] != bad["dphi"]).sum())
    print(defect, "changes", changed, "values")
    assert changed > 0
    if defect == "f64_rowmap":                                                       # structural: not a matter of rounding
        g64, _ = sm.site_gradient(W, f, labels=d["labels"])
        assert sm.worst_ratio(bad["grads"], g64, gm.bound_grads(W, f, labels=d["labels"])) > 10.
    assert np.array_equal(good["weights"], bad["weights"])


def test_chunks_add_up_in_fp64_and_dphi_ignores_them():
    kind, key = "small", cases.SMALL[2]
    d = gm.case(kind, key)
    W, f = d["W"], d["forms"]["u8"]
    one = gm.backward32(W, f, coef=d["coef"], chunk=512)
    two = gm.backward32(W, f, coef=d["coef"], chunk=64)
    assert np.array_equal(one["dphi"], two["dphi"])
    assert any((a != b).any() for a, b in zip(one["grads"], two["grads"]))
    a = gm.backward32(W, f[:64], coef=d["coef"][:64], want_dphi=False)["grads"]
    b = gm.backward32(W, f[64:], coef=d["coef"][64:], want_dphi=False)["grads"]
    assert all(np.array_equal(x + y, z) for x, y, z in zip(a, b, two["grads"]))      # one fp64 addition per element and chunk


def test_per_label_variant_and_softmax():
    phi, W, _ = cases.per_label_problem()
    labels = (np.arange(len(phi)) % 10).astype(np.int32)
    r = gm.backward32(W, phi, labels=labels, target_label=3)
    wm, pm = cm.predict32(W, phi, single=True)
    assert np.array_equal(r["weights"], wm) and np.array_equal(r["pred"], pm)
    g64, _ = sm.site_gradient(W, phi, labels=labels, target_label=3)
    assert sm.worst_ratio(r["grads"], g64, gm.bound_grads(W, phi, labels=labels, target_label=3)) <= 1.
    d64, _ = im.input_gradient(W, phi, labels=labels, target_label=3)
    assert im.worst_ratio(r["dphi"], d64, gm.bound_dphi(W, phi, labels=labels, target_label=3)) <= 1.
    import loss_model
    d = gm.case("small", cases.SMALL[0])
    f = d["forms"]["phi"]
    s = gm.backward32(d["W"], f, labels=d["labels"], loss="softmax", beta=2.5)
    assert np.array_equal(s["coef"], cm.fl32(loss_model.coefficients(s["weights"], d["labels"], 2.5)))
    g64, _ = sm.site_gradient(d["W"], f, coef=s["coef"])                             # the fp64 gradient for the very coefficients the model used
    assert sm.worst_ratio(s["grads"], g64, gm.bound_grads(d["W"], f, coef=s["coef"])) <= 1.


def test_the_fast_fma_is_the_fma():
    """random operands, and a family crafted so that fl64(a b + c) lies exactly half way between two fp32 numbers with the exact value
    beside it (towards zero for positive c, away from it for negative c)"""
    rng = np.random.default_rng(3)
    a, b = cm.fl32(rng.standard_normal(20000)), cm.fl32(rng.standard_normal(20000))
    c = cm.fl32(rng.standard_normal(20000) * 10.0 ** rng.integers(-9, 3, 20000))
    assert np.array_equal(gm.fma32_fast(a, b, c), cm.fma32(a, b, c))
    k = np.arange(1, 4001, dtype=np.float64)
    c = (1.0 + 2.0 ** -23 * k) * np.where(k % 3 == 0, -1.0, 1.0)  # fp32 numbers in [1, 2), either sign
    a = 2.0 ** -12 * (1.0 + 2.0 ** -20) + np.zeros_like(k)      # a b = 2^-24 (1 - 2^-40) exactly: the fp64 sum drops the 2^-64 and lands on
    b = 2.0 ** -12 * (1.0 - 2.0 ** -20) + np.zeros_like(k)      # c + 2^-24, half way between two fp32 numbers; the exact value lies inside
    assert np.array_equal(a, cm.fl32(a)) and np.array_equal(b, cm.fl32(b))
    got, want = gm.fma32_fast(a, b, c), cm.fma32(a, b, c)
    assert np.array_equal(got, want)
    half = (a * b + c).view(np.int64) & 0x1FFFFFFF
    assert (half == 0x10000000).sum() > 1000
    assert (want != cm.fma32_plain(a, b, c)).sum() > 500         # the family bites: rounding the fp64 sum alone gets these wrong
    tiny32 = cm.fl32(2.0 ** -70 + np.zeros(8))                   # results in the fp32 subnormals take the slow path whole
    assert np.array_equal(gm.fma32_fast(tiny32, tiny32, 0.0), cm.fma32(tiny32, tiny32, 0.0))
