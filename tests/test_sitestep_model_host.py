"""tests/sitestep_model.py, the yardstick of tests/test_sitestep_gpu.py, checked on the host: its SGD is descent_step's expression, its
ordered norm is a sum of squares within the bound of its own addition count, clipping clips, its Adam is torch.optim.Adam within a
bound derived from the operation counts of the two formulations, and twenty Adam steps on the model gradient of
tests/sitegrad_model.py halve the cost.  No GPU."""
import math

import numpy as np
import pytest

import sitegrad_model as sm
import sitestep_model as st


def _random_sites(rng, shapes):
    return [np.asfortranarray(rng.standard_normal(s)) for s in shapes]


SHAPES = [(1, 2, 3), (3, 2, 5, 10), (5, 2, 4), (4, 2, 1)]


def test_plain_sgd_is_descent_steps_expression():
    """mu = 0, clip = 0, scale = 1: A - lr * g elementwise, bit for bit, what TrainStates.descent_step sets"""
    rng = np.random.default_rng(1)
    W, G = _random_sites(rng, SHAPES), _random_sites(rng, SHAPES)
    E = st.flat(W).size
    for lr in (1e-2, 0.3, 1.7):
        new, state, rep = st.step(W, st.flat(G), st.new_state("sgd", E), method="sgd", lr=lr)
        assert all(np.array_equal(a, A - lr * g) for a, A, g in zip(new, W, G))
        assert rep["factor"] == 1. and not rep["clipped"] and rep["applied"] and rep["t"] == 1
        assert np.array_equal(state["v"], st.flat(G))
    # momentum: the second step carries the first
    s1 = st.step(W, st.flat(G), st.new_state("sgd", E), method="sgd", lr=0.1, momentum=0.9)
    s2 = st.step(s1[0], st.flat(G), s1[1], method="sgd", lr=0.1, momentum=0.9)
    v2 = 0.9 * st.flat(G) + st.flat(G)
    assert np.array_equal(s2[1]["v"], v2) and np.array_equal(st.flat(s2[0]), st.flat(s1[0]) - 0.1 * v2) and s2[2]["t"] == 2


@pytest.mark.parametrize("E", [1, 255, 65536, 3 * 65536 + 12345])
def test_ordered_norm_against_fsum(E):
    """several blocks, the last one ragged; less than one block; exactly one"""
    g = np.random.default_rng(E).standard_normal(E) * 10.0 ** np.random.default_rng(E + 1).integers(-3, 4, size=E)
    exact = math.fsum((g * g).tolist())
    total = st.ordered_sumsq(g)
    print("E", E, "relative difference", abs(total - exact) / exact, "bound", st.norm_bound(E))
    assert abs(total - exact) <= st.norm_bound(E) * exact
    assert total != 0
    norm, f, clipped = st.factor(total, -0.5, 0.)
    assert norm == 0.5 * np.sqrt(total) and f == -0.5 and not clipped


def test_norm_order_is_the_documented_one():
    """a planted defect: the same squares summed in plain index order give other bits on a long array (so the order is being tested),
    and one block's sum does not depend on what follows it"""
    g = np.random.default_rng(5).standard_normal(2 * 65536 + 77)
    plain = 0.
    for x in (g * g).tolist():
        plain += x
    assert st.ordered_sumsq(g) != plain
    # by hand on a tiny array: elements t and t + 256 meet in partial sum t, then the tree
    h = np.arange(1., 601.)
    part = np.zeros(256)
    for i, x in enumerate(h):
        part[i % 256] += x * x
    stride = 128
    while stride:
        part[:stride] += part[stride:2 * stride]
        stride //= 2
    assert st.ordered_sumsq(h) == part[0]


def test_clipped_step_keeps_the_norm_below_clip():
    rng = np.random.default_rng(2)
    W, G = _random_sites(rng, SHAPES), _random_sites(rng, SHAPES)
    g = np.concatenate([st.flat(G)] * 900)                      # more than one block
    W9 = [np.asfortranarray(rng.standard_normal(g.size))]
    raw = math.sqrt(math.fsum((g * g).tolist()))
    for scale, clip in ((1., raw / 3), (1. / 7, raw / 50), (-2., raw)):
        new, state, rep = st.step(W9, g, st.new_state("sgd", g.size), method="sgd", lr=1., clip=clip, scale=scale)
        assert rep["clipped"] and abs(rep["factor"]) < abs(scale)
        gh = state["v"]                                         # mu = 0: v is the scaled, clipped gradient
        got = math.sqrt(math.fsum((gh * gh).tolist()))
        # sqrt(total) is off by gamma / 2 and a rounding, its product with |scale| by one more; clip / grad_norm and the product
        # with scale are two; every fl(f g) one; this check's own squares, fsum and root three: gamma / 2 + 8 u
        slack = st.norm_bound(g.size) / 2 + 8 * st.U
        print("clip", clip, "norm after", got, "relative excess", got / clip - 1, "allowed", slack)
        assert got <= clip * (1 + slack)
        assert got >= clip * (1 - slack)
    new, state, rep = st.step(W9, g, st.new_state("sgd", g.size), method="sgd", lr=1., clip=2 * raw)
    assert not rep["clipped"] and rep["factor"] == 1.


def test_a_gradient_out_of_range_applies_nothing():
    rng = np.random.default_rng(3)
    W = _random_sites(rng, SHAPES)
    g = st.flat(_random_sites(rng, SHAPES))
    state = st.step(W, g, st.new_state("adam", g.size), method="adam", lr=0.1)[1]
    for bad in (1e200, np.inf, np.nan):
        gb = g.copy()
        gb[17] = bad
        new, after, rep = st.step(W, gb, state, method="adam", lr=0.1)
        assert not rep["applied"] and rep["t"] == 1 and after is state
        assert all(np.array_equal(a, b) for a, b in zip(new, W))


def test_five_adam_steps_against_torch():
    """torch.optim.Adam (CPU, fp64) on the same five gradients: inside AdamBound, which is derived in sitestep_model.py from the
    operation counts of the two formulations; and the bound has teeth: a model without bias correction is far outside it"""
    import torch
    rng = np.random.default_rng(4)
    W = _random_sites(rng, SHAPES)
    E = st.flat(W).size
    grads = [rng.standard_normal(E) * 10.0 ** rng.integers(-4, 3, size=E) for _ in range(5)]
    grads[2][::7] = 0.                                          # zeros, and an element that is zero throughout
    for g in grads:
        g[5] = 0.
    for lr, b1, b2, eps in ((1e-2, .9, .999, 1e-8), (0.3, .5, .9, 1e-3)):
        p = torch.tensor(st.flat(W), dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
        state, Wm, bound = st.new_state("adam", E), W, st.AdamBound(E)
        worst = 0.
        for g in grads:
            p.grad = torch.tensor(g, dtype=torch.float64)
            opt.step()
            prev = state
            Wm, state, rep = st.step(Wm, g, state, method="adam", lr=lr, beta1=b1, beta2=b2, eps=eps)
            allowed = bound.after_step(Wm, g, prev["m"], prev["v"], state, lr, b1, b2, eps)
            d = np.abs(st.flat(Wm) - p.detach().numpy())
            assert (d <= allowed).all(), (rep["t"], float((d / allowed).max()))
            worst = max(worst, float((d[allowed > 0] / allowed[allowed > 0]).max()))
        print("lr", lr, "worst |difference| / bound over five steps", worst, "largest bound", float(allowed.max()))
        assert np.abs(st.flat(Wm) - st.flat(W)).max() > 1e3 * allowed.max()      # the steps are many orders above the bound
        # planted defect: no bias correction (c1 = c2 = 1) -- far outside
        m = v = np.zeros(E)
        A = st.flat(W)
        for g in grads:
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            A = A - lr * m / (np.sqrt(v) + eps)
        assert not (np.abs(A - p.detach().numpy()) <= allowed).all()


def test_twenty_adam_steps_halve_the_cost():
    """the model's Adam on the model's gradient: DESCENT's lr is the one tests/test_sitestep_gpu.py takes to the device"""
    d = st.DESCENT
    case = sm.small_case(*d["case"])
    phi, labels = case["phi"][:d["images"]], case["labels"][:d["images"]]
    W = [np.array(A) for A in case["W"]]
    state = st.new_state("adam", st.flat(W).size)
    costs = [st.cost(W, phi, labels)]
    for _ in range(d["steps"]):
        g, _ = sm.site_gradient(W, phi, labels=labels)
        W, state, rep = st.step(W, st.flat(g), state, method="adam", lr=d["lr"])
        assert rep["applied"]
        costs.append(st.cost(W, phi, labels))
    print("cost / start", [round(c / costs[0], 3) for c in costs])
    assert state["t"] == d["steps"] and costs[-1] < 0.5 * costs[0]
