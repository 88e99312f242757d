"""tests/eval_model.py, the numpy restatement of tnml_eval_report, against the CPU oracle: the oracle's toverlap gives the weights, its
own quadcost on the same W gives cost, per-label cost and #correct.  No GPU."""
import math

import numpy as np
import pytest

import eval_model
from conftest import make_problem

N, NT, M = 12, 70, 4
C_TOL = 1e-11                        # between two contraction orders of the same W (the fp64 "costs" tolerance of the parity tests)


@pytest.fixture(scope="module")
def problem():
    from oracle import pyoracle
    pixels, labels, phi, W = make_problem(N, NT, M, 3, pixel_boost=200.0)
    o = pyoracle.Oracle(phi, labels, W)
    w = np.stack([o.toverlap(i) for i in range(NT)])
    o.init()
    o.set_bond(1)
    cost, label_cost, reg, ncorrect = o.quadcost(o.bond_tensor(1), 0.0)
    return np.asarray(labels), w, dict(cost=cost, label_cost=label_cost, ncorrect=ncorrect)


def test_integers_are_the_oracles(problem):
    labels, w, orc = problem
    r = eval_model.report(w, labels)
    assert r["n"] == NT and r["ncorrect"] == orc["ncorrect"]
    assert np.array_equal(r["count"], np.bincount(labels, minlength=10))
    pred = np.abs(w).argmax(axis=1)
    assert np.array_equal(r["nincorrect"], [int(((labels == l) & (pred != l)).sum()) for l in range(10)])
    for t in range(10):
        for p in range(10):
            assert r["confusion"][t, p] == int(((labels == t) & (pred == p)).sum())
    assert r["confusion"].sum() == NT and np.array_equal(r["confusion"].sum(axis=1), r["count"])
    assert np.trace(r["confusion"]) == r["ncorrect"] == NT - r["nincorrect"].sum()


def test_cost_is_the_oracles(problem):
    labels, w, orc = problem
    r = eval_model.report(w, labels)
    print("cost", r["cost"], "oracle", orc["cost"], "rel", abs(r["cost"] - orc["cost"]) / orc["cost"])
    assert abs(r["cost"] - orc["cost"]) <= C_TOL * orc["cost"]
    np.testing.assert_allclose(r["label_cost"], orc["label_cost"], rtol=C_TOL, atol=C_TOL * orc["cost"])
    terms = ((w - np.eye(10)[labels]) ** 2).ravel().tolist()
    bound = eval_model.cost_bound(NT, 10)
    assert abs(r["cost"] - math.fsum(terms)) <= bound * math.fsum(terms)
    assert abs(sum(r["label_cost"].tolist()) - math.fsum(terms)) <= bound * math.fsum(terms)


@pytest.mark.parametrize("chunk", [8192, 16, 37])
def test_the_device_summation_order_stays_inside_the_bound(problem, chunk):
    labels, w, _ = problem
    r = eval_model.report(w, labels)
    lc = eval_model.device_order_label_cost(w, labels, chunk=chunk)
    bound = eval_model.cost_bound(NT, 10)
    assert np.all(np.abs(lc - r["label_cost"]) <= bound * r["label_cost"])
    assert abs(sum(lc.tolist()) - r["cost"]) <= bound * r["cost"]


def test_per_label_variant(problem):
    labels, w, _ = problem
    f = w[:, 3:4] - np.median(w[:, 3]) + 0.5                    # any scalar output with values on both sides of 1/2
    r = eval_model.report(f, labels, target=3)
    pred = (f[:, 0] > 0.5).astype(int)
    assert 0 < pred.sum() < NT
    assert r["ncorrect"] == int((pred == (labels == 3)).sum())
    assert not r["confusion"][:, 2:].any() and r["confusion"].sum() == NT
    per = (f[:, 0] - (labels == 3)) ** 2
    np.testing.assert_allclose(r["label_cost"], [per[labels == l].sum() for l in range(10)], rtol=1e-14)
    lc = eval_model.device_order_label_cost(f, labels, target=3, chunk=16)
    assert np.all(np.abs(lc - r["label_cost"]) <= eval_model.cost_bound(NT, 1) * r["label_cost"])


def test_empty_report():
    r = eval_model.report(np.zeros((0, 10)), np.zeros(0, dtype=np.int32))
    assert r["n"] == 0 and r["ncorrect"] == 0 and r["cost"] == 0.0 and not r["confusion"].any() and not r["label_cost"].any()
