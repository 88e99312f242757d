"""tests/response_model.py against the oracle: the model's site responses are the oracle's full contraction (toverlap; the per-label
variant's output) of the image with one site's feature replaced by a unit vector.  No GPU."""
import numpy as np
import pytest

from conftest import make_problem
from response_model import response

TOL = 1e-12


def _replaced(phi, j, s):
    out = phi.copy()
    out[:, j, :] = 0.
    out[:, j, s] = 1.
    return out


@pytest.mark.parametrize("N", [6, 12])
@pytest.mark.parametrize("chosen", ["own", "given"])
def test_model_is_the_oracle_with_one_feature_replaced(N, chosen):
    from oracle import pyoracle
    pixels, labels, phi, W = make_problem(N, 20, 4, 3, pixel_boost=200.0)
    which = None if chosen == "own" else np.random.default_rng(N).integers(0, 10, size=20)
    resp, weights, label = response(W, phi, which)
    rows = np.arange(20)
    truth_w = np.stack([pyoracle.Oracle(phi, labels, W).toverlap(i) for i in range(20)])
    assert np.abs(weights - truth_w).max() <= TOL * np.abs(truth_w).max()
    if which is None:
        np.testing.assert_array_equal(label, np.abs(truth_w).argmax(axis=1))
    else:
        np.testing.assert_array_equal(label, which)
    for j in range(N):
        truth = np.zeros((20, 2))
        for s in range(2):
            o = pyoracle.Oracle(_replaced(phi, j, s), labels, W)
            truth[:, s] = [o.toverlap(i)[label[i]] for i in range(20)]
        assert np.abs(resp[:, j] - truth).max() <= TOL * np.abs(truth).max(), j
        # the identity: the image's own feature at site j gives back its output
        ident = (phi[:, j] * resp[:, j]).sum(axis=1)
        assert np.abs(ident - truth_w[rows, label]).max() <= TOL * np.abs(truth_w).max(), j


@pytest.mark.parametrize("N", [6, 12])
def test_model_per_label_variant_is_the_single_oracle(N):
    from oracle import pyoracle
    from tnml_amd import synth
    NT, m = 20, 4
    labels = synth.synthetic_labels(NT, seed=3, per_label=NT // 10)
    pixels = synth.synthetic_images(N, labels, seed=3)
    phi = pyoracle.features_single(pixels, True).copy()
    phi[..., 1] *= 300.0
    W = synth.random_mps(N, m, seed=10)
    W[N // 2 - 1] = W[N // 2 - 1][..., 0] * 3.0                 # plain MPS: no Label index
    resp, weights, label = response(W, phi)
    assert weights.shape == (NT, 1) and not label.any()
    out = np.array([pyoracle.SingleOracle(phi, labels, 3, W).output(i) for i in range(NT)])
    assert np.abs(weights[:, 0] - out).max() <= TOL * np.abs(out).max()
    for j in range(N):
        truth = np.zeros((NT, 2))
        for s in range(2):
            o = pyoracle.SingleOracle(_replaced(phi, j, s), labels, 3, W)
            truth[:, s] = [o.output(i) for i in range(NT)]
        assert np.abs(resp[:, j] - truth).max() <= TOL * np.abs(truth).max(), j
        assert np.abs((phi[:, j] * resp[:, j]).sum(axis=1) - out).max() <= TOL * np.abs(out).max(), j
    with pytest.raises(AssertionError):
        response(W, phi, np.ones(NT, dtype=np.int32))           # one output only
