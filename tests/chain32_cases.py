"""The inputs the fp32 streamed-inference tests share (test_chain32_model_host.py, test_predict_f32_gpu.py): the problems of
test_predict_gpu.py plus a list of bond dimensions that reaches 1 024, each with the oracle's fp64 weights and the fp32 model's weights,
computed once per process."""
import functools

import numpy as np

import chain32_model as cm
from conftest import make_problem

# the four lists of test_predict_gpu.py and one that reaches the fp32 kernel's upper bound (the Label site carries 1024 x 2 x 1023 x 10)
DIMS = [[1, 2, 3, 5, 9, 17, 33, 65, 120, 2, 1],
        [1, 2, 120, 97, 64, 60, 61, 128, 33, 2, 1],
        [1, 2, 4, 150, 129, 200, 300, 257, 16, 2, 1],
        [1, 2, 16, 512, 511, 130, 64, 2, 1],
        [1, 2, 16, 1024, 1023, 513, 64, 2, 1]]
SMALL = [(12, 4), (4, 2), (17, 6)]
FORMS = ("phi", "u8")


def mps_with_dims(dims, seed):
    """random weight MPS with the given bond dimensions d_0 = 1, d_1, ..., d_N = 1 (Label index on site N/2), any shapes"""
    rng = np.random.default_rng(seed)
    N = len(dims) - 1
    W = []
    for j in range(1, N + 1):
        ml, mr = dims[j - 1], dims[j]
        shape = (ml, 2, mr, 10) if j == N // 2 else (ml, 2, mr)
        A = rng.standard_normal(shape) / np.sqrt(2. * max(ml, mr) * (10 if j == N // 2 else 1))
        A[:, 0] += (np.eye(ml, mr) if A.ndim == 3 else np.eye(ml, mr)[:, :, None] / np.sqrt(10.))
        W.append(A)
    return W


def toverlap(phi, W):
    from oracle import pyoracle
    o = pyoracle.Oracle(phi, np.zeros(len(phi), dtype=np.int32), W)
    return np.stack([o.toverlap(i) for i in range(len(phi))])


@functools.lru_cache(maxsize=None)
def inputs(kind, key):
    """(pixels, {"phi": fp64 features given, "u8": fp64 features of the byte expression}, W): kind "small" with key (N, m): 70 images;
    kind "dims" with key k: 40 images on DIMS[k], 8 on the list that reaches 1 024"""
    if kind == "small":
        N, m = key
        pixels, _, phi, W = make_problem(N, 70, m, 3, pixel_boost=200.0)
    else:
        dims = DIMS[key]
        N = len(dims) - 1
        pixels, _, phi, _ = make_problem(N, 40, 2, 5, pixel_boost=200.0)
        if max(dims) > 512:
            pixels, phi = pixels[:8], phi[:8]
        W = mps_with_dims(dims, 11)
    return pixels, {"phi": phi, "u8": cm.features_u8(pixels)}, W


@functools.lru_cache(maxsize=None)
def oracle(kind, key, form):
    _, f, W = inputs(kind, key)
    return toverlap(f[form], W)


@functools.lru_cache(maxsize=None)
def model(kind, key, form):
    """(weights, pred) of the fp32 model"""
    _, f, W = inputs(kind, key)
    return cm.predict32(W, f[form])


ALL = [("small", k) for k in SMALL] + [("dims", k) for k in range(len(DIMS))]


def per_label_problem():
    """the set-up of test_predict_per_label_variant: (phi, W, f) with f the fp64 decision function"""
    from oracle import pyoracle
    from tnml_amd import synth
    N, NT, m = 12, 60, 4
    labels = synth.synthetic_labels(NT, seed=3, per_label=NT // 10)
    pixels = synth.synthetic_images(N, labels, seed=3)
    phi = pyoracle.features_single(pixels, True).copy()
    phi[..., 1] *= 300.0
    W = synth.random_mps(N, m, seed=10)
    W[N // 2 - 1] = W[N // 2 - 1][..., 0] * 3.0            # plain MPS: no Label index
    f = np.ones((NT, 1))
    for j, A in enumerate(W):
        f = np.einsum("na,nab->nb", f, np.einsum("ns,asb->nab", phi[:, j, :], A))
    return phi, W, f
