"""Shared by tests/test_mps_algebra_host.py and tests/test_mps_algebra_gpu.py: seeded Gaussian per-label weight MPS (the `W0..W9` a
`single` or `linear` run leaves), images with the normalised cos/sin features, and plain-numpy truth: part k's output on an image,
the label outputs of a summed network, dense tensors and their spectra.  Nothing here touches the device or the host library."""
import functools

import numpy as np

NL = 10


def make_parts(N, m, K=NL, seed=1):
    """K Label-free MPS of N sites and uniform bond m (1 at the chain ends), entries N(0,1)/sqrt(m)"""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(K):
        parts.append([rng.standard_normal((1 if j == 0 else m, 2, 1 if j == N - 1 else m)) / np.sqrt(m) for j in range(N)])
    return parts


def make_images(N, n, seed=2):
    """phi[n, N, 2] = [cos(pi/2 x), sin(pi/2 x)], x uniform in [0, 1]"""
    x = np.random.default_rng(seed).random((n, N))
    return np.stack([np.cos(np.pi / 2 * x), np.sin(np.pi / 2 * x)], axis=-1)


def part_outputs(parts, phi):
    """f[n, k] = part k contracted with image n"""
    out = np.empty((phi.shape[0], len(parts)))
    for k, P in enumerate(parts):
        E = np.ones((phi.shape[0], 1))
        for j, A in enumerate(P):
            E = np.einsum("na,asb,ns->nb", E, A, phi[:, j], optimize=True)
        out[:, k] = E[:, 0]
    return out


def label_outputs(W, phi):
    """out[n, l] = W_l(image n) for a weight MPS with the Label index on one site"""
    n = phi.shape[0]
    E = np.ones((n, 1, 1))                                  # [n, link, label]
    for j, A in enumerate(W):
        if A.ndim == 4:
            E = np.einsum("nax,asbl,ns->nbl", E, A, phi[:, j], optimize=True)
        else:
            E = np.einsum("nal,asb,ns->nbl", E, A, phi[:, j], optimize=True)
    return E[:, 0, :]


def check_outputs(W, parts, phi):
    """label component k of the network == part k's output: rtol 1e-5, atol 1e-6 max|f_k| (the W0..W9 test of tests/test_gpu_parity.py)"""
    out, f = label_outputs(W, phi), part_outputs(parts, phi)
    for k in range(len(parts)):
        np.testing.assert_allclose(out[:, k], f[:, k], rtol=1e-5, atol=1e-6 * np.abs(f[:, k]).max())


def dense_labelled(W):
    """T[s_1..s_N, l] of a weight MPS with the Label index on one site"""
    T = np.ones((1, 1, 1))                                  # [states, label, link]
    for A in W:
        if A.ndim == 4:
            T = np.einsum("xla,asbk->xskb", T, A).reshape(-1, A.shape[3], A.shape[2])
        else:
            T = np.einsum("xla,asb->xslb", T, A).reshape(-1, T.shape[1], A.shape[2])
    return T[:, :, 0]


def dense_sum(parts):
    """the exact sum of the parts, part k in label slot k: T[s_1..s_N, k]"""
    cols = []
    for P in parts:
        T = np.ones((1, 1))
        for A in P:
            T = np.einsum("xa,asb->xsb", T, A).reshape(-1, A.shape[2])
        cols.append(T[:, 0])
    return np.stack(cols, axis=1)


def bond_spectra(T, N):
    """for bond b = 1..N-1 of the dense T[2^N, 10] (Label index on site c0 = N/2): p = sigma^2 / sum, descending"""
    c0 = N // 2
    out = []
    for b in range(1, N):
        X = T.reshape(2 ** b, 2 ** (N - b), NL)
        M = X.transpose(0, 2, 1).reshape(2 ** b * NL, -1) if c0 <= b else X.reshape(2 ** b, -1)
        sv = np.linalg.svd(M, compute_uv=False)
        p = sv ** 2
        out.append(p / p.sum())
    return out


def generic_rank(N, m_sum):
    """bond dimensions of a sum of generic parts: min(direct-sum bond, states on the left, states on the right), the Label index on its side"""
    c0 = N // 2
    return [int(min(m_sum, 2 ** b * (NL if c0 <= b else 1), 2 ** (N - b) * (NL if c0 > b else 1))) for b in range(1, N)]


def bond_dims(W):
    return [A.shape[2] for A in W[:-1]]


def transfer_overlap(W):
    """<W|W> by the transfer chain in numpy"""
    E = np.ones((1, 1))
    for A in W:
        if A.ndim == 4:
            E = np.einsum("ab,asxl,bsyl->xy", E, A, A, optimize=True)
        else:
            E = np.einsum("ab,asx,bsy->xy", E, A, A, optimize=True)
    return float(E[0, 0])


@functools.lru_cache(maxsize=None)
def problem(N, m, seed=1, nimg=40):
    """(parts, phi) shared by the tests of one shape; treated as read-only"""
    return make_parts(N, m, seed=seed), make_images(N, nimg, seed=seed + 100)


def host_sum(parts, workdir, cutoff=1e-10, maxm=0, one_shot=True):
    """the host library's sum of the parts (files W0..W9 in workdir -> tnmlh_mps_sum) as a list of site tensors"""
    import os
    from tnml_amd import hostlib
    files = []
    for k, P in enumerate(parts):
        files.append(os.path.join(str(workdir), "W%d" % k))
        if not os.path.exists(files[-1]):
            hostlib.write_mps(files[-1], P)
    out = os.path.join(str(workdir), "Wsum_%d_%d" % (int(one_shot), int(maxm)))
    md = hostlib.mps_sum(files, out, cutoff=cutoff, maxm=maxm, one_shot=one_shot)
    W = hostlib.read_mps(out)
    assert md == max(bond_dims(W))
    return W
