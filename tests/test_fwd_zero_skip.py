"""The resident-operand forward pass with a tile's images walked zero features first (option "fwd_skip", k_fwd_res<.., ZS> in
kernels_res.hip): phi[1] is exactly 0 wherever a pixel is 0, the odd-row product of such an image is multiplied by zero in the epilogue,
and a 16-image group that holds only such images runs without its odd-row chain.  The products are per image, so the order inside a
32-image tile changes no value: every output must equal, value for value, what the same context computes in natural order with every
product."""
import functools
import os

import numpy as np
import pytest

N, NT, NTP = 12, 1100, 1280          # Label on site 6; 1 100 images pad to 1 280 = 40 tiles of 32: 34 full ones, 12 images + 20 padding, five of padding alone
# the two bond kinds k_fwd_res serves, both 120 x 120 here: bond 3 has the Label on its right environment (input feature: site 3), bond 8 on
# its left one (input feature: site 9)
BONDS = ((3, 3), (8, 9))             # (bond, site of the input feature)
# zero pixels of the feature sites in the full tiles 0..33, cyclically (site 9 starts four places on): every boundary of nz / 16 from both
# sides; the ragged tile 34 holds 12 real images beside 20 padding images (which store phi[1] = 0): site 3 none zero -> 20, site 9 all -> 32
PATTERN = (0, 1, 15, 16, 17, 31, 32, 8, 24)
RAGGED = {3: 0, 9: 12}


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _pixels():
    """synthetic images; the columns of the two feature sites carry the zero counts of PATTERN at positions scattered by a seeded generator"""
    from tnml_amd import synth
    labels = synth.synthetic_labels(NT, seed=5, per_label=NT // 10)
    pixels = synth.synthetic_images(N, labels, seed=5)
    rng = np.random.default_rng(20241020)
    for k, site in enumerate(s for _, s in BONDS):
        col = rng.integers(1, 256, size=NT).astype(np.uint8)
        for tile in range(NTP // 32):
            lo, hi = 32 * tile, min(32 * tile + 32, NT)
            if hi <= lo:
                continue
            nz = PATTERN[(tile + 4 * k) % len(PATTERN)] if hi - lo == 32 else RAGGED[site]
            col[lo + rng.permutation(hi - lo)[:nz]] = 0
        pixels[:, site - 1] = col
    return pixels, labels


def _tile_zero_counts(pixels):
    """[tiles][sites]: zero features per 32-image tile, padding images included"""
    z = np.ones((NTP, pixels.shape[1]), dtype=bool)
    z[:NT] = pixels == 0
    return z.reshape(NTP // 32, 32, -1).sum(axis=1)


def _mps(m, seed):
    """every inner bond of dimension m (a chain this short cannot grow one: the kernel under test is the 120 x 120 form)"""
    rng = np.random.default_rng(seed)
    dims = [1] + [m] * (N - 1) + [1]
    W = []
    for j in range(1, N + 1):
        ml, mr = dims[j - 1], dims[j]
        shape = (ml, 2, mr) + ((10,) if j == N // 2 else ())
        A = rng.standard_normal(shape) / np.sqrt(max(ml, mr) * (10 if j == N // 2 else 1))
        A[:, 1] *= 0.5
        W.append(A)
    return W


@functools.lru_cache(maxsize=None)
def _problem(m):
    """pixels, labels, features, the MPS and per bond under test (a bond tensor, the oracle's forward outputs for it): computed once, read only"""
    from oracle import pyoracle
    from tnml_amd import synth
    pixels, labels = _pixels()
    phi = synth.features_series(pixels)
    phi[..., 1] *= 200.0
    W = _mps(m, 100 + m)
    o = pyoracle.Oracle(phi, labels, W, nthread=min(8, os.cpu_count() or 1))
    o.init()
    rng = np.random.default_rng(3)
    Bs, at = {}, 1
    for b, _ in BONDS:
        for bb in range(at, b):
            o.shiftE(bb, True)
        at = b
        o.set_bond(b)
        B = o.bond_tensor(b)
        assert B.shape[:4] == (m, 2, 2, m)
        B = B + 0.05 * rng.standard_normal(B.shape)
        Bs[b] = (B, o.forward(B))
    return pixels, labels, phi, W, Bs


def test_tile_counts_of_the_pixels_under_test():
    """the pixel columns of both feature sites really put the zero counts of the 32-image tiles on both sides of every multiple of 16"""
    pixels, _ = _pixels()
    nz = _tile_zero_counts(pixels)
    for _, site in BONDS:
        met = {int(v) for v in nz[:, site - 1]}
        assert {0, 1, 15, 16, 17, 31, 32} <= met, (site, sorted(met))
    assert int(nz[34, 2]) == 20 and int(nz[34, 8]) == 32 and (nz[35:] == 32).all()


def test_share_of_groups_without_odd_rows_on_the_benchmark_data():
    """what the option rests on: in the benchmark's synthetic images 0.3447 of all 16-image groups hold zero pixels only once every
    32-image tile is walked zero pixels first -- 17.2 % of the forward GEMM's MFMAs"""
    from tnml_amd import synth
    labels = synth.synthetic_labels(60000)
    z = synth.synthetic_images(784, labels) == 0
    nz = z.reshape(60000 // 32, 32, -1).sum(axis=1)
    share = (nz // 16).sum() / (60000 // 16 * 784)
    per_tile = [float(((nz // 16) == k).mean()) for k in range(3)]
    print("zero pixels %.4f; groups of zero pixels only, zero-first inside each 32-image tile: %.4f; tiles with 0 / 1 / 2 such groups: %.3f / %.3f / %.3f"
          % ((z.mean(), share) + tuple(per_tile)))
    assert abs(share - 0.3447) <= 0.005, share


@pytest.mark.gpu
@pytest.mark.parametrize("m,grid", [(120, 16), (120, 32)])
def test_zero_first_forward_equals_the_natural_order_and_the_oracle(m, grid):
    """m = 120: k_fwd_res<6, 3, 0, 30, false, 8, true>, the only form built with the flag.  The context pads 1 100 images to a multiple of
    256, so the launch walks 40 tiles: the last real tile is ragged, five are padding alone.  res_grid = 16: eight pairs of workgroups run
    five rounds each -- the order prefetch and both buffers; res_grid = 32: sixteen pairs, the first eight run three rounds, the others
    two -- a partial last round (tile counts are multiples of eight, so eight pairs always run the same number).  With fwd_skip = 1 against 0 on the same context (np.array_equal): the forward outputs of both
    bond kinds, the per-image states a CG leaves (Pp, P, dP) and one bond update; with fwd_skip = 1 against the oracle: the forward
    outputs (1e-11, as test_configs_at_shape.py asks of the forced k_fwd_res); and the accessor's group counts against the pixels'."""
    from tnml_amd.fixedl import TrainStates
    pixels, labels, phi, W, Bs = _problem(m)
    ts = TrainStates(labels, N, m, phi=phi)
    for k in ("fwd_res", "shift_res", "grad_quad"):
        ts.set_option(k, 2)
    ts.set_option("res_grid", grid)
    want = (_tile_zero_counts(pixels) // 16).sum(axis=0)
    for j in range(1, N + 1):
        assert ts.fwd_skip_stats(j) == (NTP // 16, int(want[j - 1])), j
    got = {}
    for skip in (1, 0):
        ts.set_option("fwd_skip", skip)
        ts.set_mps(W)
        ts.init()
        ts.profile(True, only="fwd_res")
        ts.profile_reset()
        out, at = {}, 1
        for b, _ in BONDS:
            for bb in range(at, b):
                ts.shiftE(bb, True)
            at = b
            ts.setBond(b)
            B = Bs[b][0]
            P = ts.forward(B)
            ts.cgrad(B, 3, 1e-3, 1e-10)
            out[b] = (P, {k: ts.cg_state(k) for k in ("Pp", "P", "dP")})
        rep = ts.bond_update(BONDS[-1][0], 1, m, m // 2, 1e-10, 3, 1e-3, 1e-10)
        ts.profile(False)
        assert ts.profile_read()["fwd_res"][0] > 0                    # the kernel under test really ran (fwd_res = 2 forces it)
        got[skip] = (out, rep)
    ts.close()
    for b, _ in BONDS:
        on, off = got[1][0][b], got[0][0][b]
        assert on[0].shape == (NT, 10)
        assert np.array_equal(on[0], off[0]), b
        for k in ("Pp", "P", "dP"):
            assert on[1][k].shape == (NTP, 10)
            assert np.array_equal(on[1][k], off[1][k]), (b, k)
        assert _rel(on[0], Bs[b][1]) < 1e-11, b
    ron, roff = got[1][1], got[0][1]
    for k in ("newm", "ncorrect", "cost", "truncerr"):
        assert ron[k] == roff[k], (k, ron[k], roff[k])
    assert ron["cg"]["cost"] == roff["cg"]["cost"] and ron["cg"]["alpha"] == roff["cg"]["alpha"]
