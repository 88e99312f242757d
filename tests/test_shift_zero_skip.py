"""The Label-carrying environment shift with a tile's images walked zero features first (option "shift_skip", kernels_res.hip):
phi[1] is exactly 0 wherever a pixel is 0, the odd-row product of such an image is multiplied by zero, and a 16-image group that holds
only such images runs without its odd-row MFMAs.  The products are per image, so the order inside a tile changes no value: every
environment must equal, value for value, what the same context computes in natural order with every product."""
import os

import numpy as np
import pytest

N, NT, NTP = 12, 150, 256            # Label on site 6; 150 images pad to 256 = four 64-image tiles: two full ones, 22 images + 42 padding, padding alone
RIGHT, LEFT = (5, 4, 3), (7, 8, 9, 10)   # sites absorbed by the Label-carrying shifts of init (right environments) and of shiftE (left ones)
# zero pixels per site in the image tiles 0, 1 and among the 22 real images of tile 2 (its 42 padding images store phi[1] = 0 as well):
# the zero counts of the tiles hit 0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63 and 64 -- every boundary of nz / 16 from both sides
ZEROS = {3: (64, 64, 22), 4: (0, 0, 0), 5: (1, 15, 5), 7: (16, 17, 6), 8: (31, 32, 7), 9: (33, 47, 21), 10: (48, 49, 22), 11: (63, 40, 11)}


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _pixels():
    """site 3 all zeros, site 4 all 255, the other sites of ZEROS with their zero counts at positions scattered by a seeded generator"""
    from tnml_amd import synth
    labels = synth.synthetic_labels(NT, seed=5, per_label=NT // 10)
    pixels = synth.synthetic_images(N, labels, seed=5)
    rng = np.random.default_rng(20240607)
    for site, counts in ZEROS.items():
        col = np.full(NT, 255, dtype=np.uint8) if site == 4 else rng.integers(1, 256, size=NT).astype(np.uint8)
        for tile, k in enumerate(counts):
            lo, hi = 64 * tile, min(64 * tile + 64, NT)
            col[lo + rng.permutation(hi - lo)[:k]] = 0
        pixels[:, site - 1] = col
    return pixels, labels


def _group_counts(pixels):
    """per site: 16-image groups of zero features only once each 64-image tile (padding included) is walked zero pixels first"""
    z = np.ones((NTP, pixels.shape[1]), dtype=bool)
    z[:NT] = pixels == 0
    return (z.reshape(NTP // 64, 64, -1).sum(axis=1) // 16).sum(axis=0)


def _mps(m, seed):
    """every inner bond of dimension m (a chain this short cannot grow one: the shifts under test need input dimensions from 33 on)"""
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


def test_tile_counts_of_the_pixels_under_test():
    """the pixel columns really put the zero counts of the tiles on both sides of every multiple of 16"""
    pixels, _ = _pixels()
    z = np.ones((NTP, N), dtype=bool)
    z[:NT] = pixels == 0
    nz = z.reshape(NTP // 64, 64, N).sum(axis=1)
    met = {int(v) for s in ZEROS for v in nz[:, s - 1]}
    assert {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64} <= met, sorted(met)
    assert (pixels[:, 2] == 0).all() and (pixels[:, 3] == 255).all()


def test_share_of_groups_without_odd_rows_on_the_benchmark_data():
    """what the option rests on: in the benchmark's synthetic images 0.487 of all 16-image groups hold zero pixels only once every
    64-image tile is walked zero pixels first (natural order: 0.05)"""
    from tnml_amd import synth
    labels = synth.synthetic_labels(60000)
    z = synth.synthetic_images(784, labels) == 0
    nt = 60000 // 64 * 64
    nz = z[:nt].reshape(nt // 64, 64, -1).sum(axis=1)
    share = (nz // 16).sum() / (nt // 16 * 784)
    print("zero pixels %.4f; groups of zero pixels only, zero-first inside each tile: %.4f" % (z.mean(), share))
    assert abs(share - 0.487) <= 0.005, share


@pytest.mark.gpu
@pytest.mark.parametrize("m", [33, 72, 120])
def test_zero_first_shift_equals_the_natural_order_and_the_oracle(m):
    """m = 33: instantiation <12>, three column tiles, half-tile dealing; 72: five column tiles; 120: instantiation <30>.  Two workgroups
    (res_grid = 2) run 20 rounds each and prefetch the next tile's order.  Per m: the seven Label-carrying environments with shift_skip = 1
    against the same context's with shift_skip = 0 (np.array_equal) and against the oracle's (1e-12, as test_configs_at_shape.py does), the
    accessor's group counts against a count from the pixels, and one bond update with the resident kernels forced, on and off."""
    from oracle import pyoracle
    from tnml_amd import synth
    from tnml_amd.fixedl import TrainStates
    pixels, labels = _pixels()
    phi = synth.features_series(pixels)
    phi[..., 1] *= 200.0
    W = _mps(m, 100 + m)
    ts = TrainStates(labels, N, m, phi=phi)
    for k in ("fwd_res", "shift_res", "grad_quad"):
        ts.set_option(k, 2)
    ts.set_option("res_grid", 2)
    want = _group_counts(pixels)
    for j in range(1, N + 1):
        assert ts.shift_skip_stats(j) == (NTP // 16, int(want[j - 1])), j
    got = {}
    for skip in (1, 0):
        ts.set_option("shift_skip", skip)
        ts.set_mps(W)
        ts.profile(True, only="fgemm_shift")
        ts.profile_reset()
        ts.init()
        envs = {j: ts.env(j) for j in RIGHT}
        for bb in range(1, 11):
            ts.shiftE(bb, True)
            if bb in LEFT:
                envs[bb] = ts.env(bb)
        ts.profile(False)
        assert ts.profile_read()["fgemm_shift"][0] >= len(RIGHT) + len(LEFT)          # k_shift_res ran (shift_res = 2 forces it)
        rep = ts.bond_update(11, 1, m, m // 2, 1e-10, 3, 1e-3, 1e-10)
        got[skip] = (envs, rep)
    ts.close()
    for j in RIGHT + LEFT:
        assert got[1][0][j].shape == (NT, m, 10)
        assert np.array_equal(got[1][0][j], got[0][0][j]), j
    ron, roff = got[1][1], got[0][1]
    for k in ("newm", "ncorrect", "cost", "truncerr"):
        assert ron[k] == roff[k], (k, ron[k], roff[k])
    assert ron["cg"]["cost"] == roff["cg"]["cost"] and ron["cg"]["alpha"] == roff["cg"]["alpha"]
    o = pyoracle.Oracle(phi, labels, W, nthread=min(8, os.cpu_count() or 1))
    o.init()
    for j in RIGHT:
        assert _rel(got[1][0][j], o.env(j)) < 1e-12, j
    for bb in range(1, 11):
        o.shiftE(bb, True)
        if bb in LEFT:
            assert _rel(got[1][0][bb], o.env(bb)) < 1e-12, bb
