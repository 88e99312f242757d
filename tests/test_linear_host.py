"""CPU tests of the `linear` driver's host side (linear.cc:92-240): the bond-dimension-2 MPS embedding of V (:205-236), the
V%d file format and the driver's refusals.  No GPU involved."""
import os
import subprocess

import numpy as np
import pytest

from tnml_amd import hostlib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tnml_amd", "linear")
if not (os.path.exists(EXE) and os.path.exists(os.path.join(ROOT, "tnml_amd", "libtnml_host.so"))):
    import __graft_entry__                               # an older build tree: conftest builds only when its own targets are missing
    __graft_entry__.build()


def _contract(W, phi):
    """W . Phi for the product state phi[N, 2]"""
    env = np.ones(1)
    for j, A in enumerate(W):
        env = np.einsum("l,lsr,s->r", env, A, phi[j])
    assert env.shape == (1,)
    return env[0]


@pytest.mark.parametrize("N", [4, 16, 784])
def test_embedding_evaluates_to_v_dot_v(tmp_path, N):
    rng = np.random.default_rng(N)
    V = rng.normal(size=N + 1)
    path = str(tmp_path / "W3")
    ovl = hostlib.linear_mps(V, path)
    W = hostlib.read_mps(path)
    assert len(W) == N and all(A.ndim == 3 for A in W)                     # no Label index: fixedL attaches it
    assert max(max(A.shape[0], A.shape[2]) for A in W) <= 2
    assert W[0].shape[0] == 1 and W[-1].shape[2] == 1
    assert abs(ovl - V @ V) <= 1e-13 * (V @ V)                              # overlap(W,W) = sqr(norm(V)), :231-232
    for t in range(3):
        b = rng.integers(0, 256, size=N)
        x = (b / 255.0) / 4.0                                               # linear.cc:118-121,138
        v = np.concatenate([[1.0], x])
        phi = np.stack([np.ones(N), x], axis=1)
        want = V @ v
        assert abs(_contract(W, phi) - want) <= 1e-13 * np.abs(V * v).sum(), (N, t)


@pytest.mark.parametrize("s", [1.0, 255.0, 37.5])
def test_embedding_under_fixedl_feature_map(tmp_path, s):
    """entries V(j) 255/s: W evaluates to V.v under fixedL's map [1, s (b/255/255)/4] (init_w.h features_series)"""
    N = 16
    rng = np.random.default_rng(7)
    V = rng.normal(size=N + 1)
    path = str(tmp_path / "W0")
    hostlib.linear_mps(V, path, entry_scale=255.0 / s)
    W = hostlib.read_mps(path)
    b = rng.integers(0, 256, size=N)
    phi = np.stack([np.ones(N), s * ((b / 255.0 / 255.0) / 4.0)], axis=1)
    v = np.concatenate([[1.0], (b / 255.0) / 4.0])
    assert abs(_contract(W, phi) - V @ v) <= 1e-13 * np.abs(V * v).sum()


def test_vec_file_round_trip(tmp_path):
    V = np.random.default_rng(1).normal(size=17)
    p = str(tmp_path / "V5")
    hostlib.write_vec(p, V)
    np.testing.assert_array_equal(hostlib.read_vec(p), V)
    with open(p, "r+b") as f:
        f.write(b"XXXX")
    with pytest.raises(RuntimeError, match="not a TNMLV1"):
        hostlib.read_vec(p)


def _input(tmp_path, body):
    p = tmp_path / "input_linear"
    p.write_text("input\n{\n" + body + "\n}\n")
    return str(p)


def test_driver_usage_and_refusals(tmp_path):
    out = subprocess.run([EXE], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("Usage:")                         # linear.cc:95
    # no `label` and no `labels`: the reference's mandatory in.getInt("label") (:104)
    inp = _input(tmp_path, "datadir = %s\nNlinear_iter = 3" % (tmp_path / "nodata"))
    out = subprocess.run([EXE, inp], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode != 0 and "`label` not found" in out.stderr
    # data missing
    inp = _input(tmp_path, "datadir = %s\nlabel = 3" % (tmp_path / "nodata"))
    out = subprocess.run([EXE, inp], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode != 0 and "Error opening file %s/train-images-idx3-ubyte" % (tmp_path / "nodata") in out.stderr
    # training data present, test set missing
    labels = synth.synthetic_labels(20, seed=3, per_label=2)
    d = str(tmp_path / "trainonly")
    synth.write_idx(d, synth.synthetic_images(16, labels, seed=3), labels)
    for f in os.listdir(d):
        if f.startswith("t10k"):
            os.remove(os.path.join(d, f))
    inp = _input(tmp_path, "datadir = %s\nlabels = all" % d)
    out = subprocess.run([EXE, inp], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode != 0 and "t10k-images-idx3-ubyte" in out.stderr
    # a bad label list
    inp = _input(tmp_path, "datadir = %s\nlabels = 1,12" % d)
    out = subprocess.run([EXE, inp], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode != 0 and "labels" in out.stderr
    assert not os.path.exists(tmp_path / "V1") and not os.path.exists(tmp_path / "W1")
    # a `sites` file of another size: refused before any work (no GPU is touched), on stderr, nothing written
    synth.write_idx(d, synth.synthetic_images(16, labels, seed=4), labels, train=False)
    wd = tmp_path / "sites_mismatch"
    wd.mkdir()
    hostlib.write_sites(str(wd / "sites"), 25, 2)
    inp = _input(wd, "datadir = %s\nlabel = 1" % d)
    out = subprocess.run([EXE, inp], capture_output=True, text=True, cwd=wd)
    assert out.returncode != 0 and "sites file has 25 sites" in out.stderr
    assert sorted(os.listdir(wd)) == ["input_linear", "sites"]
