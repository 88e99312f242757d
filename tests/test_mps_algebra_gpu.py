"""MPS algebra on the device (tnml_mps_place / tnml_mps_compress / tnml_mps_overlap): the sum of ten per-label weight MPS behind
fixedL's W0..W9 start (fixedL.cc:682-701) and overlap(W,W) (:729), against the host library's one-shot sum (tnmlh_mps_sum), dense
contractions and the parts' own outputs.  Parts, images and tolerances: tests/mps_parts.py."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import mps_parts as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTOFF = 1e-10


def _algebra_states(N, maxm):
    """a context for the MPS algebra alone: one image slot, no tnml_set_data_* call"""
    from tnml_amd.fixedl import TrainStates
    return TrainStates(np.zeros(1, dtype=np.int32), N, maxm, no_data=True)


@functools.lru_cache(maxsize=None)
def _device_sum(N, m, maxm=0):
    """place the ten parts, compress once; everything the tests look at (computed once per shape)"""
    parts, _ = mp.problem(N, m)
    ts = _algebra_states(N, 10 * m)
    ts.set_sum(parts)
    direct = ts.get_mps() if 10 * m <= 60 else None
    ovl0 = ts.overlap()
    rep = ts.compress(CUTOFF, maxm)
    W = ts.get_mps()
    out = dict(W=W, rep=rep, ovl_before=ovl0, ovl=ts.overlap(), direct=direct, svd=ts.svd_stats())
    ts.close()
    return out


@functools.lru_cache(maxsize=None)
def _host_sum(N, m, maxm=0):
    import tempfile
    parts, _ = mp.problem(N, m)
    with tempfile.TemporaryDirectory() as d:
        return mp.host_sum(parts, d, cutoff=CUTOFF, maxm=maxm, one_shot=True)


def _rel(a, b):
    return abs(a - b) / abs(b)


def _check_against_host(N, m, dense):
    parts, phi = mp.problem(N, m)
    dev, host = _device_sum(N, m), _host_sum(N, m)
    rank = mp.generic_rank(N, 10 * m)
    msg = "svd_stats %r, report %r" % (dev["svd"], {k: v for k, v in dev["rep"].items() if k not in ("newm", "truncerr")})
    if dense:
        # the precondition, on the reference side only: the truncation is decided by the rank, far from the cutoff
        sp = mp.bond_spectra(mp.dense_sum(parts), N)
        kept, disc = min(p[r - 1] for p, r in zip(sp, rank)), max(p[r:].sum() for p, r in zip(sp, rank))
        print("smallest kept weight %.3e, largest discarded %.3e" % (kept, disc))
        assert kept >= 1e-8 and disc <= 1e-12, (kept, disc)
    assert mp.bond_dims(host) == rank
    assert mp.bond_dims(dev["W"]) == rank, msg
    assert dev["rep"]["newm"] == rank and dev["rep"]["maxm_before"] == 10 * m and dev["rep"]["maxm_after"] == max(rank), msg
    assert [A.ndim == 4 for A in dev["W"]] == [j == N // 2 for j in range(1, N + 1)]
    mp.check_outputs(dev["W"], parts, phi)
    ref = mp.transfer_overlap(dev["W"])
    print("overlap device %.15e numpy %.15e rel %.2e; before the compress %.15e" % (dev["ovl"], ref, _rel(dev["ovl"], ref), dev["ovl_before"]))
    assert _rel(dev["ovl"], ref) <= 1e-12, msg
    assert _rel(dev["ovl_before"], dev["ovl"]) <= 1e-10, msg
    print("discarded weight %.3e" % dev["rep"]["truncerr_sum"])
    assert 0. <= dev["rep"]["truncerr_sum"] <= 2 * (N - 1) * CUTOFF, msg
    assert dev["rep"]["truncerr_sum"] == pytest.approx(float(np.sum(dev["rep"]["truncerr"])), rel=1e-12, abs=1e-300)


@pytest.mark.parametrize("m", [5, 3])
def test_sum_against_host_rank_decided(m):
    """N = 16, ten parts of bond 5 (direct sum 50, rank deficient near both ends) and of bond 3: the device's bond dimensions are the
    host's and the dense rank, its outputs are the parts', its overlap is the numpy transfer chain's"""
    _check_against_host(16, m, dense=True)


def test_placement_is_the_direct_sum():
    """before the compress the context holds the block-diagonal direct sum: part k's site tensors on the diagonal blocks, in label slot k
    on site c0, zeros elsewhere"""
    N, m = 16, 5
    parts, _ = mp.problem(N, m)
    W = _device_sum(N, m)["direct"]
    for j, A in enumerate(W, start=1):
        ref = np.zeros_like(A)
        r0 = c0 = 0
        for k, P in enumerate(parts):
            B = P[j - 1]
            rs = slice(0, 1) if j == 1 else slice(r0, r0 + B.shape[0])
            cs = slice(0, 1) if j == N else slice(c0, c0 + B.shape[2])
            if j == N // 2:
                ref[rs, :, cs, k] += B
            else:
                ref[rs, :, cs] += B
            r0 += B.shape[0]
            c0 += B.shape[2]
        assert np.array_equal(A, ref), j


def test_truncation_by_maxm():
    """maxm = 12 against the host's one-shot compress at maxm = 12: equal bond dimensions, and d^2 = |W' - W_exact|^2 / |W_exact|^2 from
    dense contractions equal to 1e-6 relative (the truncation-error tolerance of DESIGN.md section 2) and bounded by twice the sum of the
    reported truncation errors"""
    N, m = 16, 5
    parts, _ = mp.problem(N, m)
    dev, host = _device_sum(N, m, 12), _host_sum(N, m, 12)
    assert mp.bond_dims(dev["W"]) == mp.bond_dims(host) == [min(12, r) for r in mp.generic_rank(N, 10 * m)]
    T0 = mp.dense_sum(parts)
    d2 = [float(np.sum((mp.dense_labelled(W) - T0) ** 2) / np.sum(T0 ** 2)) for W in (dev["W"], host)]
    print("d2 device %.12e host %.12e rel %.2e; sum of truncation errors %.12e" % (d2[0], d2[1], _rel(d2[0], d2[1]), dev["rep"]["truncerr_sum"]))
    assert _rel(d2[0], d2[1]) <= 1e-6
    assert d2[0] <= 2 * dev["rep"]["truncerr_sum"]


def test_workgroup_cluster_eigensolver_range():
    """N = 20, ten parts of bond 13: the direct sum has bond 130, the Gram matrices of the bulk splits n = 260 > 240 (the workgroup
    cluster), the two Label-on-B bonds 2 600 rows"""
    _check_against_host(20, 13, dense=False)


def test_above_the_in_house_range():
    """N = 24, ten parts of bond 52: sum 520, n = 1 040 > 1 024 goes to rocSOLVER.  No host reference at this size (minutes): the
    outputs are the parts', and the overlap before and after the compress agree"""
    N, m = 24, 52
    parts, phi = mp.problem(N, m)
    dev = _device_sum(N, m)
    msg = "svd_stats %r" % (dev["svd"],)
    assert dev["rep"]["maxm_before"] == 520 and mp.bond_dims(dev["W"]) == dev["rep"]["newm"]
    assert all(a <= b for a, b in zip(mp.bond_dims(dev["W"]), mp.generic_rank(N, 520))), msg
    mp.check_outputs(dev["W"], parts, phi)
    print("overlap before %.15e after %.15e rel %.2e" % (dev["ovl_before"], dev["ovl"], _rel(dev["ovl_before"], dev["ovl"])))
    assert _rel(dev["ovl_before"], dev["ovl"]) <= 1e-10, msg


def test_placement_refusals():
    from tnml_amd.fixedl import TnmlError
    N = 8
    ts = _algebra_states(N, 6)
    A = np.ones((2, 2, 3))
    with pytest.raises(TnmlError, match="leaves the 4 x 6 site"):
        ts.place(3, 4, 6, 3, 0, A)                       # rows 3..4 of 4
    with pytest.raises(TnmlError, match="leaves the 4 x 6 site"):
        ts.place(3, 4, 6, 0, 4, A)                       # columns 4..6 of 6
    with pytest.raises(TnmlError, match="leaves"):
        ts.place(3, 4, 6, -1, 0, A)
    with pytest.raises(TnmlError, match="has no Label index"):
        ts.place(3, 4, 6, 0, 0, A, label=2)              # a label slot off c0
    with pytest.raises(TnmlError, match="label must be in 0..9"):
        ts.place(N // 2, 4, 6, 0, 0, A)                  # none on c0
    with pytest.raises(TnmlError, match="label must be in 0..9"):
        ts.place(N // 2, 4, 6, 0, 0, A, label=10)
    with pytest.raises(TnmlError, match="outside 1..maxm"):
        ts.place(3, 7, 6, 0, 0, A)
    with pytest.raises(TnmlError, match="edge sites"):
        ts.place(1, 2, 6, 0, 0, A)
    with pytest.raises(TnmlError, match="out of range"):
        ts.place(N + 1, 4, 6, 0, 0, A)
    # nothing above touched the site; two placements add, a new shape starts over
    ts.place(3, 4, 6, 1, 2, A)
    ts.place(3, 4, 6, 2, 3, 2 * A)
    ref = np.zeros((4, 2, 6))
    ref[1:3, :, 2:5] += 1.
    ref[2:4, :, 3:6] += 2.
    assert np.array_equal(ts.get_site(3), ref)
    ts.place(3, 2, 3, 0, 0, A)
    assert np.array_equal(ts.get_site(3), A)
    ts.place(N // 2, 2, 3, 0, 0, A, label=7)
    got = ts.get_site(N // 2)
    assert got.shape == (2, 2, 3, 10) and np.array_equal(got[..., 7], A) and np.count_nonzero(got) == A.size
    with pytest.raises(TnmlError, match="site 1 not set"):
        ts.compress(CUTOFF)                               # an incomplete W
    ts.close()


def _data_states(N, maxm, NT=40, seed=5, **kw):
    from tnml_amd.fixedl import TrainStates
    phi = mp.make_images(N, NT, seed=seed)
    lab = (np.arange(NT) % 10).astype(np.int32)
    return TrainStates(lab, N, maxm, phi=phi, **kw), phi, lab


def test_compress_refusals(monkeypatch):
    from tnml_amd.fixedl import TnmlError, TrainStates
    N, m = 10, 2
    parts = mp.make_parts(N, m, seed=9)
    # a bond update in flight
    ts, phi, lab = _data_states(N, 10 * m)
    ts.set_sum(parts)
    ts.init()
    ts.bond_update_begin(1, 1, 10 * m, 1, 1e-10, 2, 1e-3, 1e-10)
    with pytest.raises(TnmlError, match="bond update is in flight"):
        ts.compress(CUTOFF)
    with pytest.raises(TnmlError, match="bond update is in flight"):
        ts.place(3, 1, 1, 0, 0, np.ones((1, 2, 1)))
    ts.bond_update_end()
    # a held-out context attached: refused on both sides
    ts.set_sum(parts)
    ts.init()
    hs, _, _ = _data_states(N, 10 * m, NT=20, seed=6)
    ts.attach_heldout(hs)
    with pytest.raises(TnmlError, match="held-out"):
        ts.compress(CUTOFF)
    with pytest.raises(TnmlError, match="held-out"):
        hs.compress(CUTOFF)
    ts.detach_heldout()
    ts.compress(CUTOFF)                                   # and allowed again
    hs.close()
    ts.close()
    # a communicator, even of one rank
    monkeypatch.setenv("TNML_FORCE_COMM", "1")
    tc, _, _ = _data_states(N, 10 * m)
    tc.comm_init(TrainStates.comm_unique_id())
    tc.set_sum(parts)
    with pytest.raises(TnmlError, match="one rank only"):
        tc.compress(CUTOFF)
    tc.close()


def test_environments_after_a_compress():
    """after a compress the caller runs tnml_env_init: the cost on bond 1 is the oracle's cost of the downloaded W (TOL of tests/test_gpu_parity.py)"""
    from oracle import pyoracle
    N, m = 12, 3
    parts, _ = mp.problem(N, m)
    ts, phi, lab = _data_states(N, 10 * m)
    ts.set_sum(parts)
    ts.init()                                             # environments of the direct sum: stale after the compress
    rep = ts.compress(CUTOFF)
    assert rep["newm"] == mp.generic_rank(N, 10 * m) and rep["newm"][0] == 2 < rep["maxm_before"]      # the bonds changed under the old environments
    W = ts.get_mps()
    ts.init()
    B = ts.bond_tensor(1)
    o = pyoracle.Oracle(phi, lab, W)
    o.init()
    assert np.allclose(B, o.bond_tensor(1), rtol=0, atol=1e-13 * np.abs(B).max())
    cost, ref = ts.quadcost(B, 1e-3)[0], o.quadcost(o.bond_tensor(1), 1e-3)[0]
    print("cost %.15e oracle %.15e rel %.2e" % (cost, ref, _rel(cost, ref)))
    assert _rel(cost, ref) <= 1e-11
    ts.close()


def _driver_dir(tmp_path, name, m, extra=""):
    from tnml_amd import hostlib, synth
    N, per_label = 16, 4
    labels = synth.synthetic_labels(10 * per_label, seed=12, per_label=per_label)
    pixels = np.clip(synth.synthetic_images(N, labels, seed=12).astype(np.int32) * 3, 0, 255).astype(np.uint8)
    data = str(tmp_path / "data")
    if not os.path.exists(data):
        synth.write_idx(data, pixels, labels)
    wd = tmp_path / name
    wd.mkdir()
    parts, _ = mp.problem(N, m)
    for k, P in enumerate(parts):
        hostlib.write_mps(str(wd / ("W%d" % k)), P)
    (wd / "input").write_text("input\n{\ndatadir = %s\nNtrain = %d\nNbatch = 4\nNsweep = 0\nmaxm = 60\nlambda = 1E-3\nfeature_scale = 255\n%s}\n" % (data, per_label, extra))
    run = subprocess.run([os.path.join(ROOT, "tnml_amd", "fixedL"), "input"], capture_output=True, text=True, cwd=wd, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    assert "Found separate W0,W1,...,W9 MPS: summing" in run.stdout and "Summing all 10 label states together" in run.stdout
    return run.stdout, wd, data, per_label, parts


def _check_driver_w(out, wd, data, per_label, parts):
    from oracle import pyoracle
    from tnml_amd import hostlib
    W = hostlib.read_mps(str(wd / "W"))
    N = len(W)
    assert [A.ndim == 4 for A in W] == [j == N // 2 for j in range(1, N + 1)]
    px, lab, _ = hostlib.read_mnist(data, True, per_label)
    g = px.astype(np.float64) / 255.0
    phi = np.stack([np.ones_like(g), 255.0 * ((g / 255.0) / 4.0)], axis=-1)
    mp.check_outputs(W, parts, phi)
    mp.check_outputs(W, parts, mp.problem(N, parts[0][1].shape[0])[1])
    o = pyoracle.Oracle(phi, lab, W)
    o.init()
    C0 = o.quadcost(o.bond_tensor(1), 1e-3)[0] / len(lab)
    m0 = re.search(r"Before starting DMRG Cost = ([0-9.eE+-]+)", out)
    assert m0 and float(m0.group(1)) == pytest.approx(C0, rel=1e-8)
    ov = re.search(r"overlap\(W,W\) = ([0-9.eE+-]+)", out)
    assert ov and float(ov.group(1)) == pytest.approx(mp.transfer_overlap(W), rel=1e-10)


def test_driver_sums_w0_w9_on_the_gpu(tmp_path):
    """parts of bond 5 (direct sum 50 > 40): mps_device = auto takes the device path and says so; mps_device = no stays on the host;
    both leave a W whose label outputs are the parts' and print the oracle's cost of that W"""
    out, wd, data, per_label, parts = _driver_dir(tmp_path, "auto", 5)
    line = re.search(r"Compressed on the GPU: largest bond (\d+) -> (\d+), discarded weight ([0-9.eE+-]+)", out)
    assert line, out[-1500:]
    assert int(line.group(1)) == 50 and int(line.group(2)) == 50 and float(line.group(3)) <= 2 * 15 * CUTOFF
    _check_driver_w(out, wd, data, per_label, parts)
    out, wd, data, per_label, parts = _driver_dir(tmp_path, "host", 5, "mps_device = no\n")
    assert "Compressed on the GPU" not in out
    _check_driver_w(out, wd, data, per_label, parts)


def test_driver_keeps_small_sums_on_the_host(tmp_path):
    """parts of bond 4 (direct sum 40) and no key: the host path, unchanged; sum_maxm reaches the compress on either path"""
    out, wd, data, per_label, parts = _driver_dir(tmp_path, "small", 4)
    assert "Compressed on the GPU" not in out
    _check_driver_w(out, wd, data, per_label, parts)
    from tnml_amd import hostlib
    for name, extra in (("mx_host", "mps_device = no\nsum_maxm = 9\n"), ("mx_dev", "mps_device = yes\nsum_maxm = 9\n")):
        out, wd, *_ = _driver_dir(tmp_path, name, 4, extra)
        assert ("Compressed on the GPU" in out) == (name == "mx_dev")
        assert max(mp.bond_dims(hostlib.read_mps(str(wd / "W")))) == 9
