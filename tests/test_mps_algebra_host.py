"""The host mirror of the W0..W9 sum (tnmlh_mps_sum): sum(ipsis,{"Cutoff",1E-10}) of fixedL.cc:682-697 part by part, as the fixedL
driver's host path does it, and in one shot -- the reference of tests/test_mps_algebra_gpu.py.  No GPU."""
import numpy as np
import pytest

import mps_parts as mp

N, M = 12, 3
RANK = [2, 4, 8, 16, 30, 30, 30, 16, 8, 4, 2]


def test_dense_rank_of_the_exact_sum():
    """the expected bond dimensions are the exact rank of the sum: from the dense SVD of every bond, every kept weight is >= 1e-8 of
    the total and everything beyond the rank <= 1e-12"""
    parts, _ = mp.problem(N, M)
    assert mp.generic_rank(N, 10 * M) == RANK
    for b, p in enumerate(mp.bond_spectra(mp.dense_sum(parts), N), start=1):
        r = RANK[b - 1]
        assert p[r - 1] >= 1e-8 and p[r:].sum() <= 1e-12, (b, p[r - 1], p[r:].sum())


@pytest.mark.parametrize("one_shot", [False, True], ids=["part_by_part", "one_shot"])
def test_host_sum_of_ten_parts(tmp_path, one_shot):
    parts, phi = mp.problem(N, M)
    W = mp.host_sum(parts, tmp_path, cutoff=1e-10, one_shot=one_shot)
    assert len(W) == N and [A.ndim == 4 for A in W] == [j == N // 2 for j in range(1, N + 1)]
    assert mp.bond_dims(W) == RANK
    mp.check_outputs(W, parts, phi)
    # and the whole tensor, not only 40 images of it
    T, T0 = mp.dense_labelled(W), mp.dense_sum(parts)
    assert np.linalg.norm(T - T0) <= 1e-5 * np.linalg.norm(T0)


def test_host_sum_maxm_is_handed_to_the_compress(tmp_path):
    parts, _ = mp.problem(N, M)
    W = mp.host_sum(parts, tmp_path, cutoff=1e-10, maxm=7, one_shot=True)
    assert mp.bond_dims(W) == [min(7, r) for r in RANK]


def test_host_sum_refuses_a_labelled_part(tmp_path):
    from tnml_amd import hostlib
    parts, _ = mp.problem(N, M)
    W = mp.host_sum(parts, tmp_path)
    hostlib.write_mps(str(tmp_path / "L"), W)
    with pytest.raises(RuntimeError, match="already carries a Label index"):
        hostlib.mps_sum([str(tmp_path / "L")], str(tmp_path / "out"))


def test_host_overlap_of_a_weight_file(tmp_path):
    """tnmlh_mps_overlap: the whole chain is overlap(W,W); the first k sites alone are the chain cut after site k with its right link at 0"""
    from tnml_amd import hostlib
    parts, _ = mp.problem(N, M)
    W = mp.host_sum(parts, tmp_path)
    f = str(tmp_path / "Wf")
    hostlib.write_mps(f, W)
    assert hostlib.mps_overlap(f) == pytest.approx(mp.transfer_overlap(W), rel=1e-12)
    cut = W[:3] + [W[3][:, :, :1]]
    assert hostlib.mps_overlap(f, 4) == pytest.approx(mp.transfer_overlap(cut), rel=1e-12)
