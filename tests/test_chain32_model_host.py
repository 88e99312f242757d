"""The fp32 chain model (chain32_model.py) proved on the host before it judges the kernel: its fma against exact rational arithmetic, its
index order against the oracle with rounding switched off, its distance from the oracle against every image's top-two gap, and that
the k order inside a block shows in the bits."""
from fractions import Fraction

import numpy as np
import pytest

import chain32_cases as cases
import chain32_model as cm


def _exact_fma32(a, b, c):
    """fl32(a b + c) by rational arithmetic: round to nearest, ties to even, normal range"""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return 0.0
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    ulp = Fraction(2) ** (e - 23)
    qf = x / ulp
    q = qf.numerator // qf.denominator
    rem = qf - q
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and q % 2 == 1):
        q += 1
    return sign * float(q * ulp)


def test_fma_emulation_is_correctly_rounded():
    rng = np.random.default_rng(1)
    n = 4000
    a = cm.fl32(rng.standard_normal(n) * 2. ** rng.integers(-8, 8, n))
    b = cm.fl32(rng.standard_normal(n) * 2. ** rng.integers(-8, 8, n))
    c = cm.fl32(rng.standard_normal(n) * 2. ** rng.integers(-8, 8, n))
    c[:n // 2] = cm.fl32(-a[:n // 2] * b[:n // 2] * (1 + rng.standard_normal(n // 2) * 1e-3))      # cancellation
    got = cm.fma32(a, b, c)
    want = np.array([_exact_fma32(*t) for t in zip(a, b, c)])
    assert np.array_equal(got, want)
    # the crafted family: a b = 2^-24 + 2^-70 - ..., just above half an ulp of c; the fp64 sum rounds it onto the tie
    k = np.arange(2000, dtype=np.float64)
    a = np.full(2000, 1. + 2. ** -23)
    b = np.full(2000, 2. ** -24 - 2. ** -47)
    c = 1. + k * 2. ** -23
    assert np.array_equal(cm.fl32(a), a) and np.array_equal(cm.fl32(b), b) and np.array_equal(cm.fl32(c), c)
    want = np.array([_exact_fma32(*t) for t in zip(a, b, c)])
    assert np.array_equal(cm.fma32(a, b, c), want)
    wrong = int((cm.fma32_plain(a, b, c) != want).sum())
    print("plain form wrong on", wrong, "of 2000")
    assert wrong > 500                                          # the family bites


def test_byte_features_are_the_oracles():
    from oracle import pyoracle
    px = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(cm.features_u8(px), pyoracle.features_series(px))


@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("kind,key", cases.ALL)
def test_model_without_rounding_is_the_oracle(kind, key, form):
    """fp64 operands and fp64 sums in the model's order: the index order is right"""
    _, f, W = cases.inputs(kind, key)
    w = cm.chain32(W, f[form], exact=True)
    truth = cases.oracle(kind, key, form)
    rel = np.abs(w - truth).max() / np.abs(truth).max()
    print(kind, key, form, "exact model against the oracle: relmax", rel)
    assert rel < 1e-12


@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("kind,key", cases.ALL)
def test_model_stays_inside_half_the_top_two_gap(kind, key, form):
    """every image: max_l |model fp32 - oracle fp64| < half of the oracle's top-two gap, so the predictions agree -- no tolerance, no
    image left out"""
    truth = cases.oracle(kind, key, form)
    w, pred = cases.model(kind, key, form)
    s = np.sort(np.abs(truth), axis=1)
    gap = s[:, -1] - s[:, -2]
    dist = np.abs(w - truth).max(axis=1)
    scale = np.abs(truth).max()
    print(kind, key, form, "relmax(model fp32, oracle fp64) %.3e, smallest top-two gap %.3e (of max|w|), largest distance / half gap %.3e"
          % (dist.max() / scale, gap.min() / scale, (dist / (0.5 * gap)).max()))
    assert np.isfinite(w).all()
    assert (dist < 0.5 * gap).all()
    assert np.array_equal(pred, np.abs(truth).argmax(axis=1))


def test_per_label_model_against_its_oracle():
    phi, W, f = cases.per_label_problem()
    w = cm.chain32(W, phi, exact=True)
    assert np.abs(w - f).max() / np.abs(f).max() < 1e-12
    w32, pred = cm.predict32(W, phi, single=True)
    dist = np.abs(w32 - f)[:, 0]
    print("per-label variant: relmax %.3e, closest to 1/2 %.3e" % (dist.max() / np.abs(f).max(), np.abs(f[:, 0] - 0.5).min()))
    assert (dist < np.abs(f[:, 0] - 0.5)).all()
    assert np.array_equal(pred, (f[:, 0] > 0.5).astype(np.int32))


def test_the_k_order_inside_a_block_shows_in_the_bits():
    differ = []
    for kind, key in (("small", (17, 6)), ("dims", 0)):
        _, f, W = cases.inputs(kind, key)
        rev = cm.chain32(W, f["phi"], reverse=True)
        fwd = cases.model(kind, key, "phi")[0]
        assert np.abs(rev - fwd).max() / np.abs(fwd).max() < 1e-4          # the same sum
        differ.append(not np.array_equal(rev, fwd))
    assert any(differ)
