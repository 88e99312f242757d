"""The host side of the input map (tnml_set_input_map): the feature table of the drivers' maps (hostlib.feature_table over
init_w.h feature_of_value) and the geometry and integer reference of InputMap.  No GPU."""
import numpy as np
import pytest

BLOCKS = (1, 2, 8)


def _values(block):
    """the block mean of every code, as reduce() forms it: an exact integer sum divided once"""
    return np.arange(255 * block * block + 1) / float(block * block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("scale", [1.0, 255.0])
def test_series_table_is_the_numpy_formula_exactly(block, scale):
    from tnml_amd import hostlib
    t = hostlib.feature_table("series", scale, block)
    g = _values(block) / 255.
    assert t.shape == (255 * block * block + 1, 2)
    assert np.array_equal(t[:, 0], np.ones(len(g)))
    assert np.array_equal(t[:, 1], scale * ((g / 255.) / 4.))
    assert tuple(t[0]) == (1.0, 0.0)


@pytest.mark.parametrize("block", BLOCKS)
def test_normal_table_is_the_numpy_formula_within_two_ulps_of_one(block):
    from tnml_amd import hostlib
    t = hostlib.feature_table("normal", 1.0, block)
    x = (_values(block) / 255.) / 255.
    err = max(np.abs(t[:, 0] - np.cos(np.pi / 2. * x)).max(), np.abs(t[:, 1] - np.sin(np.pi / 2. * x)).max())
    print("block", block, "max |table - numpy| =", err)
    assert t.shape == (255 * block * block + 1, 2)
    assert err <= 4e-16                                           # two ulps of 1: the only freedom between two libms
    assert tuple(t[0]) == (1.0, 0.0)
    assert np.array_equal(t, hostlib.feature_table("normal", 255.0, block))    # the normal map has no scale


def test_feature_table_refuses_what_it_cannot_build():
    from tnml_amd import hostlib
    with pytest.raises(ValueError):
        hostlib.feature_table("series", 1.0, 9)
    with pytest.raises(ValueError):
        hostlib.feature_table("cosine", 1.0, 1)


@pytest.mark.parametrize("side,imglen,block,origin", [(28, 14, 2, 0), (28, 10, 2, 0), (13, 4, 3, 1), (8, 8, 1, 0)])
def test_from_imglen_has_the_geometry_of_reduce(side, imglen, block, origin):
    """(28, 10) leaves the bottom and right rows uncovered, (13, 4) starts its blocks at 1; the block means of codes() are the
    doubles reduce() keeps, and table[codes] the doubles the feature functions make of them"""
    from tnml_amd import hostlib
    from tnml_amd.input_map import InputMap
    m = InputMap.from_imglen(side, imglen, "series", 255.0)
    assert (m.src_rows, m.src_cols, m.block, m.row0, m.col0, m.out_rows, m.out_cols) == (side, side, block, origin, origin, imglen, imglen)
    assert m.ncodes == 255 * block * block + 1 and m.S == side * side and m.N == imglen * imglen
    px = np.random.default_rng(side * 100 + imglen).integers(0, 256, (5, side * side), dtype=np.uint8)
    px[0] = 0
    px[1] = 255
    codes = m.codes(px)
    assert codes.shape == (5, imglen * imglen) and codes.dtype.kind == "i"
    if imglen == side:
        assert np.array_equal(codes, px)
    else:
        assert np.array_equal(codes / float(block * block), hostlib.reduce(px, side, imglen))
    assert np.array_equal(m.features(px)[..., 1], 255.0 * (((codes / float(block * block)) / 255.) / 255.) / 4.)
    # table[codes] is bit for bit what the drivers' host path (reduce + all_features) makes of the same images, for both maps
    assert np.array_equal(m.features(px), hostlib.features(px, "series", 255.0, imglen=0 if imglen == side else imglen))
    mn = InputMap.from_imglen(side, imglen, "normal")
    assert np.array_equal(mn.features(px), hostlib.features(px, "normal", imglen=0 if imglen == side else imglen))
    # the uncovered pixels do not count
    if origin + block * imglen < side:
        edge = px.reshape(5, side, side).copy()
        edge[:, origin + block * imglen:, :] ^= 0xff
        edge[:, :, origin + block * imglen:] ^= 0xff
        assert np.array_equal(m.codes(edge.reshape(5, -1)), codes)
    if origin:
        edge = px.reshape(5, side, side).copy()
        edge[:, :origin, :] ^= 0xff
        edge[:, :, :origin] ^= 0xff
        assert np.array_equal(m.codes(edge.reshape(5, -1)), codes)


@pytest.mark.parametrize("side,imglen", [(28, 14), (13, 4), (16, 2), (8, 8)])
def test_codes_of_an_all_255_image_are_the_last_table_row(side, imglen):
    from tnml_amd.input_map import InputMap
    m = InputMap.from_imglen(side, imglen, "normal")
    codes = m.codes(np.full((2, side * side), 255, dtype=np.uint8))
    assert np.array_equal(codes, np.full((2, imglen * imglen), 255 * m.block * m.block))
    assert codes.max() == m.ncodes - 1


def test_from_imglen_refuses_what_reduce_refuses():
    from tnml_amd.input_map import InputMap
    for bad in (0, 29):
        with pytest.raises(ValueError, match="imglen must be between 1 and the image side"):
            InputMap.from_imglen(28, bad)
    with pytest.raises(ValueError, match="shape"):
        InputMap.from_imglen(8, 4).codes(np.zeros((3, 16), dtype=np.uint8))


def test_describe_is_the_drivers_line():
    from tnml_amd.input_map import InputMap
    assert InputMap.from_imglen(28, 14, "normal").describe() == \
        "Input map: 28 x 28 bytes -> 14 x 14 sites (2 x 2 block sums from (0, 0)), feature = normal, 1021 codes"
