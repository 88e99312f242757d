"""The device input map (tnml_set_input_map): raw bytes -> block sums -> table look-up -> site-first features, in the staging kernel, in
the chain kernel's third feature source and in tnml_set_data_u8.  The reference for bit equality is always the library's own fp64
feature path fed with table[InputMap.codes(pixels)]: identical feature bits in, identical bits out -- np.array_equal, never a tolerance."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# src_rows, src_cols, block, row0, col0, out_rows, out_cols
GEOMS = {
    "12x12_b2": (12, 12, 2, 0, 0, 6, 6),
    "13x13_b3_from_1": (13, 13, 3, 1, 1, 4, 4),             # S = 169 odd, origin (1, 1), pixels no block covers on every side
    "5x7_b1": (5, 7, 1, 0, 0, 5, 7),                        # not square, S = 35 odd
    "28x28_b2": (28, 28, 2, 0, 0, 14, 14),
    "16x16_b8": (16, 16, 8, 0, 0, 2, 2),                    # all-255 image: code 16 320, the last table row
}
TABLES = ("random", "series255", "normal")
NPRED = 150                                                 # chunks of 64, 64 and 22 at predict_chunk = 64
SWEEP = (6, 3, 1e-10, 3, 1e-3, 1e-10)


def _relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _table(kind, block, seed=0):
    from tnml_amd import hostlib
    if kind == "random":                                    # proves a look-up, not an expression
        rng = np.random.default_rng(1000 + seed)
        n = 255 * block * block + 1
        return np.stack([1. + 0.1 * rng.standard_normal(n), 0.5 * rng.standard_normal(n)], axis=-1)
    return hostlib.feature_table("series", 255.0, block) if kind == "series255" else hostlib.feature_table("normal", 1.0, block)


def _map(geom, kind):
    from tnml_amd.input_map import InputMap
    g = GEOMS[geom]
    return InputMap(*g, _table(kind, g[2], seed=len(geom)))


def _raw(S, n, seed):
    """random byte images; image 0 is all 0, image 1 all 255"""
    px = np.random.default_rng(seed).integers(0, 256, (n, S), dtype=np.uint8)
    px[0] = 0
    if n > 1:
        px[1] = 255
    return px


def _mps_with_dims(dims, seed):
    """random weight MPS with bond dimensions d_0 = 1, d_1, ..., d_N = 1 (Label index on site N/2), any shapes"""
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


def _random_dims(N, top, seed):
    rng = np.random.default_rng(seed)
    return [1] + [int(x) for x in rng.integers(1, top + 1, N - 1)] + [1]


def _dataless(N, maxm, W, single_label=None):
    from tnml_amd.fixedl import TrainStates
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, maxm, no_data=True, single_label=single_label)
    ts.set_mps(W)
    return ts


@functools.lru_cache(maxsize=None)
def _predict_case(geom, kind, top):
    """(map, raw images, W, the oracle's weights on table[codes]) -- computed once per case"""
    from oracle import pyoracle
    m = _map(geom, kind)
    px = _raw(m.S, NPRED, 7 + len(geom))
    dims = _random_dims(m.N, top, 31 + m.N)
    if top > 6:
        dims[m.N // 2] = top                                # the largest bond is really reached
    W = _mps_with_dims(dims, 5)
    o = pyoracle.Oracle(m.features(px), np.zeros(NPRED, dtype=np.int32), W)
    return m, px, W, np.stack([o.toverlap(i) for i in range(NPRED)]), max(dims)


@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("geom,top", [(g, 6) for g in GEOMS] + [("12x12_b2", 40)])
def test_predict_under_a_map_equals_the_feature_path_bitwise(geom, top, kind):
    """data-less contexts, n = 150 in chunks of 64 / 64 / 22, tiles of 16, 32 and 64 images, a permuted batch and 1-image calls"""
    m, px, W, truth, maxm = _predict_case(geom, kind, top)
    assert px[0].max() == 0 and px[1].min() == 255
    if geom == "16x16_b8":
        assert m.codes(px[1:2]).min() == 16320 == m.ncodes - 1
    ts = _dataless(m.N, maxm, W)
    ts.set_option("predict_chunk", 64)
    w_ref, p_ref = ts.predict(phi=m.features(px))
    print(geom, kind, "bonds <=", top, "feature path against the oracle: relmax", _relmax(w_ref, truth))
    assert _relmax(w_ref, truth) <= 1e-12
    ts.set_input_map(m)
    assert ts.input_map() == dict(zip(("src_rows", "src_cols", "block", "row0", "col0", "out_rows", "out_cols"), GEOMS[geom]), ncodes=m.ncodes)
    for tile in (16, 32, 64):
        ts.set_option("predict_tile", tile)
        w, p = ts.predict(pixels=px)
        assert np.array_equal(w, w_ref), (tile, np.abs(w - w_ref).max())
        assert np.array_equal(p, p_ref), tile
        assert _relmax(w, truth) <= 1e-12
    ts.set_option("predict_tile", 0)
    perm = np.random.default_rng(5).permutation(NPRED)
    wp, pp = ts.predict(pixels=px[perm])
    assert np.array_equal(wp, w_ref[perm]) and np.array_equal(pp, p_ref[perm])
    for i in (0, 1, 77, NPRED - 1):
        w1, p1 = ts.predict(pixels=px[i:i + 1])
        assert np.array_equal(w1, w_ref[i:i + 1]) and np.array_equal(p1, p_ref[i:i + 1]), i
    ts.close()


# ---- training data ---------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _same_report(a, b):
    for key in a:
        if key == "cg":
            for k2 in a["cg"]:
                assert _same(a["cg"][k2], b["cg"][k2]), ("cg", k2, a["cg"][k2], b["cg"][k2])
        else:
            assert _same(a[key], b[key]), (key, a[key], b[key])


def _envs(ts):
    out = {}
    for j in range(1, ts.N + 1):
        try:
            out[j] = ts.env(j)
        except Exception:
            pass
    return out


def _bond_updates(ts, bonds):
    """init, then one bond update at each bond of `bonds` (ascending), walking there by shifts: (environments after init, [(report, A_b, A_b+1)])"""
    ts.init()
    envs = _envs(ts)
    out, at = [], 1
    for b in bonds:
        for bb in range(at, b):
            ts.shiftE(bb, True)
        rep = ts.bond_update(b, 1, *SWEEP)
        out.append((rep, ts.get_site(b), ts.get_site(b + 1)))
        at = b + 1
    return envs, out


@pytest.mark.parametrize("dtype", ["f64", "f64_e32"])
@pytest.mark.parametrize("NT", [1, 37, 257])
def test_training_data_under_a_map_equals_set_data_phi(NT, dtype):
    """TrainStates(pixels=raw, input_map=m) against TrainStates(phi=table[codes]): every environment after init, and the report and the
    two rewritten site tensors of a bond update at a Label-free bond (1) and at a Label-on-B bond (17: sites 17 and 18 = N/2)"""
    from tnml_amd import synth
    from tnml_amd.fixedl import TrainStates
    m = _map("12x12_b2", "normal")
    N = m.N
    px = _raw(m.S, NT, 100 + NT)
    labels = np.random.default_rng(NT).integers(0, 10, NT).astype(np.int32)
    W = synth.random_mps(N, 6, seed=12)
    got = []
    for mapped in (True, False):
        ts = TrainStates(labels, N, 6, dtype=dtype, **(dict(pixels=px, input_map=m) if mapped else dict(phi=m.features(px))))
        ts.set_mps(W)
        got.append(_bond_updates(ts, (1, N // 2 - 1)))
        ts.close()
    (ea, ua), (eb, ub) = got
    assert sorted(ea) == sorted(eb) == list(range(3, N + 1)), (sorted(ea), sorted(eb))     # init builds the environments of sites N .. 3
    for j in ea:
        assert _same(ea[j], eb[j]), j
    assert [u[0]["label_on_B"] for u in ua] == [False, True]
    for (ra, a1, a2), (rb, b1, b2) in zip(ua, ub):
        _same_report(ra, rb)
        assert _same(a1, b1) and _same(a2, b2), ra["bond"]


def test_zero_skip_tables_follow_the_mapped_features():
    """maxm = 40, fp64: the tile order tables of the resident-operand shift are built from the stored features, so they must follow the
    map.  sin(pi x / 2) is zero at code 0 only, so the groups left out are the 16-image groups of zero block sums: compared with the
    reference context site by site, and they differ between the sites"""
    from tnml_amd.fixedl import TrainStates
    m = _map("12x12_b2", "normal")
    assert (m.table[1:, 1] != 0).all() and m.table[0, 1] == 0
    NT = 257
    rng = np.random.default_rng(77)
    img = rng.integers(1, 256, (NT, 12, 12), dtype=np.uint8)
    img[:, :, :4] = 0                                       # sites of columns 0, 1: zero in every image
    img[:128, 4:8, :] = 0                                   # sites of rows 2, 3: zero in the first 128 images
    img[rng.random((NT, 12, 12)) < 0.3] = 0                 # single zero bytes: no zero block sum by themselves
    px = img.reshape(NT, -1)
    labels = rng.integers(0, 10, NT).astype(np.int32)
    a = TrainStates(labels, m.N, 40, pixels=px, input_map=m)
    b = TrainStates(labels, m.N, 40, phi=m.features(px))
    sa = [a.shift_skip_stats(j) for j in range(1, m.N + 1)]
    sb = [b.shift_skip_stats(j) for j in range(1, m.N + 1)]
    a.close()
    b.close()
    print("groups, skipped per site:", sa)
    assert sa == sb
    skipped = [s[1] for s in sa]
    # (the 255 padding images count as zero features everywhere, so no site is at 0; the all-zero columns reach every group)
    assert max(skipped) == sa[0][0] and min(skipped) < max(skipped) and len(set(skipped)) >= 3, skipped


# ---- per-label variant -----------------------------------------------------------------------------------------------------------
def test_per_label_variant_under_a_map():
    """single_label = 3, the drivers' normal map on 8 x 8 -> 4 x 4: predict on a data-less context and one bond update of a training context"""
    from tnml_amd import synth
    from tnml_amd.fixedl import TrainStates
    from tnml_amd.input_map import InputMap
    m = InputMap.from_imglen(8, 4, "normal")
    N, NT = m.N, 90
    px = _raw(m.S, NT, 8)
    labels = np.random.default_rng(8).integers(0, 10, NT).astype(np.int32)
    W = synth.random_mps(N, 4, seed=10)
    W[N // 2 - 1] = W[N // 2 - 1][..., 0] * 3.0            # plain MPS: no Label index
    ts = _dataless(N, 4, W, single_label=3)
    w_ref, p_ref = ts.predict(phi=m.features(px))
    ts.set_input_map(m)
    w, p = ts.predict(pixels=px)
    ts.close()
    assert w.shape == (NT, 1) and np.array_equal(w, w_ref) and np.array_equal(p, p_ref)
    got = []
    for mapped in (True, False):
        ts = TrainStates(labels, N, 4, single_label=3, **(dict(pixels=px, input_map=m) if mapped else dict(phi=m.features(px))))
        ts.set_mps(W)
        ts.init()
        rep = ts.bond_update(1, 1, 4, 2, 1e-10, 3, 1e-3, 1e-10)
        got.append((rep, ts.get_site(1), ts.get_site(2)))
        ts.close()
    _same_report(got[0][0], got[1][0])
    assert _same(got[0][1], got[1][1]) and _same(got[0][2], got[1][2])


# ---- no map, and map removed -----------------------------------------------------------------------------------------------------
def test_without_a_map_and_after_removing_it_the_builtin_path_is_untouched():
    from tnml_amd import hostlib
    from tnml_amd.input_map import InputMap
    N = 16
    W = _mps_with_dims(_random_dims(N, 6, 3), 9)
    px = _raw(N, 70, 2)
    fresh = _dataless(N, 6, W)
    w0, p0 = fresh.predict(pixels=px)
    fresh.close()
    ts = _dataless(N, 6, W)
    assert ts.input_map() is None
    ts.set_input_map(_map("13x13_b3_from_1", "random"))
    ts.predict(pixels=_raw(169, 5, 1))
    ts.set_input_map(None)
    assert ts.input_map() is None
    w1, p1 = ts.predict(pixels=px)
    assert np.array_equal(w1, w0) and np.array_equal(p1, p0)
    # the built-in map as a table: the same features up to the device's own division
    ident = InputMap(4, 4, 1, 0, 0, 4, 4, hostlib.feature_table("series", 1.0, 1))
    ts.set_input_map(ident)
    w2, p2 = ts.predict(pixels=px)
    ts.close()
    print("series table at scale 1 against the built-in byte path: relmax", _relmax(w2, w0))
    assert _relmax(w2, w0) <= 1e-12


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_previous_map_in_force():
    from conftest import make_problem
    from tnml_amd import lib as _lib
    from tnml_amd.fixedl import TnmlError, TrainStates
    from tnml_amd.input_map import InputMap
    good = _map("13x13_b3_from_1", "random")                # N = 16
    N = good.N
    W = _mps_with_dims(_random_dims(N, 6, 3), 9)
    px = _raw(good.S, 40, 4)
    ts = _dataless(N, 6, W)
    ts.set_input_map(good)
    geometry = ts.input_map()
    w0, p0 = ts.predict(pixels=px)

    def still_good():
        assert ts.input_map() == geometry
        w, p = ts.predict(pixels=px)
        assert np.array_equal(w, w0) and np.array_equal(p, p0)

    t3 = good.table
    bad_nan = t3.copy()
    bad_nan[1234, 1] = np.nan
    bad_inf = t3.copy()
    bad_inf[-1, 0] = np.inf
    cases = [
        ("block", InputMap(13, 13, 0, 1, 1, 4, 4, t3)),
        ("block", InputMap(80, 80, 9, 0, 0, 4, 4, np.zeros((255 * 81 + 1, 2)))),
        ("ncodes", InputMap(13, 13, 3, 1, 1, 4, 4, t3[:-1])),
        ("out_rows", InputMap(13, 13, 3, 1, 1, 4, 3, t3)),
        ("row0", InputMap(13, 13, 3, 2, 1, 4, 4, t3)),       # 2 + 3 * 4 = 14 > 13 rows
        ("row0", InputMap(13, 13, 3, -1, 1, 4, 4, t3)),
        ("col0", InputMap(13, 13, 3, 1, 2, 4, 4, t3)),
        ("col0", InputMap(13, 12, 3, 1, 1, 4, 4, t3)),       # 1 + 3 * 4 = 13 > 12 columns
        ("table", InputMap(13, 13, 3, 1, 1, 4, 4, bad_nan)),
        ("table", InputMap(13, 13, 3, 1, 1, 4, 4, bad_inf)),
    ]
    for field, m in cases:
        with pytest.raises(TnmlError, match=field):
            ts.set_input_map(m)
        still_good()
    st = _lib.InputMapStruct(13, 13, 3, 1, 1, 4, 4, good.ncodes, None)           # table = NULL
    assert ts._L.tnml_set_input_map(ts._h, C.byref(st)) != 0
    assert "table" in ts._L.tnml_last_error(ts._h).decode()
    still_good()
    # the byte count of an image is checked in Python before the call
    for call in (lambda: ts.predict(pixels=px[:, :16]), lambda: ts.predict(pixels=np.zeros((3, 170), dtype=np.uint8)),
                 lambda: TrainStates(np.zeros(3, dtype=np.int32), N, 6, pixels=np.zeros((3, N), dtype=np.uint8), input_map=good)):
        with pytest.raises(ValueError, match="pixels must have shape"):
            call()
    still_good()
    ts.close()
    # a bond update in flight, and a context attached as a held-out set
    pixels, labels, phi, Wt = make_problem(16, 60, 4, 3, pixel_boost=200.0)
    tr = TrainStates(labels, 16, 4, phi=phi)
    tr.set_mps(Wt)
    tr.set_input_map(good)
    geometry = tr.input_map()
    w0, p0 = tr.predict(pixels=px)
    tr.init()
    tr.bond_update_begin(1, 1, 4, 2, 1e-10, 3, 1e-3, 1e-10)
    with pytest.raises(TnmlError, match="bond update is in flight"):
        tr.set_input_map(_map("13x13_b3_from_1", "normal"))
    with pytest.raises(TnmlError, match="bond update is in flight"):
        tr.set_input_map(None)
    tr.bond_update_end()
    assert tr.input_map() == geometry
    assert np.array_equal(tr.predict(pixels=px)[0], tr.predict(phi=good.features(px))[0])      # (W has moved: compared on the new W)
    tr.close()
    tr = TrainStates(labels, 16, 4, phi=phi)
    tr.set_mps(Wt)
    tr.init()
    hs = TrainStates(labels[:40], 16, 4, phi=phi[:40])
    hs.set_input_map(good)
    tr.attach_heldout(hs)
    with pytest.raises(TnmlError, match="attached as a held-out set"):
        hs.set_input_map(_map("13x13_b3_from_1", "normal"))
    with pytest.raises(TnmlError, match="attached as a held-out set"):
        hs.set_input_map(None)
    assert hs.input_map() == geometry
    tr.set_input_map(good)                                  # the training context itself may: the map touches neither W nor environments
    w, p = tr.predict(pixels=px)
    assert np.array_equal(w, w0) and np.array_equal(p, p0)
    tr.detach_heldout()
    hs.set_mps(Wt)
    w, p = hs.predict(pixels=px)                            # the map the held-out context had before the refusals is still the one in force
    assert np.array_equal(w, w0) and np.array_equal(p, p0)
    tr.close()
    hs.close()


# ---- workspace and launches ------------------------------------------------------------------------------------------------------
def _workspace(N, nl, maxm, C_, S, ncodes):
    M = (min(maxm, 512) + 15) // 16 * 16
    return 16 * N + 8 * nl * C_ + 4 * C_ + 8 * M * C_ + S * C_ + 2 * N * C_ + 16 * ncodes


def test_workspace_formula_and_launch_counts():
    a, b = _map("13x13_b3_from_1", "random"), _map("12x12_b2", "normal").with_table(_table("normal", 2))
    b.src_rows, b.src_cols, b.out_rows, b.out_cols = 10, 9, 4, 4        # another S (90) and another table size for the same N = 16
    N = a.N
    W = _mps_with_dims(_random_dims(N, 6, 3), 9)
    ts = _dataless(N, 6, W)
    ts.set_option("predict_chunk", 50)                      # C = 64
    before = ts.device_bytes()
    ts.set_input_map(a)
    assert ts.device_bytes() == before                      # allocated by the first predict, not by the map
    pa = _raw(a.S, 64, 1)
    w_small = ts.predict(pixels=pa)[0]
    small = ts.device_bytes()
    assert small - before == _workspace(N, 10, 6, 64, a.S, a.ncodes), (small - before, _workspace(N, 10, 6, 64, a.S, a.ncodes))
    ts.profile(True)
    ts.profile_reset()
    w_big = ts.predict(pixels=np.tile(pa, (100, 1)))[0]     # 6 400 images: 128 chunks of 50
    prof = ts.profile_read()
    ts.profile(False)
    assert ts.device_bytes() == small
    assert np.array_equal(w_big[:64], w_small) and np.array_equal(w_big[-64:], w_small)
    assert prof["chain"][0] == 128 and prof["pack"][0] == 128, prof
    assert all(v[0] == 0 for k, v in prof.items() if k.startswith("fgemm")), prof
    ts.set_input_map(b)                                     # released with the map it was sized for ...
    assert ts.device_bytes() < small
    pb = _raw(b.S, 64, 2)
    w = ts.predict(pixels=pb)[0]                            # ... and re-made by the next predict
    assert ts.device_bytes() - before == _workspace(N, 10, 6, 64, b.S, b.ncodes)
    assert np.array_equal(w, ts.predict(phi=b.features(pb))[0])
    ts.close()


# ---- drivers ---------------------------------------------------------------------------------------------------------------------
def _result_table(out):
    """the result table of fullTest as the evaluators print it"""
    lines = [l for l in out.splitlines() if re.search(r"\d+/\d+ correct", l) or l.startswith("Total # test images")]
    assert len(lines) >= 3, out[-1500:]
    return lines


def _run(exe, inp, cwd):
    cmd = [sys.executable, "-m", "tnml_amd.train"] if exe == "train" else [os.path.join(ROOT, "tnml_amd", exe)]
    run = subprocess.run(cmd + [str(inp)], capture_output=True, text=True, cwd=cwd, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    return run.stdout


def _idx_sets(tmp_path, per_label, ntest, seed):
    """8 x 8 images as idx files: (datadir, training pixels, test pixels, test labels)"""
    from tnml_amd import synth
    labels = synth.synthetic_labels(10 * per_label, seed=seed, per_label=per_label)
    tl = synth.synthetic_labels(ntest, seed=seed + 17)
    allpx = np.clip(synth.synthetic_images(64, np.concatenate([labels, tl]), seed=seed).astype(np.int32) * 3, 0, 255).astype(np.uint8)
    data = str(tmp_path / "data")
    synth.write_idx(data, allpx[:len(labels)], labels)
    synth.write_idx(data, allpx[len(labels):], tl, train=False)
    return data, allpx[:len(labels)], allpx[len(labels):], tl


MAP_LINE = "Input map: 8 x 8 bytes -> 4 x 4 sites (2 x 2 block sums from (0, 0)), feature = %s, 1021 codes"


def test_evaluators_with_input_map(tmp_path):
    """`fulltest` with feature = normal and `separate_fulltest`, both at imglen = 4 and predict = yes: input_map = yes prints the result
    table of input_map = no, the `Input map:` line, and tnml_predict_u8 as the device path"""
    from tnml_amd import hostlib
    data, _, tp, tl = _idx_sets(tmp_path, 16, 120, 6)
    hostlib.build_initial_w(data, 16, 3, 5, str(tmp_path / "W"), imglen=4)
    for L in range(10):
        (tmp_path / ("L%d" % L)).mkdir()
        hostlib.build_initial_single(data, 16, L, 3, 4, True, str(tmp_path / ("L%d" % L) / ("W%d" % L)), imglen=4)
    hostlib.write_sites(str(tmp_path / "sites"), 16)
    for exe, keys in (("fulltest", "fname = W\nfeature = normal\nprecision = f64\n"), ("separate_fulltest", "feature_scale = 1\n")):
        outs = {}
        for mode in ("no", "yes"):
            tin = tmp_path / ("input_%s_%s" % (exe, mode))
            tin.write_text("input\n{\ndatadir = %s\n%simglen = 4\npredict = yes\npredict_chunk = 50\ninput_map = %s\n}\n" % (data, keys, mode))
            outs[mode] = _run(exe, tin, tmp_path)
        assert _result_table(outs["yes"]) == _result_table(outs["no"]), exe
        assert "Total # test images = 120" in outs["yes"]
        assert len(set(re.findall(r"Digit \d (\d+)/", outs["yes"]))) >= 2                  # not the same count for every digit
        assert MAP_LINE % "normal" in outs["yes"] and "Input map" not in outs["no"]
        assert "Device path: streamed chain kernel (tnml_predict_u8), 50 images per chunk" in outs["yes"]
        assert "Device path: streamed chain kernel (tnml_predict_phi), 50 images per chunk" in outs["no"]
        assert outs["yes"].index("Input map:") < outs["yes"].index("Device path") < outs["yes"].index(_result_table(outs["yes"])[0])
        if exe == "separate_fulltest":                      # the same features bit for bit: the same overlaps, the same printed costs
            costs = {k: re.findall(r"Digit \d C = \S+", v) for k, v in outs.items()}
            assert len(costs["yes"]) == 10 and costs["yes"] == costs["no"]


@pytest.mark.parametrize("exe", ["fixedL", "single", "train"])
def test_training_drivers_with_input_map(tmp_path, exe):
    """one sweep at maxm 6 on 200 images, feature_scale = 255, imglen = 4: every Cost, Percent correct and After SVD line of the
    input_map = yes run is the line of the input_map = no run, and the written W files are the same bytes"""
    data, _, _, _ = _idx_sets(tmp_path, 20, 30, 9)
    wname = "W3" if exe == "single" else "W"
    outs, files = {}, {}
    for mode in ("no", "yes"):
        wd = tmp_path / mode
        wd.mkdir()
        tin = wd / "input"
        tin.write_text("input\n{\ndatadir = %s\nNtrain = 20\nNbatch = 4\nNsweep = 1\ncutoff = 1E-10\nmaxm = 6\nminm = 3\nninitial = 3\nlambda = 1E-3\n"
                       "Npass = 3\nseed = 5\nprecision = f64\nfeature_scale = 255\nimglen = 4\nlabel = 3\ninput_map = %s\n}\n" % (data, mode))
        outs[mode] = _run(exe, tin, wd)
        files[mode] = (wd / wname).read_bytes()
    pick = lambda out: [l for l in out.splitlines() if "Cost" in l or "Percent correct" in l or "After SVD" in l or " C = " in l]
    assert len(pick(outs["yes"])) >= 2 * 15 and pick(outs["yes"]) == pick(outs["no"])
    assert files["yes"] == files["no"] and len(files["yes"]) > 100
    assert MAP_LINE % ("normal" if exe == "single" else "series") in outs["yes"]
    assert "Input map" not in outs["no"]
    assert outs["yes"].index("Input map:") < outs["yes"].index("Projecting training states")
