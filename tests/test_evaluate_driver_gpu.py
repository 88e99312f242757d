"""`heldout = stream` in the drivers (fixedL, single, tnml_amd.train): the t10k images are evaluated by tnml_evaluate_* on the training
context itself -- no second context -- before the first sweep, after every sweep and after every `heldout_every`-th bond update.
Every training number must be that of the same run with heldout = no; the held-out numbers must be those of heldout = yes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, PER_LABEL, NHELD, NSWEEP = 16, 20, 60, 2
BONDS = 2 * (N - 1)                                              # bond updates per sweep
HELD_RE = r"^Held-out: Percent correct = ([0-9.]+)%, # incorrect = (\d+)/(\d+), Cost = ([0-9.]+)$"
BODY = ("feature_scale = 255\nNtrain = %d\nNbatch = 10\nNsweep = %d\ncutoff = 1E-10\nmaxm = 8\nminm = 4\nninitial = 4\nlambda = 1E-3\nNpass = 3\nseed = 3\n"
        % (PER_LABEL, NSWEEP))


class Runs:
    """runs of a driver on one small idx data set (4 x 4 images: 200 for training, 60 as the t10k set), each made once"""

    def __init__(self, top):
        from tnml_amd import synth
        self.top = top
        labels = synth.synthetic_labels(10 * PER_LABEL, seed=5, per_label=PER_LABEL)
        pixels = synth.synthetic_images(N, labels, seed=5)
        self.data = str(top / "data")
        synth.write_idx(self.data, pixels[np.argsort(labels, kind="stable")], np.sort(labels), side=4)
        tl = synth.synthetic_labels(NHELD, seed=21, per_label=NHELD // 10)
        synth.write_idx(self.data, synth.synthetic_images(N, tl, seed=21), tl, train=False, side=4)
        self.done = {}

    def __call__(self, name, extra, prog="fixedL"):
        if name in self.done:
            return self.done[name]
        wd = self.top / name
        wd.mkdir()
        (wd / "input").write_text("input\n{\ndatadir = %s\n%s%s}\n" % (self.data, BODY, extra))
        cmd = [sys.executable, "-m", "tnml_amd.train"] if prog == "train" else [os.path.join(ROOT, "tnml_amd", prog)]
        r = subprocess.run(cmd + ["input"], capture_output=True, text=True, cwd=wd, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        self.done[name] = (r.stdout, wd)
        return self.done[name]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("evaluate_driver"))


def _held(out):
    return re.findall(HELD_RE, out, re.M)


def _csv(wd):
    rows = (wd / "bonds.csv").read_text().splitlines()
    return rows[0].split(","), [r.split(",") for r in rows[1:]]


def _same_held_numbers(a, b):
    """two Held-out lines: the same counts, costs (printed with ten decimals) within the 1e-10 relative that tests/test_heldout_gpu.py
    allows between the follower and a full contraction, plus the last printed digit"""
    assert a[1:3] == b[1:3], (a, b)
    ca, cb = float(a[3]), float(b[3])
    assert abs(ca - cb) <= 1e-10 * max(abs(cb), 1.0) + 1.0001e-10, (a, b)


def test_stream_leaves_the_training_as_heldout_no_has_it(runs):
    st, ws = runs("stream", "heldout = stream\nbond_log = bonds.csv\n")
    no, wn = runs("no", "heldout = no\nbond_log = bonds.csv\n")
    hs, rs = _csv(ws)
    hn, rn = _csv(wn)
    assert hs[:len(hn)] == hn and hs[len(hn):] == ["heldout_cost", "heldout_ncorrect", "nheldout"]
    assert len(rs) == len(rn) == NSWEEP * BONDS
    seconds = hn.index("seconds")                               # (wall time: the one column that is not a training number)
    for a, b in zip(rs, rn):
        assert [x for k, x in enumerate(a[:len(hn)]) if k != seconds] == [x for k, x in enumerate(b) if k != seconds]
    assert (ws / "W").read_bytes() == (wn / "W").read_bytes()
    # the log: one line that names the mode, 1 + Nsweep Held-out lines, and nothing else on top of the run without
    assert "Held-out: streamed evaluation of %d images on the training context (tnml_evaluate_phi), before the first sweep and after every sweep\n" % NHELD in st
    extra = [ln for ln in st.splitlines() if ln.startswith("Held-out:")]
    assert len(extra) == 1 + 1 + NSWEEP and len(_held(st)) == 1 + NSWEEP
    assert [ln for ln in st.splitlines() if not ln.startswith("Held-out:")] == no.splitlines()
    lines = st.splitlines()
    assert lines[lines.index(next(ln for ln in lines if ln.startswith("Before starting DMRG Cost"))) + 1].startswith("Held-out: Percent")
    # bond_log: filled on the last row of each sweep, empty on the others
    for k, row in enumerate(rs, start=1):
        if k % BONDS == 0:
            assert int(row[-1]) == NHELD and int(row[-2]) == NHELD - int(_held(st)[k // BONDS][1]), row
        else:
            assert row[-3:] == ["", "", ""], row


def test_stream_reports_what_the_follower_reports(runs):
    st, _ = runs("stream", "heldout = stream\nbond_log = bonds.csv\n")
    yes, wy = runs("yes", "heldout = yes\nbond_log = bonds.csv\n")
    hy, hst = _held(yes), _held(st)
    assert len(hy) == 1 + NSWEEP * BONDS and len(hst) == 1 + NSWEEP
    assert all(int(h[2]) == NHELD for h in hst)
    for k, h in enumerate(hst):
        print("stream", h, "follower", hy[k * BONDS])
        _same_held_numbers(h, hy[k * BONDS])
    assert len({hy[k * BONDS][3] for k in range(1 + NSWEEP)}) == 1 + NSWEEP   # the cost moves from sweep to sweep: no comparison of a constant


def test_heldout_every_fills_the_rows_it_names(runs):
    ev, we = runs("every", "heldout = stream\nheldout_every = 5\nbond_log = bonds.csv\n")
    yes, wy = runs("yes", "heldout = yes\nbond_log = bonds.csv\n")
    no, wn = runs("no", "heldout = no\nbond_log = bonds.csv\n")
    assert "after every sweep and every 5 bond updates\n" in ev
    _, re_ = _csv(we)
    _, ry = _csv(wy)
    filled = [k for k, row in enumerate(re_, start=1) if row[-1] != ""]
    assert filled == [s * BONDS + i for s in range(NSWEEP) for i in range(1, BONDS + 1) if i % 5 == 0 or i == BONDS]
    for k in filled:                                            # the follower's row of the same bond update
        assert re_[k - 1][-2:] == ry[k - 1][-2:], k
        assert abs(float(re_[k - 1][-3]) - float(ry[k - 1][-3])) <= 1e-10 * float(ry[k - 1][-3]), k
    assert all(row[-3:] == ["", "", ""] for k, row in enumerate(re_, start=1) if k not in filled)
    assert len(_held(ev)) == 1 + len(filled)
    assert (we / "W").read_bytes() == (wn / "W").read_bytes()   # ending those bond updates early changes no training number


def test_two_ranks_sum_to_the_one_rank_numbers(runs):
    one, _ = runs("stream", "heldout = stream\nbond_log = bonds.csv\n")
    two, _ = runs("two", "heldout = stream\nngpu = 2\nshare_device = yes\n")
    assert "in-process communicator of 2 ranks" in two
    h1, h2 = _held(one), _held(two)
    assert len(h1) == len(h2) == 1 + NSWEEP
    assert [h[1:3] for h in h2] == [h[1:3] for h in h1]
    assert abs(float(h2[0][3]) - float(h1[0][3])) <= 1.0001e-10  # the same W before the first sweep: two shards against one
    np.testing.assert_allclose([float(h[3]) for h in h2], [float(h[3]) for h in h1], rtol=1e-6)   # (the trainings differ by the shards' summation order, as tests/test_multirank_one_gpu.py allows)


def test_python_driver_streams_too(runs):
    st, _ = runs("stream", "heldout = stream\nbond_log = bonds.csv\n")
    py, _ = runs("py", "heldout = stream\n", prog="train")
    assert "Held-out: streamed evaluation of %d images" % NHELD in py
    hp, hc = _held(py), _held(st)
    assert len(hp) == len(hc) == 1 + NSWEEP
    for a, b in zip(hp, hc):
        _same_held_numbers(a, b)


def test_single_driver_streams(runs):
    st, ws = runs("single_stream", "label = 3\nheldout = stream\nheldout_every = 7\n", prog="single")
    yes, _ = runs("single_yes", "label = 3\nheldout = yes\n", prog="single")
    no, wn = runs("single_no", "label = 3\nheldout = no\n", prog="single")
    assert (ws / "W3").read_bytes() == (wn / "W3").read_bytes()
    assert [ln for ln in st.splitlines() if not ln.startswith("Held-out:")] == no.splitlines()
    at = [0] + [s * BONDS + i for s in range(NSWEEP) for i in range(1, BONDS + 1) if i % 7 == 0 or i == BONDS]
    hs, hy = _held(st), _held(yes)
    assert len(hs) == len(at) and len(hy) == 1 + NSWEEP * BONDS
    for h, k in zip(hs, at):
        _same_held_numbers(h, hy[k])
