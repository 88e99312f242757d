"""The drivers' `heldout` / `Ntest` keys without a GPU: a bad value of the key and a missing t10k set are refused with a clear
message and exit status 1 before any context is created (the key before the training data is even read)."""
import os
import subprocess
import sys

import pytest

from tnml_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = ["fixedL", "single"]


def _input(tmp_path, datadir, extra):
    f = tmp_path / "input"
    f.write_text("input\n{\ndatadir = %s\nNtrain = 3\nNbatch = 1\nNsweep = 1\nmaxm = 4\nminm = 2\nninitial = 2\n%s}\n" % (datadir, extra))
    return str(f)


def _train_only(tmp_path):
    labels = synth.synthetic_labels(30, seed=5, per_label=3)
    d = str(tmp_path / "data")
    synth.write_idx(d, synth.synthetic_images(16, labels, seed=5), labels)
    return d


def _run(tmp_path, name, inp):
    if name == "train":
        cmd = [sys.executable, "-m", "tnml_amd.train", inp]
    else:
        cmd = [os.path.join(ROOT, "tnml_amd", name), inp]
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=120, env=env)


@pytest.mark.parametrize("name", DRIVERS + ["train"])
def test_heldout_key_must_be_yes_or_no(tmp_path, name):
    out = _run(tmp_path, name, _input(tmp_path, "/nonexistent/data", "heldout = maybe\n"))    # refused before the training data is read
    assert out.returncode == 1, out.stdout + out.stderr
    msg = out.stdout + out.stderr
    assert "heldout" in msg and "maybe" in msg, msg
    assert "train-images" not in msg


@pytest.mark.parametrize("name", DRIVERS)
def test_heldout_needs_the_t10k_set(tmp_path, name):
    d = _train_only(tmp_path)
    out = _run(tmp_path, name, _input(tmp_path, d, "heldout = yes\nNtest = 5\n"))
    assert out.returncode == 1, out.stdout + out.stderr
    assert "t10k-images-idx3-ubyte" in out.stderr, out.stdout + out.stderr
    assert "tnml_create" not in out.stderr
