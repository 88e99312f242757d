"""`python -m tnml_amd.finetune`: the driver of the gradient steps.  One run on a small idx data set (4 x 4 images, 30 per label for
training, 100 as the t10k set), W = synth.random_mps(16, 4), two epochs of Adam in batches of 64 under the softmax loss with a step log;
the test replays the run in-process through TrainStates with the same permutations."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, PER_LABEL, NHELD, EPOCHS, BATCH, SEED, LR, BETA = 16, 30, 100, 2, 64, 1, 3e-3, 16.0
HELD_RE = r"^Held-out: Percent correct = ([0-9.]+)%, # incorrect = (\d+)/(\d+), Cost = ([0-9.]+)$"
BODY = ("feature_scale = 255\nNtrain = %d\nNtest = %d\ninfile = W\noutfile = W_ft\nepochs = %d\nbatch = %d\noptimizer = adam\nlr = %r\nloss_beta = %r\nseed = %d\n"
        % (PER_LABEL, NHELD, EPOCHS, BATCH, LR, BETA, SEED))


def _features(p):
    g = p.astype(np.float64) / 255.0
    return np.stack([np.ones_like(g), 255.0 * ((g / 255.0) / 4.0)], axis=-1)          # feature_scale = 255, as the drivers form it


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from tnml_amd import hostlib, synth
    top = tmp_path_factory.mktemp("finetune_driver")
    labels = synth.synthetic_labels(10 * PER_LABEL, seed=5, per_label=PER_LABEL)
    pixels = synth.synthetic_images(N, labels, seed=5)
    pixels, labels = pixels[np.argsort(labels, kind="stable")], np.sort(labels)
    data = str(top / "data")
    synth.write_idx(data, pixels, labels, side=4)
    tl = synth.synthetic_labels(NHELD, seed=21, per_label=NHELD // 10)
    tp = synth.synthetic_images(N, tl, seed=21)
    synth.write_idx(data, tp, tl, train=False, side=4)
    W = synth.random_mps(N, 4, seed=7)
    return dict(top=top, data=data, W=W, hostlib=hostlib)


def _run(setup, name, extra):
    wd = setup["top"] / name
    wd.mkdir()
    setup["hostlib"].write_mps(str(wd / "W"), setup["W"])
    (wd / "input").write_text("input\n{\ndatadir = %s\n%s%s}\n" % (setup["data"], BODY, extra))
    r = subprocess.run([sys.executable, "-m", "tnml_amd.finetune", "input"], capture_output=True, text=True, cwd=wd, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    return r, wd


def test_the_run_is_the_replay_and_the_cost_falls(setup):
    """every CSV row equal by repr and W_ft bit for bit against a replay through TrainStates; the held-out cost after the last epoch
    at most 0.9 of the cost before the first.  lr = 3e-3 and loss_beta = 16 come from a replay of this run in the numpy models
    (sitegrad_model, loss_model, sitestep_model) on the CPU: the held-out cost per image went from 3.8149 to 2.4238, 0.635 of its
    start (loss_beta = 8: 0.857 at this lr; these images carry no label information, ln 10 = 2.3026 is the floor)"""
    from tnml_amd import finetune, hostlib
    from tnml_amd.fixedl import TrainStates
    r, wd = _run(setup, "run", "log = steps.csv\n")
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    print(r.stdout)
    held = re.findall(HELD_RE, r.stdout, re.M)
    assert len(held) == 1 + EPOCHS and all(int(h[2]) == NHELD for h in held)
    assert len(re.findall(r"^Epoch \d+: mean batch cost per image = [0-9.]+, clipped steps = 0/5$", r.stdout, re.M)) == EPOCHS
    assert float(held[-1][3]) <= 0.9 * float(held[0][3])
    # the replay
    px, lab, _ = hostlib.read_mnist(setup["data"], True, PER_LABEL)
    tpx, tlab, _ = hostlib.read_mnist(setup["data"], False, NHELD)
    phi, lab = _features(px), np.asarray(lab, dtype=np.int32)
    ts = TrainStates(np.zeros(1, dtype=np.int32), N, 4, no_data=True)
    ts.set_mps(hostlib.read_mps(str(wd / "W")))
    ts.set_loss("softmax", BETA)
    rows, step = [finetune.LOG_HEADER], 0
    for epoch in range(1, EPOCHS + 1):
        perm = np.random.default_rng(SEED + epoch).permutation(len(lab))
        for at in range(0, len(lab), BATCH):
            b = perm[at:at + BATCH]
            rep = ts.gradient_step(labels=lab[b], phi=phi[b], method="adam", lr=LR, scale=1.0 / len(b))
            step += 1
            rows.append(finetune.log_row(epoch, step, rep))
    assert step == EPOCHS * 5
    assert (wd / "steps.csv").read_text().splitlines() == rows
    e = ts.evaluate(np.asarray(tlab, dtype=np.int32), phi=_features(tpx))
    assert "%.10f" % (e.cost / e.n) == held[-1][3] and int(held[-1][1]) == e.n - e.ncorrect
    got, want = hostlib.read_mps(str(wd / "W_ft")), ts.get_mps()
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    ts.close()


def test_a_bad_key_value_ends_with_a_message(setup):
    r, _ = _run(setup, "nonsense", "loss = nonsense\n")
    assert r.returncode == 1
    assert "loss = nonsense: must be one of quadratic | softmax" in r.stdout
    assert "Traceback" not in r.stdout + r.stderr
