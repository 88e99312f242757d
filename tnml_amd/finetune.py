"""`python -m tnml_amd.finetune <inputfile>`: mini-batch fine-tuning of a trained W by gradient steps on the device
(tnml_site_step_u8 / tnml_site_step_phi), under the softmax cross-entropy of option loss = 1 or the quadratic cost.  One GPU.

Keys of the `input` group: datadir, Ntrain, Ntest, imglen, feature_scale, input_map as tnml_amd.train reads them (the images reach the
device in the form train.py takes for heldout = stream); infile (W) and outfile (W_ft); epochs (1), batch (256), optimizer = sgd | adam
(adam), lr, momentum, beta1, beta2, eps, clip; loss = quadratic | softmax (softmax), loss_beta (1); seed (1); log (none);
gradient_dtype = f64 | f32 (f64): the arithmetic of the gradient of every step (option gradient_dtype; f32: an fp32 gradient on the fp64
master W and optimiser state, bonds up to 1 024), named in the "Device path" line;
device_data = yes | no (no): with yes the training images and labels are uploaded once as torch tensors, every mini-batch is gathered
on the device and every step goes through tnml_site_step_dev, so that no image crosses the bus after the upload.  The numbers of a
run do not depend on the key; with yes one more line is printed, which says so.

W is read from infile into a context that holds no data, sized by W's largest bond.  The t10k set is evaluated before the first
epoch and after every epoch.  Epoch e (1-based) walks the permutation numpy.random.default_rng(seed + e).permutation(NT) in batches
(the last one short); a batch is ONE gradient_step with scale = 1 / its size.  After an epoch one line gives the mean batch cost per
image (from the step reports: the batch at the W before its step), the count of clipped steps and the held-out line.  W goes to
outfile at the end.  log = FILE: one CSV row per step, epoch, step, n, cost, ncorrect, grad_norm, factor, clipped, floats by repr."""
import sys

import numpy as np

LOG_HEADER = "epoch,step,n,cost,ncorrect,grad_norm,factor,clipped"


class BadInput(Exception):
    pass


def log_row(epoch, step, rep):
    """the CSV row of a StepReport"""
    return "%d,%d,%d,%r,%d,%r,%r,%d" % (epoch, step, rep.eval.n, rep.eval.cost, rep.eval.ncorrect, rep.grad_norm, rep.factor, int(rep.clipped))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        print("Usage: python -m tnml_amd.finetune inputfile")
        return 0
    try:
        return _run(argv[0])
    except BadInput as e:
        print(str(e), flush=True)
        return 1


def _run(inp):
    from . import hostlib
    from .fixedl import TnmlError, TrainStates

    def key(name, default, conv=str):
        v = hostlib.input_get(inp, name)
        if v is None:
            return default
        try:
            return conv(v.strip() if conv is str else v)
        except ValueError:
            raise BadInput("%s = %s: not a valid %s" % (name, v.strip(), "integer" if conv is int else "number"))

    def choice(name, default, allowed):
        v = key(name, default)
        if v not in allowed:
            raise BadInput("%s = %s: must be one of %s" % (name, v, " | ".join(allowed)))
        return v

    datadir = key("datadir", ".")
    Ntrain = key("Ntrain", 60000, int)
    Ntest = key("Ntest", 50000, int)
    imglen = key("imglen", 0, int)
    feature_scale = key("feature_scale", 1.0, float)
    infile, outfile = key("infile", "W"), key("outfile", "W_ft")
    epochs, batch, seed = key("epochs", 1, int), key("batch", 256, int), key("seed", 1, int)
    optimizer = choice("optimizer", "adam", ("sgd", "adam"))
    loss = choice("loss", "softmax", ("quadratic", "softmax"))
    loss_beta = key("loss_beta", 1.0, float)
    gradient_dtype = choice("gradient_dtype", "f64", ("f64", "f32"))
    lr = key("lr", None, float)
    par = dict(method=optimizer, lr=lr, momentum=key("momentum", 0.0, float), beta1=key("beta1", 0.9, float), beta2=key("beta2", 0.999, float),
               eps=key("eps", 1e-8, float), clip=key("clip", 0.0, float))
    logfile = key("log", None)
    if lr is None:
        raise BadInput("lr is required")
    if epochs < 0 or batch < 1:
        raise BadInput("epochs = %d, batch = %d: epochs must be >= 0 and batch >= 1" % (epochs, batch))
    try:
        use_map = hostlib.input_yesno(inp, "input_map", False)
        device_data = hostlib.input_yesno(inp, "device_data", False)
        px, lab, _ = hostlib.read_mnist(datadir, True, Ntrain)
        tpx, tlab, _ = hostlib.read_mnist(datadir, False, Ntest)
        W = hostlib.read_mps(infile)
    except (RuntimeError, OSError) as e:
        raise BadInput(str(e))

    # the input form, chosen as tnml_amd.train chooses it for heldout = stream
    imap = None
    if use_map:
        from .input_map import InputMap
        side = int(round(np.sqrt(px.shape[1])))
        try:
            if side * side != px.shape[1]:
                raise ValueError("reduce: image is not square")
            imap = InputMap.from_imglen(side, imglen if imglen > 0 else side, "series", feature_scale)
        except ValueError as e:
            raise BadInput(str(e))
        print(imap.describe())

    def images(p):
        v = hostlib.reduce(p, int(round(np.sqrt(p.shape[1]))), imglen) if imglen > 0 and imap is None else None
        if imap is not None or (v is None and feature_scale == 1.0):
            return "pixels", p
        g = (v if v is not None else p.astype(np.float64)) / 255.0
        return "phi", np.stack([np.ones_like(g), feature_scale * ((g / 255.0) / 4.0)], axis=-1)
    form, train = images(px)
    _, held = images(tpx)
    N = imap.N if imap is not None else train.shape[1]
    NT = len(lab)
    if len(W) != N or W[N // 2 - 1].ndim != 4:
        raise BadInput("Expected %s to have %d sites with the Label type Index at site %d" % (infile, N, N // 2))
    lab, tlab = np.asarray(lab, dtype=np.int32), np.asarray(tlab, dtype=np.int32)
    print("Fine-tuning %s: %d sites, largest bond %d; %d training images, %d held out; loss = %s%s, %s, lr = %r, batch = %d, %d epochs"
          % (infile, N, max(max(A.shape[0], A.shape[2]) for A in W), NT, len(tlab), loss, ", loss_beta = %r" % loss_beta if loss == "softmax" else "",
             optimizer, lr, batch, epochs), flush=True)

    ts = TrainStates(np.zeros(1, dtype=np.int32), N, max(max(A.shape[0], A.shape[2]) for A in W), no_data=True, input_map=imap)
    log = None
    try:
        ts.set_mps(W)
        ts.set_loss(loss, loss_beta)
        print("Device path: gradient steps on the device (tnml_site_step_%s), gradient_dtype = %s" % ("u8" if form == "pixels" else "phi", gradient_dtype), flush=True)

        def say_heldout():
            e = ts.evaluate(tlab, **{form: held})
            print("Held-out: Percent correct = %.4f%%, # incorrect = %d/%d, Cost = %.10f" % (e.ncorrect * 100.0 / e.n, e.n - e.ncorrect, e.n, e.cost / e.n), flush=True)
        say_heldout()
        if device_data:
            import torch
            print("device_data = yes: the training set lives on the device, batches are gathered there (tnml_site_step_dev)", flush=True)
            dev = torch.device("cuda", ts.device)
            train_d, lab_d = torch.from_numpy(np.ascontiguousarray(train)).to(dev), torch.from_numpy(lab).to(dev)
        if logfile:
            log = open(logfile, "w")
            log.write(LOG_HEADER + "\n")
        step = 0
        for epoch in range(1, epochs + 1):
            perm = np.random.default_rng(seed + epoch).permutation(NT)
            cost, clipped = 0.0, 0
            for at in range(0, NT, batch):
                rows = perm[at:at + batch]
                if device_data:
                    idx = torch.from_numpy(rows).to(dev)
                    rep = ts.gradient_step(labels=lab_d[idx], scale=1.0 / len(rows), **{form: train_d[idx]}, dtype=gradient_dtype, **par)
                else:
                    rep = ts.gradient_step(labels=lab[rows], scale=1.0 / len(rows), **{form: train[rows]}, dtype=gradient_dtype, **par)
                step += 1
                cost += rep.eval.cost / len(rows)
                clipped += int(rep.clipped)
                if log:
                    log.write(log_row(epoch, step, rep) + "\n")
            nb = -(-NT // batch)
            print("Epoch %d: mean batch cost per image = %.10f, clipped steps = %d/%d" % (epoch, cost / nb, clipped, nb), flush=True)
            say_heldout()
        hostlib.write_mps(outfile, ts.get_mps())
        print("Wrote %s" % outfile, flush=True)
    except TnmlError as e:
        raise BadInput(str(e))
    finally:
        if log:
            log.close()
        ts.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
