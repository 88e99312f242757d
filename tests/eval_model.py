"""A numpy restatement of tnml_eval_report (include/tnml.h): what tnml_evaluate_u8 / tnml_evaluate_phi report, from a weights array
[n, nl] and the labels.  The decision rule is tnml_classify's (first maximum of |W_l|; w > 1/2 in the per-label variant), the targets
are y_nl = [l == label_n] (per-label variant: y_n = [label_n == target]), and label_cost[l] collects the images of true label l in both
modes, as the reports of training do.  The sums here are math.fsum of the same non-negative terms, so they are the reference for any
summation order."""
import math

import numpy as np

NL = 10
FIELDS = ("n", "ncorrect", "cost", "label_cost", "count", "nincorrect", "confusion")


def cost_bound(n, nl):
    """relative bound between a sum, in any order, of the k = n nl terms (w - y)^2 and math.fsum of the same terms.  The terms are the
    same bits on both sides (IEEE subtract and multiply, no contraction) and non-negative, so a sum in any order is off by less than
    (k - 1) 2^-53 of the exact sum; fsum adds one rounding."""
    return (n * nl + 3) * 2.0 ** -53


def predictions(w, target=None):
    w = np.asarray(w)
    if target is None:
        return np.abs(w).argmax(axis=1).astype(np.int32)           # first maximum
    return (w[:, 0] > (np.float32(0.5) if w.dtype == np.float32 else 0.5)).astype(np.int32)


def device_order_label_cost(w, labels, target=None, chunk=8192, threads=256):
    """label_cost in the summation order that the header of kernels_eval.hip states: per chunk, thread t takes images t, t + threads,
    ... in ascending order (an image's terms added in label order, then to the partial sum of its true label), a tree over the threads
    (element t += element t + stride, stride = threads / 2 ... 1), then the chunk's sums are added to the running totals"""
    w = np.asarray(w, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    y = np.eye(NL)[lab] if target is None else (lab == target).astype(np.float64)[:, None]
    d = w - y
    terms = d * d
    total = np.zeros(NL)
    for off in range(0, len(lab), chunk):
        s = np.zeros((threads, NL))
        for i in range(off, min(off + chunk, len(lab))):
            per = 0.0
            for x in terms[i].tolist():
                per += x
            s[(i - off) % threads, lab[i]] += per
        stride = threads // 2
        while stride > 0:
            s[:stride] += s[stride:2 * stride]
            stride //= 2
        total += s[0]
    return total


def report(w, labels, target=None):
    """dict with the fields of tnml_eval_report; target: the selected label of TNML_MODE_SINGLE (w is then [n, 1]), None: fixedL"""
    w = np.asarray(w, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    n = len(lab)
    assert w.shape == (n, 1 if target is not None else NL), w.shape
    assert n == 0 or (lab.min() >= 0 and lab.max() < NL)
    pred = predictions(w, target)
    if target is None:
        y = np.eye(NL)[lab] if n else np.zeros((0, NL))
        truth = lab
    else:
        y = (lab == target).astype(np.float64)[:, None]
        truth = (lab == target).astype(np.int64)
    d = w - y
    terms = d * d                                                   # [n, nl], each exact up to the two roundings the device makes too
    label_cost = np.array([math.fsum(terms[lab == l].ravel().tolist()) for l in range(NL)])
    wrong = pred != truth
    confusion = np.zeros((NL, NL), dtype=np.int64)
    np.add.at(confusion, (lab, pred), 1)
    return dict(n=n, ncorrect=int((~wrong).sum()), cost=math.fsum(terms.ravel().tolist()), label_cost=label_cost,
                count=np.bincount(lab, minlength=NL).astype(np.int64), nincorrect=np.bincount(lab[wrong], minlength=NL).astype(np.int64),
                confusion=confusion)
