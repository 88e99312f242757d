"""The torch layer on device tensors (tnml_amd/torch_layer.py: MPSFunction with a CUDA phi, MPSLayer(.., device=...)) and the
driver key device_data of `python -m tnml_amd.finetune`.  The yardstick is the CPU layer / the host path on the same values,
bit for bit: N = 12, m = 5, n = 17, and the bond class with 17 and 33."""
import numpy as np
import pytest
import torch

import inputgrad_model as im
import sitegrad_model as sm
import test_finetune_driver_gpu as fd
from test_finetune_driver_gpu import setup  # noqa: F401  (the module-scoped data set of the driver test)

pytestmark = pytest.mark.gpu


def _dataless(W):
    from tnml_amd.fixedl import TrainStates
    maxm = max(max(A.shape[0], A.shape[2]) for A in W)
    ts = TrainStates(np.zeros(1, dtype=np.int32), len(W), maxm, no_data=True)
    ts.set_mps(W)
    return ts


def _problem(kind):
    case = sm.small_case(12, 5, 17) if kind == "small" else sm.odd_case(0, 17)
    go = np.random.default_rng(2).standard_normal((17, 10))
    return case["W"], np.ascontiguousarray(case["phi"]), case["labels"], go


@pytest.mark.parametrize("kind", ["small", "odd0"])
def test_device_layer_equals_cpu_layer_through_an_sgd_step(kind):
    from tnml_amd.torch_layer import MPSLayer
    W, phi, labels, go = _problem(kind)
    a, b = _dataless(W), _dataless(W)
    cpu, dev = MPSLayer(a, train_sites=True), MPSLayer(b, train_sites=True, device="cuda")
    assert all(p.is_cuda and p.dtype == torch.float64 and p.stride() == b._fstrides(p.shape) for p in dev.sites)
    assert all(np.array_equal(p.detach().cpu().numpy(), A) for p, A in zip(dev.sites, W))
    xc = torch.tensor(phi, requires_grad=True)
    xd = torch.tensor(phi, device="cuda", requires_grad=True)
    oc, od = cpu(xc), dev(xd)
    assert od.is_cuda and torch.equal(od.cpu(), oc)
    (oc * torch.tensor(go)).sum().backward()
    (od * torch.tensor(go, device="cuda")).sum().backward()
    assert xd.grad.is_cuda and torch.equal(xd.grad.cpu(), xc.grad) and xc.grad.abs().max() > 0
    for k, (pc, pd) in enumerate(zip(cpu.sites, dev.sites)):
        assert pd.grad.is_cuda and torch.equal(pd.grad.cpu(), pc.grad) and pc.grad.abs().max() > 0, k
    # a power of two: lr * grad is exact, so a fused and an unfused p - lr * grad agree whatever the two optimiser kernels do
    lr = 2.0 ** np.floor(np.log2(1e-3 / max(float(p.grad.abs().max()) for p in cpu.sites)))
    oc_, od_ = torch.optim.SGD(cpu.parameters(), lr=lr), torch.optim.SGD(dev.parameters(), lr=lr)
    oc_.step(); od_.step()
    assert all(torch.equal(pd.detach().cpu(), pc.detach()) for pc, pd in zip(cpu.sites, dev.sites))
    with torch.no_grad():
        oc2, od2 = cpu(xc), dev(xd)
    assert sorted(dev.sync_sites()) == [] and torch.equal(od2.cpu(), oc2) and not torch.equal(oc2, oc)
    for j, p in enumerate(dev.sites, start=1):                                         # the context holds the stepped sites
        assert np.array_equal(b.get_site(j), p.detach().cpu().numpy())
    a.close(); b.close()


@pytest.mark.parametrize("train", [True, False])
def test_cpu_layer_under_a_cuda_phi_is_the_all_cpu_run(train):
    """the layer with CPU parameters between GPU modules: phi on the device goes through the CPU, phi.grad returns to the device, the
    site gradients stay with their CPU parameters; forward, backward and one SGD step against the run with everything on the CPU"""
    from tnml_amd.torch_layer import MPSLayer
    W, phi, labels, go = _problem("small")
    a, b = _dataless(W), _dataless(W)
    ref, mixed = MPSLayer(a, train_sites=train), MPSLayer(b, train_sites=train)
    assert not any(p.is_cuda for p in mixed.sites)
    xc = torch.tensor(phi, requires_grad=True)
    xd = torch.tensor(phi, device="cuda", requires_grad=True)
    oc, od = ref(xc), mixed(xd)
    assert od.is_cuda and torch.equal(od.cpu(), oc)
    (oc * torch.tensor(go)).sum().backward()
    (od * torch.tensor(go, device="cuda")).sum().backward()
    assert xd.grad.is_cuda and torch.equal(xd.grad.cpu(), xc.grad) and xc.grad.abs().max() > 0
    if train:
        for pc, pm in zip(ref.sites, mixed.sites):
            assert not pm.grad.is_cuda and torch.equal(pm.grad, pc.grad) and pc.grad.abs().max() > 0
        lr = 2.0 ** np.floor(np.log2(1e-3 / max(float(p.grad.abs().max()) for p in ref.sites)))
        torch.optim.SGD(ref.parameters(), lr=lr).step()
        torch.optim.SGD(mixed.parameters(), lr=lr).step()
        with torch.no_grad():
            oc2, od2 = ref(xc), mixed(xd)
        assert torch.equal(od2.cpu(), oc2) and not torch.equal(oc2, oc)
        assert all(np.array_equal(b.get_site(j), a.get_site(j)) for j in range(1, len(W) + 1))
    else:
        assert all(p.grad is None for p in mixed.sites)
    a.close(); b.close()


def test_euler_tie_on_the_device_layers_tensors():
    """sum_s phi[n, j, s] phi.grad[n, j, s] = sum_l grad_output[n, l] out[n, l] at every site (tests/inputgrad_model.py), on what the
    device layer returns"""
    from tnml_amd.torch_layer import MPSLayer
    case = sm.odd_case(0, 70)
    W, phi, coef = case["W"], case["phi"], case["coef"]
    ts = _dataless(W)
    ts.set_option("predict_tile", 64)
    layer = MPSLayer(ts, device="cuda")
    x = torch.tensor(phi, device="cuda", requires_grad=True)
    out = layer(x)
    out.backward(torch.tensor(coef, device="cuda"))
    assert x.grad.is_cuda and out.is_cuda
    _, _, bnd = im.model_of(case, "phi", "coef")
    _, w_abs, c_abs = im.abs_input_gradient(W, phi, coef=coef)
    K, U = im.rounding_count(len(W), 120, 10), 2.0 ** -53
    allowed = (np.abs(phi) * bnd).sum(axis=2) + K * U * (c_abs * w_abs).sum(axis=1)[:, None]
    got = (phi * x.grad.cpu().numpy()).sum(axis=2)
    want = (coef * out.detach().cpu().numpy()).sum(axis=1)[:, None]
    assert (np.abs(got - want) <= allowed).all()
    assert (allowed < 1e-6 * (c_abs * w_abs).sum(axis=1)[:, None]).all()
    ts.close()


def test_fp32_phi_gets_an_fp32_gradient_rounded_once():
    from tnml_amd.torch_layer import MPSLayer
    W, phi, labels, go = _problem("small")
    ts = _dataless(W)
    layer = MPSLayer(ts, device="cuda")
    x32 = torch.tensor(phi.astype(np.float32), device="cuda", requires_grad=True)
    x64 = x32.detach().double().requires_grad_(True)
    g = torch.tensor(go, device="cuda")
    o32, o64 = layer(x32), layer(x64)
    assert o32.dtype == torch.float64 and torch.equal(o32, o64)
    (o32 * g).sum().backward()
    (o64 * g).sum().backward()
    assert x32.grad.dtype == torch.float32 and x64.grad.dtype == torch.float64
    assert torch.equal(x32.grad, x64.grad.float()) and x32.grad.abs().max() > 0
    assert all(p.grad is None for p in layer.sites)
    ts.close()


def test_a_cross_entropy_step_on_the_device_lowers_the_loss():
    from tnml_amd.torch_layer import MPSLayer
    W, phi, labels, _ = _problem("small")
    ts = _dataless(W)
    layer = MPSLayer(ts, train_sites=True, device="cuda")
    opt = torch.optim.SGD(layer.parameters(), lr=1e-2)
    x, y = torch.tensor(phi, device="cuda"), torch.tensor(labels, device="cuda").long()
    loss = torch.nn.functional.cross_entropy(layer(x), y)
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert len(layer.sync_sites()) == len(W)
    with torch.no_grad():
        after = torch.nn.functional.cross_entropy(layer(x), y)
    assert float(after) < float(loss.detach())
    ts.close()


def test_driver_device_data_prints_the_same_numbers(setup):  # noqa: F811
    """`python -m tnml_amd.finetune` on the small input of tests/test_finetune_driver_gpu.py: device_data = yes against no.  Every
    line but the one that names the path is identical, the step logs and W_ft too"""
    from tnml_amd import hostlib
    r0, wd0 = fd._run(setup, "host_data", "log = steps.csv\n")
    r1, wd1 = fd._run(setup, "device_data", "log = steps.csv\ndevice_data = yes\n")
    assert r0.returncode == 0 and r1.returncode == 0, r0.stdout[-800:] + r0.stderr[-800:] + r1.stdout[-800:] + r1.stderr[-800:]
    l0, l1 = r0.stdout.splitlines(), r1.stdout.splitlines()
    extra = [ln for ln in l1 if ln.startswith("device_data = yes")]
    assert len(extra) == 1 and "tnml_site_step_dev" in extra[0]
    assert [ln for ln in l1 if ln not in extra] == l0
    assert sum(ln.startswith(("Held-out:", "Epoch ")) for ln in l0) == 1 + 2 * fd.EPOCHS
    assert (wd0 / "steps.csv").read_text() == (wd1 / "steps.csv").read_text()
    a, b = hostlib.read_mps(str(wd0 / "W_ft")), hostlib.read_mps(str(wd1 / "W_ft"))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
