"""The MPS as a differentiable torch layer: MPSFunction (a torch.autograd.Function) and MPSLayer (a torch.nn.Module) around a
TrainStates (tnml_amd/fixedl.py).

forward:  phi[n, N, 2] fp64 -> weights[n, nl], through TrainStates.predict();
backward: ONE TrainStates.backward(coef=grad_output, ..) call (tnml_backward_phi): the gradient for phi and, when the layer was made
          with train_sites=True, one gradient per site tensor.

Two paths, chosen by where phi lives.  A CPU phi (fp64) goes through host pointers, as the streamed calls always have: the library
stages it chunk by chunk and copies the results back.  A phi on the context's device (fp64 or fp32) goes through the device-resident
calls (tnml_predict_dev / tnml_backward_dev, include/tnml.h): the kernels read the tensor where it lies and write weights, the
gradient for phi (in phi's dtype) and the site gradients into device tensors; nothing is brought to the CPU and torch's stream is
not synchronised by the host on the way in (the library's stream waits for it through an event).
W lives in the context; `layer.sites` mirrors it as fp64 parameters shaped like get_site()'s -- CPU tensors, or with
MPSLayer(.., device=...) device tensors in the library's first-index-fastest layout -- and a site whose tensor has changed since its
last upload (an optimiser step, a load_state_dict) is uploaded again before the next forward: set_site() from the host, ONE
batched device-to-device upload of all of them (TrainStates.set_sites, tnml_set_sites_dev) from the device.

Taped forward (MPSLayer(.., taped=True); MPSFunction itself): when a gradient will be asked for and the batch fits one chunk of the
gradient workspace, the forward is TrainStates.forward_taped() and the backward TrainStates.backward_taped() on its ticket -- the
chain is walked inward once per step, not twice.  A ticket that is no longer the context's live one (another forward, a changed W)
falls back to the one backward() call; the numbers are the same bits either way.

The two directions on numpy arrays, forward_arrays() and backward_arrays(), are plain functions of a TrainStates: the autograd
function only converts tensors and calls them.

MPSLayer(.., compute_dtype="f32") computes in float32 (MPSFunction32): the forward runs under option predict_dtype = 1 and the backward
under gradient_dtype = 1, so that the weights the forward returns are those of the backward's own inward pass, bit for bit.  Both
options are put back after each call; the default "f64" is the path described above, unchanged."""
import threading

import numpy as np
import torch


def forward_arrays(ts, phi):
    """weights[n, nl] of phi[n, N, 2] through ts.predict()"""
    w, _ = ts.predict(phi=np.ascontiguousarray(phi, dtype=np.float64))
    return w


def backward_arrays(ts, phi, grad_output, want_sites, want_inputs=True):
    """one ts.backward() call with coef = grad_output[n, nl] -> (dphi[n, N, 2] | None, list of site gradients | None)"""
    grads, dphi = ts.backward(coef=np.ascontiguousarray(grad_output, dtype=np.float64), phi=np.ascontiguousarray(phi, dtype=np.float64),
                              want_sites=bool(want_sites), want_inputs=bool(want_inputs))
    return dphi, grads


class _option:
    """with _option(ts, name, value): the context option holds value inside the block and what it held before after it"""

    def __init__(self, ts, name, value):
        self.ts, self.name, self.value = ts, name, value

    def __enter__(self):
        self.old = self.ts.get_dtype_option(self.name)
        self.ts.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.ts.set_option(self.name, self.old)
        return False


_outer = threading.local()     # .grad: torch.is_grad_enabled() where this thread called apply() (forward() itself always runs with it off)


def _apply_noting_grad_mode(base_apply, args):
    before = getattr(_outer, "grad", True)
    _outer.grad = torch.is_grad_enabled()
    try:
        return base_apply(*args)
    finally:
        _outer.grad = before


def _use_tape(ctx, ts, phi):
    """the forward keeps its tape when something it is asked about needs a gradient (never under torch.no_grad()) and the batch is
    one chunk of the gradient workspace (1 <= n <= gradient_chunk)"""
    n = int(phi.shape[0])
    return getattr(_outer, "grad", True) and any(ctx.needs_input_grad[1:]) and 1 <= n <= ts.gradient_chunk()


def _forward(ctx, ts, phi, sites, taped):
    """the forward of both functions; taped: forward_taped() in predict()'s place, the ticket kept beside the saved x"""
    ctx.site_devices = [s.device for s in sites]
    ctx.on_device = phi.is_cuda and phi.device.index == ts.device and all(s.is_cuda and s.device == phi.device for s in sites)
    ctx.ticket = 0
    if ctx.on_device:
        if phi.dtype not in (torch.float64, torch.float32):
            raise TypeError("MPSFunction: phi must be float64 or float32 on the device, got %s" % phi.dtype)
        x = phi.detach().contiguous()
        ctx.ts, ctx.x, ctx.nsites, ctx.device = ts, x, len(sites), phi.device
        if taped:
            w, _, ctx.ticket = ts.forward_taped(phi=x)
            return w
        return ts.predict(phi=x)[0]
    if phi.dtype != torch.float64:
        raise TypeError("MPSFunction: phi must be float64, got %s" % phi.dtype)
    x = phi.detach().cpu().contiguous().numpy()
    ctx.ts, ctx.x, ctx.nsites, ctx.device = ts, x, len(sites), phi.device
    if taped:
        w, _, ctx.ticket = ts.forward_taped(phi=np.ascontiguousarray(x, dtype=np.float64))
        return torch.from_numpy(w).to(phi.device)
    return torch.from_numpy(forward_arrays(ts, x)).to(phi.device)


def _backward(ctx, grad_output):
    """the backward of both functions: backward_taped() while tape_ticket() still gives the forward's ticket, otherwise the one
    backward(coef = grad_output, phi = x) call, which gives the same bits"""
    need_phi = ctx.needs_input_grad[1]
    need_sites = ctx.nsites > 0 and any(ctx.needs_input_grad[2:])
    if not (need_phi or need_sites):
        return (None, None) + (None,) * ctx.nsites
    ts = ctx.ts
    taped = ctx.ticket > 0 and ts.tape_ticket()[0] == ctx.ticket
    if ctx.on_device:                                       # one device call, every result a device tensor
        coef = grad_output.detach().to(torch.float64)
        if taped:
            grads, gphi = ts.backward_taped(ctx.ticket, coef, want_sites=need_sites, want_inputs=need_phi, inputs32=ctx.x.dtype == torch.float32)
        else:
            grads, gphi = ts.backward(coef=coef, phi=ctx.x, want_sites=need_sites, want_inputs=need_phi)
        gs = (None,) * ctx.nsites
        if need_sites:
            gs = tuple(g if ctx.needs_input_grad[2 + k] else None for k, g in enumerate(grads))
        return (None, gphi) + gs
    go = grad_output.detach().cpu().contiguous().numpy()
    if taped:
        grads, dphi = ts.backward_taped(ctx.ticket, np.ascontiguousarray(go, dtype=np.float64), want_sites=need_sites, want_inputs=need_phi)
    else:
        dphi, grads = backward_arrays(ts, ctx.x, go, need_sites, need_phi)
    gphi = torch.from_numpy(dphi).to(ctx.device) if need_phi else None
    gs = (None,) * ctx.nsites
    if need_sites:
        gs = tuple(torch.from_numpy(np.ascontiguousarray(g)).to(ctx.site_devices[k]) if ctx.needs_input_grad[2 + k] else None for k, g in enumerate(grads))
    return (None, gphi) + gs


class MPSFunction(torch.autograd.Function):
    """apply(ts, phi, *sites): sites are the layer's parameters (or none).  They enter only so that autograd asks for their
    gradients; the numbers are those of W in the context ts, which the caller keeps equal to them (MPSLayer does).
    The device path is taken when phi lies on the context's device and every site passed does too (none passed: phi alone decides),
    so that every gradient comes back on the device of the tensor it belongs to.  Anything else -- a CPU phi, CPU parameters under
    a CUDA phi, a phi on another GPU -- takes the host path: phi goes through the CPU and each gradient returns to its tensor's
    device.
    The forward keeps its tape (TrainStates.forward_taped) when a gradient will be asked for and the batch is one chunk; the
    backward then starts from that tape while the context still holds its ticket.  MPSFunctionPlain never does."""

    @classmethod
    def apply(cls, *args):
        return _apply_noting_grad_mode(super().apply, args)

    @staticmethod
    def forward(ctx, ts, phi, *sites):
        return _forward(ctx, ts, phi, sites, _use_tape(ctx, ts, phi))

    @staticmethod
    def backward(ctx, grad_output):
        return _backward(ctx, grad_output)


class MPSFunctionPlain(torch.autograd.Function):
    """MPSFunction without the tape: predict() forward, one backward() call"""

    @staticmethod
    def forward(ctx, ts, phi, *sites):
        return _forward(ctx, ts, phi, sites, False)

    @staticmethod
    def backward(ctx, grad_output):
        return _backward(ctx, grad_output)


class MPSFunction32(torch.autograd.Function):
    """MPSFunction in float32 arithmetic: a taped forward and the backward run under gradient_dtype = 1, a forward without tape under
    predict_dtype = 1; each option is put back when its call returns, so other users of the context see it as they left it."""

    @classmethod
    def apply(cls, *args):
        return _apply_noting_grad_mode(super().apply, args)

    @staticmethod
    def forward(ctx, ts, phi, *sites):
        taped = _use_tape(ctx, ts, phi)
        with _option(ts, "gradient_dtype" if taped else "predict_dtype", 1):
            return _forward(ctx, ts, phi, sites, taped)

    @staticmethod
    def backward(ctx, grad_output):
        with _option(ctx.ts, "gradient_dtype", 1):
            return _backward(ctx, grad_output)


class MPSFunction32Plain(torch.autograd.Function):
    """MPSFunction32 without the tape"""

    @staticmethod
    def forward(ctx, ts, phi, *sites):
        with _option(ts, "predict_dtype", 1):
            return _forward(ctx, ts, phi, sites, False)

    @staticmethod
    def backward(ctx, grad_output):
        with _option(ctx.ts, "gradient_dtype", 1):
            return _backward(ctx, grad_output)


class MPSLayer(torch.nn.Module):
    """phi[n, N, 2] -> weights[n, nl] of the MPS the context ts holds.  train_sites=True: `sites`, a ParameterList of fp64
    tensors shaped like get_site()'s, receives gradients and any torch optimiser can step it; False: W is fixed and only phi
    is differentiated.
    device None (or a CPU device): the sites are CPU tensors, as ever; phi may be a CPU tensor or, when the layer sits between GPU
    modules, a CUDA tensor, which then goes through the CPU while the gradient for phi returns to phi's device.  A CUDA device (the context's): the sites are
    device parameters in the library's layout (first-index-fastest strides, filled by tnml_get_site_dev), phi is a tensor on that
    device, the optimiser steps on the device and sync_sites() uploads device to device.
    The place of the parameters is fixed when the layer is made: layer.to(...) / .cuda() / .cpu() between host and device is not
    supported (it would drop the strides the library reads); make a new layer instead.
    compute_dtype "f64" (the default) or "f32": the arithmetic of both directions (the module's header); the parameters stay fp64.
    taped=True: the forward keeps its tape and the backward starts from it (MPSFunction / MPSFunction32: one inward walk of the chain
    per step instead of two, the same bits); False (the default): predict() and one backward() call, as before the tape existed."""

    def __init__(self, ts, train_sites=False, device=None, compute_dtype="f64", taped=False):
        super().__init__()
        self.taped = bool(taped)
        if compute_dtype not in ("f64", "f32"):
            raise ValueError("MPSLayer: compute_dtype must be \"f64\" or \"f32\", got %r" % (compute_dtype,))
        self.compute_dtype = compute_dtype
        self.ts = ts
        self.train_sites = bool(train_sites)
        dev = torch.device(device) if device is not None else None
        self.on_device = dev is not None and dev.type == "cuda"
        if self.on_device:
            if dev.index is not None and dev.index != ts.device:
                raise ValueError("MPSLayer: device %s, the context is on device %d" % (dev, ts.device))
            tensors = ts.get_mps(device=True)
        else:
            tensors = [torch.from_numpy(np.ascontiguousarray(ts.get_site(j))) for j in range(1, ts.N + 1)]
        self.sites = torch.nn.ParameterList([torch.nn.Parameter(t, requires_grad=self.train_sites) for t in tensors])
        self._uploaded = [p._version for p in self.sites]

    def sync_sites(self):
        """upload every site whose tensor has changed since its last upload; -> the sites uploaded (1-based)"""
        done = [k + 1 for k, p in enumerate(self.sites) if p._version != self._uploaded[k]]
        if self.on_device and done:                         # ONE tnml_set_sites_dev call for all of them
            self.ts.set_sites(done, [self.sites[j - 1].detach() for j in done])
        for j in done:
            if not self.on_device:
                self.ts.set_site(j, self.sites[j - 1].detach().numpy())
            self._uploaded[j - 1] = self.sites[j - 1]._version
        return done

    def forward(self, phi):
        self.sync_sites()
        if self.compute_dtype == "f32":
            fn = MPSFunction32 if self.taped else MPSFunction32Plain
        else:
            fn = MPSFunction if self.taped else MPSFunctionPlain
        return fn.apply(self.ts, phi, *(tuple(self.sites) if self.train_sites else ()))
