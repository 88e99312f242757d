"""The MPS as a differentiable torch layer: MPSFunction (a torch.autograd.Function) and MPSLayer (a torch.nn.Module) around a
TrainStates (tnml_amd/fixedl.py).

forward:  phi[n, N, 2] fp64 -> weights[n, nl], through TrainStates.predict();
backward: ONE TrainStates.backward(coef=grad_output, ..) call (tnml_backward_phi): the gradient for phi and, when the layer was made
          with train_sites=True, one gradient per site tensor.

Tensors cross the bus through host pointers, as every streamed call does: phi, grad_output and the site tensors are CPU tensors (or
are brought to the CPU here), the library stages them chunk by chunk and copies the results back.  Device-resident torch tensors
are not served.  W lives in the context; `layer.sites` mirrors it as fp64 CPU parameters shaped like get_site()'s, and a site whose
tensor has changed since its last upload (an optimiser step, a load_state_dict) is uploaded again with set_site() before the next
forward.

The two directions on numpy arrays, forward_arrays() and backward_arrays(), are plain functions of a TrainStates: the autograd
function only converts tensors and calls them."""
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


class MPSFunction(torch.autograd.Function):
    """apply(ts, phi, *sites): sites are the layer's parameters (or none).  They enter only so that autograd asks for their
    gradients; the numbers are those of W in the context ts, which the caller keeps equal to them (MPSLayer does)."""

    @staticmethod
    def forward(ctx, ts, phi, *sites):
        if phi.dtype != torch.float64:
            raise TypeError("MPSFunction: phi must be float64, got %s" % phi.dtype)
        x = phi.detach().cpu().contiguous().numpy()
        ctx.ts, ctx.x, ctx.nsites, ctx.device = ts, x, len(sites), phi.device
        return torch.from_numpy(forward_arrays(ts, x)).to(phi.device)

    @staticmethod
    def backward(ctx, grad_output):
        need_phi = ctx.needs_input_grad[1]
        need_sites = ctx.nsites > 0 and any(ctx.needs_input_grad[2:])
        if not (need_phi or need_sites):
            return (None, None) + (None,) * ctx.nsites
        go = grad_output.detach().cpu().contiguous().numpy()
        dphi, grads = backward_arrays(ctx.ts, ctx.x, go, need_sites, need_phi)
        gphi = torch.from_numpy(dphi).to(ctx.device) if need_phi else None
        gs = (None,) * ctx.nsites
        if need_sites:
            gs = tuple(torch.from_numpy(np.ascontiguousarray(g)) if ctx.needs_input_grad[2 + k] else None for k, g in enumerate(grads))
        return (None, gphi) + gs


class MPSLayer(torch.nn.Module):
    """phi[n, N, 2] -> weights[n, nl] of the MPS the context ts holds.  train_sites=True: `sites`, a ParameterList of fp64 CPU
    tensors shaped like get_site()'s, receives gradients and any torch optimiser can step it; False: W is fixed and only phi
    is differentiated."""

    def __init__(self, ts, train_sites=False):
        super().__init__()
        self.ts = ts
        self.train_sites = bool(train_sites)
        self.sites = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(ts.get_site(j))), requires_grad=self.train_sites) for j in range(1, ts.N + 1)])
        self._uploaded = [p._version for p in self.sites]

    def sync_sites(self):
        """upload every site whose tensor has changed since its last upload; -> the sites uploaded (1-based)"""
        done = []
        for k, p in enumerate(self.sites):
            if p._version != self._uploaded[k]:
                self.ts.set_site(k + 1, p.detach().numpy())
                self._uploaded[k] = p._version
                done.append(k + 1)
        return done

    def forward(self, phi):
        self.sync_sites()
        return MPSFunction.apply(self.ts, phi, *(tuple(self.sites) if self.train_sites else ()))
