"""Host-side mirror of the reference's fixedL interface on top of the C-ABI (include/tnml.h).

Names follow /root/reference/fixedL.cc so that parity tests read like the reference:
  TrainStates.{init,setBond,shiftE}   fixedL.cc:122-233   (device resident environments)
  quadcost / cgrad                    fixedL.cc:280-445
  mldmrg                              fixedL.cc:451-570   (sweep loop; one C call per bond update)
Tensors cross this layer as numpy arrays with ITensor index order as axis order:
A_j[a,s,r(,L)], B[a,s,t,r(,L)], E[n,m(,L)].  Everything here calls the HIP path; nothing falls
back to the CPU and nothing imports the oracle.
"""
import ctypes as C

import numpy as np
import torch

from . import lib as _lib

NL = _lib.NL


class TnmlError(RuntimeError):
    pass


class EvalReport:
    """tnml_eval_report as numpy values: n, ncorrect, cost, label_cost[10], count[10], nincorrect[10], confusion[10, 10] ([true][pred])"""
    FIELDS = ("n", "ncorrect", "cost", "label_cost", "count", "nincorrect", "confusion")

    def __init__(self, r):
        self.n, self.ncorrect, self.cost = int(r.n), int(r.ncorrect), float(r.cost)
        self.label_cost = np.array(r.label_cost[:], dtype=np.float64)
        self.count = np.array(r.count[:], dtype=np.int64)
        self.nincorrect = np.array(r.nincorrect[:], dtype=np.int64)
        self.confusion = np.array([row[:] for row in r.confusion], dtype=np.int64)

    def __eq__(self, other):
        return isinstance(other, EvalReport) and all(np.array_equal(getattr(self, f), getattr(other, f)) for f in self.FIELDS)

    __hash__ = None

    def __repr__(self):
        return "EvalReport(n=%d, ncorrect=%d, cost=%r)" % (self.n, self.ncorrect, self.cost)


class StepReport:
    """tnml_step_report: t (steps the optimiser state has taken, this one included), grad_norm (|scale| ||G||_2 over all sites),
    factor (what G was multiplied by), clipped, eval (an EvalReport: in the labels mode the batch at the W before the step, in the
    coef mode zero but for n)"""

    def __init__(self, r):
        self.t, self.grad_norm, self.factor, self.clipped = int(r.t), float(r.grad_norm), float(r.factor), bool(r.clipped)
        self.eval = EvalReport(r.eval)

    def __repr__(self):
        return "StepReport(t=%d, grad_norm=%r, factor=%r, clipped=%r, eval=%r)" % (self.t, self.grad_norm, self.factor, self.clipped, self.eval)


class TrainStates:
    """Training set + environments + W replica of one rank (TrainStates + MPS W of fixedL.cc)."""

    def __init__(self, labels, N, maxm, pixels=None, phi=None, device=0, rank=0, nranks=1, NT_total=None, dtype="f64",
                 single_label=None, svd_backend=0, no_data=False, input_map=None):
        """input_map: an InputMap (tnml_amd/input_map.py), set before the data: `pixels` is then [NT, input_map.S] raw bytes and the
        device does block sums, table look-up and transpose (tnml_set_input_map);
        no_data: a context for the MPS algebra alone (place / set_sum / compress / overlap): `labels` only sizes it (one entry will do);
        single_label = L selects the per-label variant (single.cc): plain weight MPS, target y_n = [l_n == L];
        svd_backend = 1: the split on stock rocsolver_dsyevd (TNML_SVD_ROCSOLVER) instead of the in-house eigensolver"""
        self._L = _lib.load()
        self._h = C.c_void_p()
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.NT = int(labels.shape[0])
        self.N = int(N)
        self.single = single_label is not None
        self.c0 = -1 if self.single else self.N // 2
        self.nl = 1 if self.single else NL
        self.maxm = int(maxm)
        self.rank, self.nranks = rank, nranks
        self.device = int(device)
        self.NT_total = int(NT_total if NT_total is not None else self.NT)
        self.dtype = dtype
        cfg = _lib.Config(device, rank, nranks, self.N, self.NT, self.NT_total, self.maxm, _lib.DTYPES[dtype], int(svd_backend),
                          1 if self.single else 0, int(single_label) if self.single else 0)
        self._cfg = cfg
        rc = self._L.tnml_create(C.byref(self._h), C.byref(cfg))
        if rc != 0:
            self._h = C.c_void_p()
            raise TnmlError(self._L.tnml_last_error(None).decode())
        self._bytes_per_image = self.N
        self._loss = "quadratic"
        self._last_chunk = None
        if input_map is not None:
            self.set_input_map(input_map)
        if pixels is not None:
            px = np.ascontiguousarray(pixels, dtype=np.uint8)
            if px.shape != (self.NT, self._bytes_per_image):
                raise ValueError("pixels must have shape %s, got %s" % ((self.NT, self._bytes_per_image), px.shape))
            self._ck(self._L.tnml_set_data_u8(self._h, px.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              labels.ctypes.data_as(C.POINTER(C.c_int32))))
        elif phi is not None:
            ph = np.ascontiguousarray(phi, dtype=np.float64)
            assert ph.shape == (self.NT, self.N, 2)
            self._ck(self._L.tnml_set_data_phi(self._h, _lib.dptr(ph), labels.ctypes.data_as(C.POINTER(C.c_int32))))
        elif not no_data:
            raise ValueError("need pixels or phi")

    # -- plumbing
    def _ck(self, rc):
        if rc != 0:
            raise TnmlError(self._L.tnml_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.tnml_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def comm_init(self, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, 128)
        self._ck(self._L.tnml_comm_init(self._h, buf))

    @staticmethod
    def comm_init_local(states, oneshot=False):
        """in-process communicator: ranks sharing one device through a staging buffer (tnml_comm_init_local), or -- oneshot --
        the peer-write all-reduce for the ranks of one process on any devices (tnml_comm_init_oneshot); afterwards drive every
        rank from its own host thread"""
        arr = (C.c_void_p * len(states))(*[s._h for s in states])
        f = _lib.load().tnml_comm_init_oneshot if oneshot else _lib.load().tnml_comm_init_local
        if f(arr, len(states)) != 0:
            raise TnmlError(_lib.load().tnml_last_error(None).decode() or "in-process communicator setup failed")

    def oneshot_export(self) -> bytes:
        """the cross-process one-shot all-reduce, step 1 (tnml_oneshot_export): allocates this rank's receive region and returns the
        64-byte IPC handle the other ranks need"""
        buf = C.create_string_buffer(64)
        self._ck(self._L.tnml_oneshot_export(self._h, buf))
        return buf.raw

    def oneshot_connect(self, handles):
        """step 2 (tnml_oneshot_connect): `handles` = the handles of ALL ranks in rank order (gathered over any control plane)"""
        blob = b"".join(handles)
        assert len(blob) == 64 * self.nranks, (len(blob), self.nranks)
        self._ck(self._L.tnml_oneshot_connect(self._h, C.create_string_buffer(blob, len(blob))))

    def oneshot_region_bytes(self):
        """bytes of the receive region oneshot_export allocates (not part of estimate_bytes)"""
        return int(self._L.tnml_oneshot_region_bytes(C.byref(self._cfg)))

    def oneshot_mem_kind(self):
        """memory kind of the receive region of the cross-process one-shot transport: 1 fine-grained, 2 uncached, 0 none"""
        return self._L.tnml_oneshot_mem_kind(self._h)

    def collective_mode(self):
        """0 none (one rank), 1 RCCL, 2 in-process staging buffer, 3 in-process one-shot peer write, 4 cross-process one-shot (IPC)"""
        return self._L.tnml_collective_mode(self._h)

    def allreduce_mode(self):
        return ("none", "rccl", "in-process staging buffer", "one-shot peer write (threads of one process)",
                "one-shot peer write (processes, IPC-mapped receive regions, device-side arrival flags)")[self.collective_mode()]

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        if _lib.load().tnml_comm_unique_id(buf) != 0:
            raise TnmlError("tnml_comm_unique_id failed")
        return buf.raw

    def replica_check(self):
        """collective: communicator size == nranks and bit-identical W replicas on every rank; returns the communicator size"""
        n = C.c_int()
        self._ck(self._L.tnml_replica_check(self._h, C.byref(n)))
        return n.value

    def replica_repairs(self):
        return self._L.tnml_replica_repairs(self._h)

    def collective_stats(self):
        """(sum all-reduces, broadcasts) this rank has entered so far"""
        a, b = C.c_int64(), C.c_int64()
        self._ck(self._L.tnml_collective_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_option(self, name, value):
        self._ck(self._L.tnml_set_option(self._h, name.encode(), int(value)))
        if name == "gradient_chunk":
            self._gchunk = int(value)
        elif name == "loss":
            self._loss = {v: k for k, v in _lib.LOSSES.items()}[int(value)]
        elif name in ("predict_dtype", "gradient_dtype"):
            self._dtypes = dict(getattr(self, "_dtypes", {}), **{name: int(value)})

    def get_dtype_option(self, name):
        """the value set_option() last gave "predict_dtype" or "gradient_dtype" on this object (0, the library's default, before any)"""
        return getattr(self, "_dtypes", {}).get(name, 0)

    def set_loss(self, loss="quadratic", beta=1.0):
        """options loss and loss_beta: the loss of evaluate() and of the labels mode of site_gradient() / gradient_step().
        "quadratic" (the default, the reference's cost) or "softmax": cross-entropy on the logits beta W_l (refused on a per-label
        context); beta must be finite and > 0.  Nothing else is touched: predict(), the coef mode, training."""
        if loss not in _lib.LOSSES:
            raise ValueError("loss must be one of %s, got %r" % (sorted(_lib.LOSSES), loss))
        self._ck(self._L.tnml_set_option_real(self._h, b"loss_beta", float(beta)))
        self.set_option("loss", _lib.LOSSES[loss])
        self._loss = loss

    @property
    def loss(self):
        """the loss set_loss() has set: "quadratic" or "softmax" """
        return self._loss

    def size(self):
        return self.NT

    def synchronize(self):
        self._ck(self._L.tnml_synchronize(self._h))

    def svd_stats(self):
        fb, cr, d0, d1 = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        self._ck(self._L.tnml_svd_stats(self._h, C.byref(fb), C.byref(cr), C.byref(d0), C.byref(d1)))
        return dict(fallbacks=fb.value, cluster_repairs=cr.value, dev_before_polish=d0.value, dev_after_first_polish=d1.value)

    def split_stats(self):
        """speculative splits so far, how many tnml_bond_update_end rolled back (failed deferred check), device ms of the repeated work"""
        a, b, ms = C.c_int64(), C.c_int64(), C.c_double()
        self._ck(self._L.tnml_split_stats(self._h, C.byref(a), C.byref(b), C.byref(ms)))
        return dict(speculative_splits=a.value, roll_backs=b.value, roll_back_ms=ms.value)

    def spec_predict_stats(self):
        """option spec_predict: splits that ran on a predicted column count, how many of them tnml_bond_update_end rolled back because
        the truncation rule kept another count, device ms of the work repeated for those (tnml_spec_predict_stats)"""
        a, b, ms = C.c_int64(), C.c_int64(), C.c_double()
        self._ck(self._L.tnml_spec_predict_stats(self._h, C.byref(a), C.byref(b), C.byref(ms)))
        return dict(predicted=a.value, mispredicted=b.value, redo_ms=ms.value)

    def truncate_device(self, evals_ascending, maxm, minm, cutoff, m_pred):
        """test entry (tnml_truncate_device): the device-side truncation rule on a host spectrum -> (kept count, count != m_pred)"""
        ev = np.ascontiguousarray(evals_ascending, dtype=np.float64)
        m, wrong = C.c_int(), C.c_int()
        self._ck(self._L.tnml_truncate_device(self._h, _lib.dptr(ev), len(ev), int(maxm), int(minm), float(cutoff), int(m_pred), C.byref(m), C.byref(wrong)))
        return m.value, wrong.value

    def shift_skip_stats(self, j):
        """site j (1..N): (16-image groups, groups of zero features only once each 64-image tile is walked zero features first) --
        the share of odd-row products the resident-operand shift leaves out (tnml_shift_skip_stats)"""
        a, b = C.c_int64(), C.c_int64()
        self._ck(self._L.tnml_shift_skip_stats(self._h, int(j), C.byref(a), C.byref(b)))
        return a.value, b.value

    def fwd_skip_stats(self, j):
        """site j (1..N): (16-image groups, groups of zero features only once each 32-image tile is walked zero features first) --
        the share of odd-row products the resident-operand forward pass leaves out (tnml_fwd_skip_stats)"""
        a, b = C.c_int64(), C.c_int64()
        self._ck(self._L.tnml_fwd_skip_stats(self._h, int(j), C.byref(a), C.byref(b)))
        return a.value, b.value

    def device_bytes(self):
        return self._L.tnml_device_bytes(self._h)

    def estimate_bytes(self):
        """tnml_estimate_bytes for this context's configuration: what the drivers plan maxm with (tnml_plan_maxm)"""
        return int(self._L.tnml_estimate_bytes(C.byref(self._cfg)))

    def classify(self):
        """toverlap / fullTest (util.h:19-40,123-200) over the local images: returns (weights[NT,10], pred[NT],
        count[10], nincorrect[10])."""
        w = np.zeros((self.NT, self.nl))
        pred = np.zeros(self.NT, dtype=np.int32)
        cnt = np.zeros(10, dtype=np.int64)
        ninc = np.zeros(10, dtype=np.int64)
        self._ck(self._L.tnml_classify(self._h, _lib.dptr(w), pred.ctypes.data_as(C.POINTER(C.c_int32)),
                                       cnt.ctypes.data_as(C.POINTER(C.c_int64)), ninc.ctypes.data_as(C.POINTER(C.c_int64))))
        return w, pred, cnt, ninc

    def set_input_map(self, m):
        """tnml_set_input_map: from now on set-data and predict calls that take bytes read m.S bytes per image and look the features of
        every block sum up in m.table; None: back to the built-in map.  Stored features are not touched."""
        if m is None:
            self._ck(self._L.tnml_set_input_map(self._h, None))
            self._bytes_per_image = self.N
            return
        table = np.ascontiguousarray(m.table, dtype=np.float64)
        st = _lib.InputMapStruct(m.src_rows, m.src_cols, m.block, m.row0, m.col0, m.out_rows, m.out_cols, int(table.shape[0]), _lib.dptr(table))
        self._ck(self._L.tnml_set_input_map(self._h, C.byref(st)))
        self._bytes_per_image = int(m.src_rows) * int(m.src_cols)

    def input_map(self):
        """tnml_get_input_map: the geometry of the map in force as a dict, or None without a map"""
        st = _lib.InputMapStruct()
        self._ck(self._L.tnml_get_input_map(self._h, C.byref(st)))
        if st.block == 0:
            return None
        return {k: getattr(st, k) for k in ("src_rows", "src_cols", "block", "row0", "col0", "out_rows", "out_cols", "ncodes")}

    def predict(self, pixels=None, phi=None, dtype=None):
        """streamed inference on images this context does not hold (tnml_predict_u8 / tnml_predict_phi): pixels[n, N] bytes
        (under an input map: [n, S] raw bytes) or phi[n, N, 2] features -> (weights[n, nl], pred[n]); pred is argmax_l |W_l|
        (per-label variant: [f > 1/2]).  Reads W only.  dtype "f64" / "f32" sets option predict_dtype for this call and the ones
        after it (None: leave it): "f32" runs the fp32 chain kernel, weights are its fp32 results widened.
        Device tensors: here and in evaluate / site_response / site_gradient / backward / gradient_step the arrays may be torch
        tensors on the context's device (all of a call's arrays, or none; phi float64 or float32).  The call then goes through the
        tnml_*_dev entry point on torch's current stream, nothing crosses the bus, the results are device tensors, and every number
        is bit for bit the host path's."""
        if self._on_device(pixels, phi):
            b, keep = self._dev_batch(pixels, phi, dtype=dtype)
            w, pred, o = self._weights(b.n, True, dev=True)
            self._ck(self._L.tnml_predict_dev(self._h, C.byref(b), C.byref(o)))
            return w, pred
        n, keep, (xp, _, _, _) = self._host_batch(pixels, phi, dtype=dtype)
        w, pred, (wp, pp) = self._weights(n, True)
        self._ck(self._entry("predict", pixels)(self._h, n, xp, wp, pp))
        return w, pred

    # -- device-resident arguments (the tnml_*_dev calls): torch tensors on the context's device, results as device tensors
    def _on_device(self, *arrays):
        """True when the array arguments of a streamed call are torch tensors on the context's device, False when none is a device
        tensor (numpy arrays and CPU tensors: the host-pointer path); a mix, or another device, is a ValueError"""
        given = [a for a in arrays if a is not None]
        dev = [isinstance(a, torch.Tensor) and a.is_cuda for a in given]
        if not any(dev):
            return False
        if not all(dev):
            raise ValueError("the array arguments of one call must all be device tensors, or none of them (%d of %d are)" % (sum(dev), len(dev)))
        for a in given:
            if a.device.index != self.device:
                raise ValueError("a tensor lies on device %s, the context is on device %d" % (a.device.index, self.device))
        return True

    def _dev_batch(self, pixels, phi, labels=None, coef=None, which=None, dtype=None):
        """-> (DevBatch, the tensors it points at): every array contiguous and of the call's dtype (made so on the device), phi
        float64 or float32, the stream torch's current one"""
        if (pixels is None) == (phi is None):
            raise ValueError("need exactly one of pixels or phi")
        self._set_dtype("predict_dtype", dtype)
        b = _lib.DevBatch()
        if pixels is not None:
            x = pixels.to(torch.uint8).contiguous()
            if x.ndim != 2 or x.shape[1] != self._bytes_per_image:
                raise ValueError("pixels must have shape [n, %d], got %s" % (self._bytes_per_image, tuple(x.shape)))
            b.pixels = x.data_ptr()
        else:
            x = (phi if phi.dtype in (torch.float64, torch.float32) else phi.to(torch.float64)).contiguous()
            if x.ndim != 3 or tuple(x.shape[1:]) != (self.N, 2):
                raise ValueError("phi must have shape [n, %d, 2], got %s" % (self.N, tuple(x.shape)))
            if x.dtype == torch.float32:
                b.phi32 = x.data_ptr()
            else:
                b.phi = x.data_ptr()
        n = int(x.shape[0])
        keep = [x]
        for name, a, dt, shape in (("labels", labels, torch.int32, (n,)), ("coef", coef, torch.float64, (n, self.nl)), ("which", which, torch.int32, (n,))):
            if a is None:
                continue
            a = a.to(dt).contiguous()
            if tuple(a.shape) != shape:
                raise ValueError("%s must have shape %s, got %s" % (name, list(shape), tuple(a.shape)))
            setattr(b, name, a.data_ptr())
            keep.append(a)
        b.n = n
        b.stream = torch.cuda.current_stream(x.device).cuda_stream
        return b, keep

    def _host_batch(self, pixels, phi, labels=None, coef=None, which=None, dtype=None):
        """the host path's _dev_batch -> (n, the arrays the pointers point at, (images, labels, coef, which) as ctypes pointers):
        every array contiguous and of the call's dtype, None where an array is absent; dtype (when given) becomes option predict_dtype"""
        if (pixels is None) == (phi is None):
            raise ValueError("need exactly one of pixels or phi")
        self._set_dtype("predict_dtype", dtype)
        if pixels is not None:
            x = np.ascontiguousarray(pixels, dtype=np.uint8)
            if x.ndim != 2 or x.shape[1] != self._bytes_per_image:
                raise ValueError("pixels must have shape [n, %d], got %s" % (self._bytes_per_image, x.shape))
        else:
            x = np.ascontiguousarray(phi, dtype=np.float64)
            assert x.ndim == 3 and x.shape[1:] == (self.N, 2), x.shape
        n = int(x.shape[0])
        keep, ptrs = [x], [x.ctypes.data_as(C.POINTER(C.c_uint8 if pixels is not None else C.c_double))]
        for name, a, dt, ct, shape in (("labels", labels, np.int32, C.c_int32, (n,)), ("coef", coef, np.float64, C.c_double, (n, self.nl)),
                                       ("which", which, np.int32, C.c_int32, (n,))):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=dt)
                if a.shape != shape:
                    raise ValueError("%s must have shape %s, got %s" % (name, list(shape), a.shape))
                keep.append(a)
            ptrs.append(None if a is None else a.ctypes.data_as(C.POINTER(ct)))
        return n, keep, ptrs

    def _entry(self, call, pixels):
        """the C entry of a streamed call for the input form given: tnml_<call>_u8 or tnml_<call>_phi"""
        return getattr(self._L, "tnml_%s_%s" % (call, "u8" if pixels is not None else "phi"))

    def _set_dtype(self, option, dtype):
        """dtype (when given) becomes option predict_dtype or gradient_dtype, for this call and the ones after it"""
        if dtype is not None:
            known = _lib.PREDICT_DTYPES if option == "predict_dtype" else _lib.GRADIENT_DTYPES
            if dtype not in known:
                raise ValueError("dtype must be one of %s, got %r" % (sorted(known), dtype))
            self.set_option(option, known[dtype])

    def _weights(self, n, want, dev=False):
        """the want_weights pair of a call on n images -> (weights | None, pred | None, where the library leaves them): on the host
        path their two ctypes pointers, on the device path (dev) a DevOut with both set; without want nothing is made or set"""
        if dev:
            o, where = _lib.DevOut(), torch.device("cuda", self.device)
            if not want:
                return None, None, o
            w, pred = torch.empty((n, self.nl), dtype=torch.float64, device=where), torch.empty(n, dtype=torch.int32, device=where)
            o.weights, o.pred = w.data_ptr(), pred.data_ptr()
            return w, pred, o
        if not want:
            return None, None, (None, None)
        w, pred = np.zeros((n, self.nl)), np.zeros(n, dtype=np.int32)
        return w, pred, (_lib.dptr(w), pred.ctypes.data_as(C.POINTER(C.c_int32)))

    def _gradient_buffer(self, dev=False):
        """a flat zero array (device: an empty tensor) for the gradient of every site, in the layout of tnml_site_gradient_*'s grad"""
        elems = C.c_int64()
        self._ck(self._L.tnml_site_gradient_size(self._h, C.byref(elems), None))
        if dev:
            return torch.empty(max(elems.value, 1), dtype=torch.float64, device=torch.device("cuda", self.device))
        return np.zeros(max(elems.value, 1))

    def _site_shape(self, j):
        ml, mr, hl = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.tnml_site_dims(self._h, j, ml, mr, hl))
        return (ml.value, 2, mr.value) + ((NL,) if hl.value else ())

    def _site_shapes(self):
        return [self._site_shape(j) for j in range(1, self.N + 1)]

    @staticmethod
    def _fstrides(shape):
        """first-index-fastest strides (elements) of a tensor of that shape: the library's layout of a site"""
        st, acc = [], 1
        for d in shape:
            st.append(acc)
            acc *= d
        return tuple(st)

    def _split_sites_dev(self, flat):
        """a flat device tensor in the layout of grad -> N strided views shaped like get_site()'s (no copy)"""
        out, at = [], 0
        for shape in self._site_shapes():
            out.append(torch.as_strided(flat, shape, self._fstrides(shape), at))
            at += int(np.prod(shape))
        return out

    def _backward_dev(self, labels, coef, pixels, phi, want_sites, want_inputs, want_weights):
        b, keep = self._dev_batch(pixels, phi, labels, coef)
        n = int(b.n)
        w, pred, o = self._weights(n, want_weights, dev=True)
        grad = dphi = None
        if want_sites:
            grad = self._gradient_buffer(dev=True)
            o.grad = grad.data_ptr()
        if want_inputs:
            f32 = phi is not None and keep[0].dtype == torch.float32
            dphi = torch.empty((n, self.N, 2), dtype=torch.float32 if f32 else torch.float64, device=torch.device("cuda", self.device))
            if f32:
                o.dphi32 = dphi.data_ptr()
            else:
                o.dphi = dphi.data_ptr()
        self._ck(self._L.tnml_backward_dev(self._h, C.byref(b), C.byref(o)))
        grads = self._split_sites_dev(grad) if want_sites else None
        self._note_chunk(n)
        return (grads, dphi, (w, pred)) if want_weights else (grads, dphi)

    def evaluate(self, labels, pixels=None, phi=None, dtype=None, want_weights=False):
        """streamed evaluation of labelled images this context does not hold (tnml_evaluate_u8 / tnml_evaluate_phi): the path of
        predict() plus one tally launch per chunk.  Returns an EvalReport (fields as tnml_eval_report: n, ncorrect, cost,
        label_cost[10], count[10], nincorrect[10], confusion[10, 10]); with want_weights (report, (weights[n, nl], pred[n])), both
        bit for bit those of predict().  Without it only the report leaves the device.  Reads W only.
        Under set_loss("softmax") cost and label_cost are the cross-entropy of the logits beta W_l, and ncorrect, nincorrect and
        confusion follow the signed decision (first maximum of W_l); weights and pred stay predict()'s (pred: first maximum of |W_l|)."""
        if self._on_device(pixels, phi, labels):
            b, keep = self._dev_batch(pixels, phi, labels, dtype=dtype)
            w, pred, o = self._weights(b.n, want_weights, dev=True)
            r = _lib.EvalReport()
            self._ck(self._L.tnml_evaluate_dev(self._h, C.byref(b), C.byref(o), C.byref(r)))
            return (EvalReport(r), (w, pred)) if want_weights else EvalReport(r)
        n, keep, (xp, lp, _, _) = self._host_batch(pixels, phi, labels, dtype=dtype)
        w, pred, (wp, pp) = self._weights(n, want_weights)
        r = _lib.EvalReport()
        self._ck(self._entry("evaluate", pixels)(self._h, n, xp, lp, C.byref(r), wp, pp))
        return (EvalReport(r), (w, pred)) if want_weights else EvalReport(r)

    def site_response(self, pixels=None, phi=None, which=None, want_weights=False):
        """streamed site responses (tnml_response_u8 / tnml_response_phi) of images this context does not hold, in the input forms of
        predict(): resp[n, N, 2], where resp[n, j, s] is the output of label which[n] for image n with the feature of site j + 1
        replaced by the unit vector e_s, so that the output for any replacement psi is psi @ resp[n, j].  which None: every image's
        own prediction.  With want_weights (resp, (weights[n, nl], pred[n])), both bit for bit those of predict() in fp64.  Reads W
        only; fp64 only (refused under predict_dtype = 1)."""
        if self._on_device(pixels, phi, which):
            b, keep = self._dev_batch(pixels, phi, which=which)
            w, pred, o = self._weights(b.n, want_weights, dev=True)
            resp = torch.empty((int(b.n), self.N, 2), dtype=torch.float64, device=torch.device("cuda", self.device))
            o.resp = resp.data_ptr()
            self._ck(self._L.tnml_response_dev(self._h, C.byref(b), C.byref(o)))
            return (resp, (w, pred)) if want_weights else resp
        n, keep, (xp, _, _, whp) = self._host_batch(pixels, phi, which=which)
        resp = np.zeros((n, self.N, 2))
        w, pred, (wp, pp) = self._weights(n, want_weights)
        self._ck(self._entry("response", pixels)(self._h, n, xp, whp, _lib.dptr(resp), wp, pp))
        return (resp, (w, pred)) if want_weights else resp

    def site_gradient(self, labels=None, coef=None, pixels=None, phi=None, want_weights=False, dtype=None):
        """streamed site gradients (tnml_site_gradient_u8 / tnml_site_gradient_phi) on images this context does not hold, in the input
        forms of predict(): a list of N arrays shaped like get_site()'s, G_j = sum_n sum_l c[n, l] dW_l(x_n)/dA_j.  Exactly one of
        coef[n, nl] (c as given) and labels[n] (c = 2 (W - y) with the targets of evaluate(): the gradient of the cost evaluate()
        reports).  With want_weights (grads, (weights[n, nl], pred[n])), both bit for bit those of predict() in fp64.  Reads W only;
        fp64 only (refused under predict_dtype = 1).
        Under set_loss("softmax") the labels mode forms c = beta (softmax(beta W) - y) on the device instead: the gradient of the
        cross-entropy evaluate() then reports.  The coef mode does not know the loss.
        dtype "f64" / "f32" sets option gradient_dtype for this call and the ones after it (None: as it is).  "f32": the fp32 gradient
        kernels on an fp32 copy of W, bonds up to 1 024; weights and pred are then those of predict(dtype="f32"), the sum over a chunk's
        images is fp32, the sum over chunks fp64."""
        self._set_dtype("gradient_dtype", dtype)
        if self._on_device(pixels, phi, labels, coef):
            r = self._backward_dev(labels, coef, pixels, phi, True, False, want_weights)
            return (r[0], r[2]) if want_weights else r[0]
        n, keep, (xp, lp, cp, _) = self._host_batch(pixels, phi, labels, coef)
        grad = self._gradient_buffer()
        w, pred, (wp, pp) = self._weights(n, want_weights)
        self._ck(self._entry("site_gradient", pixels)(self._h, n, xp, lp, cp, _lib.dptr(grad), wp, pp))
        grads = self._split_sites(grad)
        self._note_chunk(n)
        return (grads, (w, pred)) if want_weights else grads

    def backward(self, labels=None, coef=None, pixels=None, phi=None, want_sites=True, want_inputs=True, want_weights=False, dtype=None):
        """streamed backward pass (tnml_backward_u8 / tnml_backward_phi) in the input forms and the labels / coef rule of
        site_gradient(): -> (grads | None, dphi | None[, (weights, pred)]).  grads (want_sites) is site_gradient()'s list, bit for
        bit; dphi[n, N, 2] (want_inputs) is the gradient with respect to the features, dphi[n, j, s] = sum_l c[n, l] dW_l(x_n)/dphi[n, j, s]
        (under an input map: the features of the N reduced sites).  Without want_sites the gradient GEMM is not launched.  At least
        one of the two must be asked for.  Reads W only; fp64 only.
        Device tensors (every array argument a torch tensor on the context's device; tnml_backward_dev): grads are strided views
        of one flat device buffer, dphi a device tensor in phi's dtype (float32 phi: the fp64 result rounded once).
        dtype: as site_gradient()'s.  Under "f32" every dphi value is an fp32 number (widened exactly; a float32 dphi is rounded no
        second time)."""
        self._set_dtype("gradient_dtype", dtype)
        if self._on_device(pixels, phi, labels, coef):
            return self._backward_dev(labels, coef, pixels, phi, want_sites, want_inputs, want_weights)
        n, keep, (xp, lp, cp, _) = self._host_batch(pixels, phi, labels, coef)
        grad = self._gradient_buffer() if want_sites else None
        dphi = np.zeros((n, self.N, 2)) if want_inputs else None
        w, pred, (wp, pp) = self._weights(n, want_weights)
        self._ck(self._entry("backward", pixels)(self._h, n, xp, lp, cp, grad if grad is None else _lib.dptr(grad),
                                                 dphi if dphi is None else _lib.dptr(dphi), wp, pp))
        grads = self._split_sites(grad) if want_sites else None
        self._note_chunk(n)
        return (grads, dphi, (w, pred)) if want_weights else (grads, dphi)

    # -- backward from the forward's tape (tnml_forward_taped_* / tnml_backward_taped*)
    def forward_taped(self, pixels=None, phi=None, dtype=None):
        """predict() that keeps its tape (tnml_forward_taped_u8 / _phi / _dev): -> (weights[n, nl], pred[n], ticket).  Runs on the
        gradient workspace under option gradient_dtype (dtype "f64" / "f32" sets it, as backward()'s), one chunk at most
        (n <= gradient_chunk); weights and pred are bit for bit predict()'s under the matching predict_dtype.  ticket (> 0; 0 for
        n = 0) is what backward_taped() takes, and lives until something else uses the gradient workspace or writes W."""
        self._set_dtype("gradient_dtype", dtype)
        t = C.c_int64(0)
        if self._on_device(pixels, phi):
            b, keep = self._dev_batch(pixels, phi)
            w, pred, o = self._weights(b.n, True, dev=True)
            self._ck(self._L.tnml_forward_taped_dev(self._h, C.byref(b), C.byref(o), C.byref(t)))
            return w, pred, t.value
        n, keep, (xp, _, _, _) = self._host_batch(pixels, phi)
        w, pred, (wp, pp) = self._weights(n, True)
        self._ck(self._entry("forward_taped", pixels)(self._h, n, xp, wp, pp, C.byref(t)))
        return w, pred, t.value

    def tape_ticket(self):
        """tnml_tape_ticket: (the live ticket, its image count); (0, 0) when there is none"""
        t, n = C.c_int64(0), C.c_int64(0)
        self._ck(self._L.tnml_tape_ticket(self._h, C.byref(t), C.byref(n)))
        return t.value, n.value

    def backward_taped(self, ticket, coef, want_sites=True, want_inputs=True, inputs32=False):
        """backward(coef=coef, ..) on the images of forward_taped()'s ticket, from its tape (tnml_backward_taped / _dev): ->
        (grads | None, dphi | None), bit for bit backward()'s.  coef[n, nl]: a numpy array / CPU tensor (results as numpy arrays) or
        a tensor on the context's device (results as device tensors; inputs32: dphi as float32, the fp64 result rounded once, what
        backward() gives for a float32 phi) -- either serves a forward of either kind.  The ticket stays valid: another coef may follow."""
        n = int(coef.shape[0])
        if tuple(coef.shape) != (n, self.nl):
            raise ValueError("coef must have shape [n, %d], got %s" % (self.nl, tuple(coef.shape)))
        # the C call takes no n: it reads and writes the forward's image count.  A live ticket must therefore come with that many rows
        # (a ticket that is not the live one is refused by the library before it touches any array)
        live, n_live = self.tape_ticket()
        if live == int(ticket) and n != n_live:
            raise ValueError("coef has %d rows, the forward of ticket %d had %d images" % (n, live, n_live))
        if self._on_device(coef):
            where = torch.device("cuda", self.device)
            cf = coef.to(torch.float64).contiguous()
            o = _lib.DevOut()
            grad = dphi = None
            if want_sites:
                grad = self._gradient_buffer(dev=True)
                o.grad = grad.data_ptr()
            if want_inputs:
                f32 = bool(inputs32)
                dphi = torch.empty((n, self.N, 2), dtype=torch.float32 if f32 else torch.float64, device=where)
                if f32:
                    o.dphi32 = dphi.data_ptr()
                else:
                    o.dphi = dphi.data_ptr()
            self._ck(self._L.tnml_backward_taped_dev(self._h, int(ticket), cf.data_ptr(), C.byref(o), torch.cuda.current_stream(where).cuda_stream))
            self._last_chunk = n or self._last_chunk
            return (self._split_sites_dev(grad) if want_sites else None), dphi
        cf = np.ascontiguousarray(coef, dtype=np.float64)
        grad = self._gradient_buffer() if want_sites else None
        dphi = np.zeros((n, self.N, 2)) if want_inputs else None
        self._ck(self._L.tnml_backward_taped(self._h, int(ticket), _lib.dptr(cf), grad if grad is None else _lib.dptr(grad),
                                             dphi if dphi is None else _lib.dptr(dphi)))
        self._last_chunk = n or self._last_chunk
        return (self._split_sites(grad) if want_sites else None), dphi

    def _note_chunk(self, n):
        """the size of the last chunk of a gradient or step call on n images (gradient_coef)"""
        if n > 0:
            chunk = self._gradient_chunk()
            self._last_chunk = n - (n - 1) // chunk * chunk

    def _gradient_chunk(self):
        return getattr(self, "_gchunk", _lib.GRADIENT_CHUNK_DEFAULT)

    def gradient_chunk(self):
        """option gradient_chunk as set_option() last set it on this object (the library's default before any)"""
        return self._gradient_chunk()

    def gradient_coef(self, cnt=None):
        """test entry (tnml_site_gradient_coef): the coefficients [cnt, nl] of the last chunk of the last site_gradient() or
        gradient_step() call, as given (coef) or as the device formed them (labels).  cnt: that chunk's images (None: what this
        object has seen go by; another value is refused by the library)"""
        cnt = int(cnt) if cnt is not None else (self._last_chunk or 0)
        out = np.zeros((max(cnt, 1), self.nl))
        self._ck(self._L.tnml_site_gradient_coef(self._h, _lib.dptr(out), cnt * self.nl))
        return out[:cnt]

    def _split_sites(self, flat):
        """a flat array in the layout of tnml_site_gradient_*'s grad -> a list of N arrays shaped like get_site()'s"""
        out, at = [], 0
        for shape in self._site_shapes():
            size = int(np.prod(shape))
            out.append(flat[at:at + size].reshape(shape, order="F").copy(order="F"))
            at += size
        return out

    def gradient_step(self, labels=None, coef=None, pixels=None, phi=None, method="sgd", lr=None, momentum=0., beta1=.9, beta2=.999,
                      eps=1e-8, clip=0., scale=1., dtype=None):
        """one optimiser step on W on the device (tnml_site_step_u8 / tnml_site_step_phi): the gradient of site_gradient() on the same
        arguments, summed as site_gradient() sums it, multiplied by scale, clipped to the norm clip (0: not), then
        method "sgd": v <- momentum v + g, A <- A - lr v, or "adam" with beta1, beta2, eps and bias correction.  Neither the gradient
        nor W crosses the bus; returns a StepReport.  The optimiser state lives on the device, is made by the first step for its
        method and the shapes of W, and goes with step_reset().  Environments are stale afterwards, as after set_mps().
        Under set_loss("softmax") the labels mode takes the gradient of the cross-entropy and the report's eval is evaluate()'s under
        that loss; the optimiser and the coef mode are the same.
        dtype: as site_gradient()'s.  Under "f32" the step is mixed precision: an fp32 gradient on an fp64 master W and fp64 state."""
        self._set_dtype("gradient_dtype", dtype)
        if method not in _lib.STEP_METHODS:
            raise ValueError("method must be one of %s, got %r" % (sorted(_lib.STEP_METHODS), method))
        if lr is None:
            raise ValueError("lr is required")
        dev = self._on_device(pixels, phi, labels, coef)
        if dev:
            b, keep = self._dev_batch(pixels, phi, labels, coef)
            n = int(b.n)
        else:
            n, keep, (xp, lp, cp, _) = self._host_batch(pixels, phi, labels, coef)
        par = _lib.StepParams(_lib.STEP_METHODS[method], float(lr), float(momentum), float(beta1), float(beta2), float(eps), float(clip), float(scale))
        r = _lib.StepReport()
        if dev:
            self._ck(self._L.tnml_site_step_dev(self._h, C.byref(b), C.byref(par), C.byref(r)))
        else:
            self._ck(self._entry("site_step", pixels)(self._h, n, xp, lp, cp, C.byref(par), C.byref(r)))
        self._note_chunk(n)
        return StepReport(r)

    def step_reset(self):
        """tnml_site_step_reset: frees the optimiser state of gradient_step(); the next step starts from t = 1"""
        self._ck(self._L.tnml_site_step_reset(self._h))

    def step_state(self, which):
        """test entry (tnml_site_step_state): the optimiser state "m" (adam) or "v" (both methods) as a list of N arrays shaped like
        get_site()'s"""
        elems = C.c_int64()
        self._ck(self._L.tnml_site_gradient_size(self._h, C.byref(elems), None))
        buf = np.zeros(max(elems.value, 1))
        self._ck(self._L.tnml_site_step_state(self._h, which.encode(), _lib.dptr(buf), elems.value))
        return self._split_sites(buf)

    def descent_step(self, grads, cost_fn, step):
        """one step of gradient descent with backtracking, for contexts that hold no environments (a context that does must call
        init() again after W has changed): sets A_j - step G_j on every site as set_mps() does and halves step until cost_fn() is
        below its value at the W it started from; after 30 halvings without that it puts W back and raises TnmlError.  cost_fn takes
        no argument and reads this context's W, e.g. lambda: ts.evaluate(labels, pixels=x).cost.  Returns the step taken."""
        old = self.get_mps()
        if len(grads) != len(old) or any(np.shape(g) != A.shape for g, A in zip(grads, old)):
            raise ValueError("grads must be %d arrays shaped like get_mps()'s" % len(old))
        start = cost_fn()
        step = float(step)
        for _ in range(31):                                   # the step as given and at most 30 halvings
            self.set_mps([A - step * np.asarray(g, dtype=np.float64) for A, g in zip(old, grads)])
            if cost_fn() < start:
                return step
            step *= 0.5
        self.set_mps(old)
        raise TnmlError("descent_step: the cost did not fall below %.17g after 30 halvings of the step" % start)

    # -- W
    def set_mps(self, W):
        for j, A in enumerate(W, start=1):
            A = np.asarray(A, dtype=np.float64)
            self._ck(self._L.tnml_set_site(self._h, j, A.shape[0], A.shape[2], int(A.ndim == 4), _lib.dptr(_lib.flat(A))))

    def set_site(self, j, A):
        """A: a numpy array or CPU tensor (tnml_set_site), or a tensor on the context's device (tnml_set_site_dev: one
        device-to-device copy; a tensor that is not fp64 in first-index-fastest strides is first brought into that layout on the device)"""
        if self._on_device(A):
            shape = tuple(A.shape)
            if A.dtype != torch.float64 or A.stride() != self._fstrides(shape):
                A = torch.empty_strided(shape, self._fstrides(shape), dtype=torch.float64, device=A.device).copy_(A)
            self._ck(self._L.tnml_set_site_dev(self._h, j, shape[0], shape[2], int(len(shape) == 4), A.data_ptr(),
                                               torch.cuda.current_stream(A.device).cuda_stream))
            return
        A = np.asarray(A, dtype=np.float64)
        self._ck(self._L.tnml_set_site(self._h, j, A.shape[0], A.shape[2], int(A.ndim == 4), _lib.dptr(_lib.flat(A))))

    def set_sites(self, js, tensors):
        """set_site() for many sites at once, in the shapes W has now.  Tensors on the context's device go up in ONE call
        (tnml_set_sites_dev: one table upload, one copy launch, one synchronisation); a tensor that is not fp64 in
        first-index-fastest strides is first brought into that layout on the device, as set_site() does.  Host arrays take
        set_site() one by one."""
        js, tensors = [int(j) for j in js], list(tensors)
        if len(js) != len(tensors):
            raise ValueError("set_sites: %d sites, %d tensors" % (len(js), len(tensors)))
        if not js:
            return
        if not self._on_device(*tensors):
            for j, A in zip(js, tensors):
                self.set_site(j, A)
            return
        keep = []
        for j, A in zip(js, tensors):
            shape = tuple(A.shape)
            if 1 <= j <= self.N and shape != self._site_shape(j):
                raise ValueError("set_sites: site %d is %s in W, the tensor is %s (set_site() changes shapes)" % (j, self._site_shape(j), shape))
            if A.dtype != torch.float64 or A.stride() != self._fstrides(shape):
                A = torch.empty_strided(shape, self._fstrides(shape), dtype=torch.float64, device=A.device).copy_(A)
            keep.append(A)
        sites = (C.c_int32 * len(js))(*js)
        ptrs = (C.c_void_p * len(js))(*[A.data_ptr() for A in keep])
        self._ck(self._L.tnml_set_sites_dev(self._h, len(js), sites, ptrs, torch.cuda.current_stream(keep[0].device).cuda_stream))

    def get_site(self, j, device=False):
        """site j as a numpy array [ml, 2, mr(, 10)]; device=True: as a tensor on the context's device in first-index-fastest
        strides, the library's layout (tnml_get_site_dev: one device-to-device copy)"""
        shape = self._site_shape(j)
        if device:
            dev = torch.device("cuda", self.device)
            A = torch.empty_strided(shape, self._fstrides(shape), dtype=torch.float64, device=dev)
            self._ck(self._L.tnml_get_site_dev(self._h, j, A.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            return A
        buf = np.empty(int(np.prod(shape)))
        self._ck(self._L.tnml_get_site(self._h, j, _lib.dptr(buf)))
        return buf.reshape(shape, order="F")

    def get_mps(self, device=False):
        return [self.get_site(j, device) for j in range(1, self.N + 1)]

    # -- MPS algebra: the W0..W9 start (fixedL.cc:682-701,729)
    def place(self, j, ML, MR, row0, col0, A, label=-1):
        """tnml_mps_place: add the block A[ml,2,mr] at link offsets (row0, col0) of site j, shaped ML x 2 x MR (x 10 on site c0, where
        `label` names the slot) and zeroed by its first placement"""
        A = np.asarray(A, dtype=np.float64)
        assert A.ndim == 3 and A.shape[1] == 2, A.shape
        self._ck(self._L.tnml_mps_place(self._h, int(j), int(ML), int(MR), int(row0), int(col0), A.shape[0], A.shape[2], int(label), _lib.dptr(_lib.flat(A))))

    def set_sum(self, parts, labels=None):
        """the direct sum of `parts` (lists of Label-free site tensors A_j[l,2,r]) as this context's W, part k in label slot labels[k]
        on site c0 (default k): in.Aref(c) *= setElt(Lval(n)) and the block structure of sum(ipsis), fixedL.cc:693-697, before its truncation"""
        labels = list(range(len(parts))) if labels is None else list(labels)
        assert len(labels) == len(parts) and all(len(p) == self.N for p in parts)
        for j in range(1, self.N + 1):
            ML = 1 if j == 1 else sum(p[j - 1].shape[0] for p in parts)
            MR = 1 if j == self.N else sum(p[j - 1].shape[2] for p in parts)
            r0 = c0 = 0
            for p, lab in zip(parts, labels):
                A = p[j - 1]
                self.place(j, ML, MR, 0 if j == 1 else r0, 0 if j == self.N else c0, A, lab if j == self.c0 else -1)
                r0 += A.shape[0]
                c0 += A.shape[2]

    def compress(self, cutoff, maxm=0):
        """tnml_mps_compress (orthogonalize(args) behind sum(psis,args)); maxm = 0: no Maxm.  Call init() before using the environments again."""
        nb = self.N - 1
        newm = np.zeros(nb, dtype=np.int32)
        te = np.zeros(nb)
        rep = _lib.CompressReport()
        rep.newm = newm.ctypes.data_as(C.POINTER(C.c_int))
        rep.truncerr = _lib.dptr(te)
        self._ck(self._L.tnml_mps_compress(self._h, float(cutoff), int(maxm or 0), C.byref(rep)))
        return dict(maxm_before=rep.maxm_before, maxm_after=rep.maxm_after, truncerr_sum=rep.truncerr_sum, fallbacks=rep.fallbacks,
                    newm=[int(x) for x in newm], truncerr=te)

    def overlap(self):
        """overlap(W,W) on the device (tnml_mps_overlap)"""
        out = C.c_double()
        self._ck(self._L.tnml_mps_overlap(self._h, C.byref(out)))
        return out.value

    # -- TrainStates
    def init(self):
        self._ck(self._L.tnml_env_init(self._h))

    def setBond(self, b):
        self._ck(self._L.tnml_set_bond(self._h, b))

    def shiftE(self, b, from_left):
        self._ck(self._L.tnml_shift_env(self._h, b, int(bool(from_left))))

    def env_stats(self):
        """host tier of the environments (option env_budget_mb): copies to the host / back, slabs on the device, bytes on the host"""
        v = [C.c_int64() for _ in range(4)]
        self._ck(self._L.tnml_env_stats(self._h, *[C.byref(x) for x in v]))
        return dict(spills=v[0].value, fetches=v[1].value, slabs=v[2].value, host_bytes=v[3].value)

    def env(self, j):
        m, hl = C.c_int(), C.c_int()
        self._ck(self._L.tnml_env_dims(self._h, j, m, hl))
        L = NL if hl.value else 1
        buf = np.empty((self.NT, m.value * L))
        self._ck(self._L.tnml_get_env(self._h, j, _lib.dptr(buf)))
        if hl.value:
            return buf.reshape(self.NT, NL, m.value).transpose(0, 2, 1).copy()
        return buf

    # -- bond tensor and per-image contractions
    def bond_shape(self, b):
        mL, mR, lab = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.tnml_bond_dims(self._h, b, mL, mR, lab))
        return (mL.value, 2, 2, mR.value) + ((NL,) if lab.value else ())

    def bond_tensor(self, b):
        shape = self.bond_shape(b)
        buf = np.empty(int(np.prod(shape)))
        self._ck(self._L.tnml_bond_tensor(self._h, b, _lib.dptr(buf)))
        return buf.reshape(shape, order="F")

    def forward(self, B):
        P = np.empty((self.NT, self.nl))
        self._ck(self._L.tnml_forward(self._h, _lib.dptr(_lib.flat(B)), _lib.dptr(P)))
        return P[:, 0] if self.single else P

    def gradient(self, B):
        G = np.empty(B.size)
        self._ck(self._L.tnml_gradient(self._h, _lib.dptr(_lib.flat(B)), _lib.dptr(G)))
        return G.reshape(B.shape, order="F")

    def quadcost(self, B, lam):
        lc = np.empty(NL)
        cost, cr, nc = C.c_double(), C.c_double(), C.c_int64()
        self._ck(self._L.tnml_quadcost(self._h, _lib.dptr(_lib.flat(B)), lam, C.byref(cost), _lib.dptr(lc),
                                       C.byref(cr), C.byref(nc)))
        return cost.value, lc, cr.value, nc.value

    def pAp(self, p, lam):
        """sum_n |p*t.v_n|^2 + lambda |p|^2 (fixedL.cc:394-403)"""
        out = C.c_double()
        self._ck(self._L.tnml_pAp(self._h, _lib.dptr(_lib.flat(p)), lam, C.byref(out)))
        return out.value

    def cgrad(self, B, npass, lam, cconv):
        buf = _lib.flat(B)
        tr = _lib.CgTrace()
        self._ck(self._L.tnml_cgrad(self._h, _lib.dptr(buf), npass, lam, cconv, C.byref(tr)))
        return buf.reshape(B.shape, order="F"), _trace_dict(tr)

    def cg_state(self, which, shape=None):
        """test entry (tnml_cg_state): what the last cgrad left on the device.  "R", "Pv", "G": the fp64 CG vectors in the shape of the bond
        tensor (`shape`: that of the B given to cgrad); "P", "Pp", "dP": [NT padded, nl], padded rows included"""
        if which in ("R", "Pv", "G"):
            buf = np.empty(int(np.prod(shape)))
            self._ck(self._L.tnml_cg_state(self._h, which.encode(), _lib.dptr(buf), buf.size))
            return buf.reshape(shape, order="F")
        NTp = -(-self.NT // 256) * 256
        buf = np.empty((NTp, self.nl))
        self._ck(self._L.tnml_cg_state(self._h, which.encode(), _lib.dptr(buf), buf.size))
        return buf

    def exact(self, b, lam, pcut=1e-8):
        """single.h:117-160 on the bond chosen by setBond(b) (per-label variant): the solved bond tensor"""
        shape = self.bond_tensor(b).shape
        buf = np.zeros(int(np.prod(shape)))
        self._ck(self._L.tnml_exact(self._h, _lib.dptr(buf), lam, pcut))
        return buf.reshape(shape, order="F")

    def pinv(self, b, V0, npass, lam, pcut=1e-8):
        """single.h:404-517 on the bond chosen by setBond(b) from the start V0 [D, r]: (B, trace of V*E, singular values of the last E)"""
        shape = self.bond_tensor(b).shape
        V0 = np.asfortranarray(V0, dtype=np.float64)
        D, r = V0.shape
        assert D == int(np.prod(shape))
        B = np.zeros(D); ve = np.zeros(npass + 1); Dsv = np.zeros(r); done = C.c_int()
        self._ck(self._L.tnml_pinv(self._h, _lib.dptr(V0), r, npass, lam, pcut, _lib.dptr(B), _lib.dptr(ve), C.byref(done), _lib.dptr(Dsv)))
        return B.reshape(shape, order="F"), ve[:done.value + 1].copy(), Dsv

    def set_option_real(self, name, value):
        self._ck(self._L.tnml_set_option_real(self._h, name.encode(), float(value)))

    def svd_split(self, B, b, ha, cutoff, maxm, minm):
        te, m, nsv = C.c_double(), C.c_int(), C.c_int()
        sv = np.empty(4 * self.maxm + 8)
        self._ck(self._L.tnml_svd_split(self._h, _lib.dptr(_lib.flat(B)), b, ha, cutoff, maxm, minm, C.byref(te),
                                        C.byref(m), _lib.dptr(sv), C.byref(nsv)))
        return m.value, te.value, sv[:nsv.value].copy()

    def bond_update(self, b, ha, maxm, minm, cutoff, npass, lam, cconv, lam_cost=None, report_costs=False):
        sp = _lib.SweepParams(maxm, minm, cutoff, npass, lam, lam if lam_cost is None else lam_cost, cconv, int(report_costs))
        rep = _lib.BondReport()
        self._ck(self._L.tnml_bond_update(self._h, b, ha, C.byref(sp), C.byref(rep)))
        return self._report(rep)

    def bond_update_begin(self, b, ha, maxm, minm, cutoff, npass, lam, cconv, lam_cost=None, report_costs=False):
        """enqueue one bond update; the report comes from bond_update_end (at most two bond updates in flight)"""
        sp = _lib.SweepParams(maxm, minm, cutoff, npass, lam, lam if lam_cost is None else lam_cost, cconv, int(report_costs))
        self._ck(self._L.tnml_bond_update_begin(self._h, b, ha, C.byref(sp)))

    def bond_update_end(self):
        rep = _lib.BondReport()
        self._ck(self._L.tnml_bond_update_end(self._h, C.byref(rep)))
        return self._report(rep)

    @staticmethod
    def _report(rep):
        return dict(bond=rep.bond, half=rep.half, c=rep.c, mL=rep.mL, mR=rep.mR, label_on_B=bool(rep.label_on_B), origm=rep.origm, newm=rep.newm, truncerr=rep.truncerr,
                    norm_newB=rep.norm_newB, diff=rep.diff_B_newB, cost=rep.cost_after_svd,
                    label_cost=np.array(rep.label_cost[:]), reg_cost=rep.reg_cost, ncorrect=rep.ncorrect,
                    cg=_trace_dict(rep.cg), cost_old=rep.cost_old, cost_cg=rep.cost_cg, reg_cost_cg=rep.reg_cost_cg, norm_oB=rep.norm_oB)

    # -- held-out evaluation during training
    def attach_heldout(self, other):
        """tnml_heldout_attach: `other` (a TrainStates of the held-out images, one rank) follows every bond update of this context;
        allowed at a sweep start only.  `other` is locked until detach_heldout (or until either context is closed)."""
        self._ck(self._L.tnml_heldout_attach(self._h, other._h))
        self._heldout = other                     # (keeps the held-out context alive while attached)

    def detach_heldout(self):
        self._ck(self._L.tnml_heldout_detach(self._h))
        self._heldout = None

    def heldout_report(self):
        """held-out values after the last bond update ended (bond = 0: at attach): bond, half, count, ncorrect, cost
        (sum over images and labels of (W_l(x_n) - y_nl)^2, un-normalised, no regulariser) and label_cost[10]"""
        r = _lib.HeldoutReport()
        self._ck(self._L.tnml_heldout_read(self._h, C.byref(r)))
        return dict(bond=r.bond, half=r.half, count=r.count, ncorrect=r.ncorrect, cost=r.cost, label_cost=np.array(r.label_cost[:]))

    # -- measurement
    def profile(self, on, only=None):
        """HIP-event timing of kernel launches; `only` restricts it to one kernel class"""
        self._ck(self._L.tnml_profile_select(self._h, (only or "").encode()))
        self._ck(self._L.tnml_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._ck(self._L.tnml_profile_reset(self._h))

    def profile_read(self):
        out = {}
        name = C.create_string_buffer(64)
        for i in range(self._L.tnml_profile_count(self._h)):
            n, ms = C.c_int64(), C.c_double()
            self._ck(self._L.tnml_profile_get(self._h, i, name, C.byref(n), C.byref(ms)))
            out[name.value.decode()] = (n.value, ms.value)
        return out


def _trace_dict(tr):
    n = tr.npass_done
    k = n if tr.converged else max(n - 1, 0)
    return dict(npass_done=n, converged=bool(tr.converged), skipped=tr.converged == 2, cost=list(tr.cost[:k]), rnorm=list(tr.rnorm[:k]),
                pAp=list(tr.pAp[:n]), alpha=list(tr.alpha[:n]))


def quadcost(B, ts, lam=0.0):
    """fixedL.cc:280-344: returns the un-normalised cost C = sum_l C_l + lambda|B|^2"""
    return ts.quadcost(B, lam)[0]


def cgrad(B, ts, npass=4, lam=0.0, cconv=1e-10):
    """fixedL.cc:349-445"""
    return ts.cgrad(B, npass, lam, cconv)


def mldmrg(ts, nsweep, maxm, minm, cutoff, npass, lam, cconv, max_bonds=0, log=None, report_costs=False, pipelined=False, heldout=None):
    """fixedL.cc:451-570 (single.h:523-728 for a per-label TrainStates): the sweep loop; emits the reference's log lines
    through `log` if given.  pipelined: bond k+1 is enqueued before the report of bond k is fetched (same results, no idle
    GPU between bond updates; the log of a bond appears one bond later).  heldout: a TrainStates of held-out images, attached
    for the run (ts must be at a sweep start) and detached after it; every record gets a "heldout" entry (heldout_report())."""
    if heldout is not None:
        ts.attach_heldout(heldout)
        try:
            return _mldmrg(ts, nsweep, maxm, minm, cutoff, npass, lam, cconv, max_bonds, log, report_costs, pipelined, True)
        finally:
            ts.detach_heldout()
    return _mldmrg(ts, nsweep, maxm, minm, cutoff, npass, lam, cconv, max_bonds, log, report_costs, pipelined, False)


def _mldmrg(ts, nsweep, maxm, minm, cutoff, npass, lam, cconv, max_bonds, log, report_costs, pipelined, with_heldout):
    NT = float(ts.NT_total)
    reports = []
    if pipelined and not log:
        sched = []
        for sw in range(1, nsweep + 1):
            b, ha = 1, 1
            while ha <= 2:
                sched.append((sw, b, ha))
                b, ha = _lib.sweepnext(b, ha, ts.N)
        if max_bonds:
            sched = sched[:max_bonds]
        for k, (sw, b, ha) in enumerate(sched):
            ts.bond_update_begin(b, ha, maxm, minm, cutoff, npass, lam, cconv, report_costs=report_costs or ts.single)
            if k > 0:
                r = ts.bond_update_end()
                r["sweep"] = sched[k - 1][0]
                if with_heldout:
                    r["heldout"] = ts.heldout_report()
                reports.append(r)
        if sched:
            r = ts.bond_update_end()
            r["sweep"] = sched[-1][0]
            if with_heldout:
                r["heldout"] = ts.heldout_report()
            reports.append(r)
        return reports
    for sw in range(1, nsweep + 1):
        if log:
            log("\nSweep %d maxm=%d minm=%d" % (sw, maxm, minm))
        b, ha = 1, 1
        while ha <= 2:
            if max_bonds and len(reports) >= max_bonds:
                return reports
            r = ts.bond_update(b, ha, maxm, minm, cutoff, npass, lam, cconv, report_costs=report_costs or ts.single)
            r["sweep"] = sw
            if with_heldout:
                r["heldout"] = ts.heldout_report()
            reports.append(r)
            if log:
                log("Sweep %d Half %d Bond %d" % (sw, ha, r["c"]))
                log("In cgrad, lambda = %.3E" % lam)
                for p in range(r["cg"]["npass_done"]):
                    log("  Conj grad pass %d" % (p + 1))
                    if p < len(r["cg"]["cost"]):
                        log("  Cost = %.10f" % (r["cg"]["cost"][p] / NT))
                        log("  |r| = %.1E" % r["cg"]["rnorm"][p])
                log("SVD trunc err = %.2E" % r["truncerr"])
                log("Original m=%d, New m=%d" % (r["origm"], r["newm"]))
                log("|B-newB| = %.3E" % r["diff"])
                for l in range(NL):
                    log("  Label l=%d C%d = %.10f" % (l, l, r["label_cost"][l] / NT))
                log("  Reg. cost CR = %.10f" % (r["reg_cost"] / NT))
                log("Percent correct = %.4f%%, # incorrect = %d/%d" % (r["ncorrect"] * 100.0 / NT, NT - r["ncorrect"], NT))
                log("--> After SVD, Cost = %.10f" % (r["cost"] / NT))
            b, ha = _lib.sweepnext(b, ha, ts.N)
    return reports
