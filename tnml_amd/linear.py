"""Host-side mirror of the reference's linear classifier (linear.cc) on top of the C-ABI (include/tnml.h, tnml_lin_*).

  LinearCG.start / run     cgrad, linear.cc:27-90 (K label columns over one shared data set, device-resident CG)
  LinearCG.evaluate        the evaluate lambda, linear.cc:169-187
Vectors are numpy arrays V[K, N+1] (bias first, then one weight per pixel).  Everything here calls the HIP path; nothing
falls back to the CPU and nothing imports the oracle.
"""
import ctypes as C

import numpy as np

from . import lib as _lib


class LinearError(RuntimeError):
    pass


class LinearCG:
    """Training (or test) set + K ridge-regression columns on one GPU.

    pixels:   uint8 [NT, N], decoded as (b/255.)/4 (linear.cc:133-139, mllib/mnist.h:495), or
    features: float64 [NT, N], the feature values x/4 themselves (reduced images, tests);
    labels:   int [NT]; cols: the label of each column (y = +1 if label == cols[k] else -1, linear.cc:132)."""

    def __init__(self, labels, cols, pixels=None, features=None, device=0):
        self._L = _lib.load()
        self._h = C.c_void_p()
        data = pixels if pixels is not None else features
        if data is None:
            raise ValueError("need pixels or features")
        self.N = int(np.asarray(data).shape[1])
        rc = self._L.tnml_lin_create(C.byref(self._h), int(device), self.N)
        if rc != 0:
            self._h = C.c_void_p()
            raise LinearError(self._L.tnml_lin_last_error(None).decode())
        self.set_data(labels, pixels=pixels, features=features)
        self.set_cols(cols)

    def _ck(self, rc):
        if rc != 0:
            raise LinearError(self._L.tnml_lin_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.tnml_lin_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, labels, pixels=None, features=None):
        """(re)load the data set, e.g. the test set before evaluate(); the CG has to be started again afterwards"""
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        self.NT = int(lab.shape[0])
        lp = lab.ctypes.data_as(C.POINTER(C.c_int32))
        if pixels is not None:
            px = np.ascontiguousarray(pixels, dtype=np.uint8)
            assert px.shape == (self.NT, self.N), px.shape
            self._ck(self._L.tnml_lin_set_data_u8(self._h, self.NT, px.ctypes.data_as(C.POINTER(C.c_uint8)), lp))
        elif features is not None:
            ft = np.ascontiguousarray(features, dtype=np.float64)
            assert ft.shape == (self.NT, self.N), ft.shape
            self._ck(self._L.tnml_lin_set_data_f64(self._h, self.NT, _lib.dptr(ft), lp))
        else:
            raise ValueError("need pixels or features")

    def set_cols(self, cols):
        c = np.ascontiguousarray(np.atleast_1d(cols), dtype=np.int32)
        self.K = int(c.shape[0])
        self.cols = c
        self._ck(self._L.tnml_lin_set_labels(self._h, self.K, c.ctypes.data_as(C.POINTER(C.c_int32))))

    def _vec(self, V):
        V = np.ascontiguousarray(V, dtype=np.float64).reshape(self.K, self.N + 1)
        return V

    def start(self, V, lam=0.0):
        """cgrad's preamble (linear.cc:37-48): W = V, r = p = residual gradient"""
        V = self._vec(V)
        self._ck(self._L.tnml_lin_cg_start(self._h, _lib.dptr(V), float(lam)))

    def run(self, npass):
        """npass more CG passes (linear.cc:51-89); returns the costs [npass, K]"""
        costs = np.zeros((int(npass), self.K))
        self._ck(self._L.tnml_lin_cg_run(self._h, int(npass), _lib.dptr(costs)))
        return costs

    @property
    def V(self):
        out = np.zeros((self.K, self.N + 1))
        self._ck(self._L.tnml_lin_get_v(self._h, _lib.dptr(out)))
        return out

    def evaluate(self, V):
        """linear.cc:169-187 on the loaded data: (ncorrect[K], Cnl[K]) with correct = f y > 0, Cnl = sum (f - y)^2 / NT"""
        V = self._vec(V)
        nc = np.zeros(self.K, dtype=np.int64)
        cnl = np.zeros(self.K)
        self._ck(self._L.tnml_lin_evaluate(self._h, _lib.dptr(V), nc.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dptr(cnl)))
        return nc, cnl
