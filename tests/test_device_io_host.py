"""CPU tests of the device-resident interface (include/tnml.h, "device-resident arguments"): the symbols are there, the ctypes structs
have the header's layout, and the Python wrappers decide between the two paths -- and refuse a mix -- before any C call.  No GPU: the
wrappers run on a TrainStates that was never created, with a recorder in the library's place, and "device tensors" are CPU tensors of
a subclass that says it lives on a CUDA device."""
import ctypes as C

import numpy as np
import pytest
import torch

NEW = ["tnml_predict_dev", "tnml_evaluate_dev", "tnml_response_dev", "tnml_backward_dev", "tnml_site_step_dev", "tnml_set_site_dev",
       "tnml_get_site_dev", "tnml_abi_layout"]


def test_new_symbols_are_exported():
    from tnml_amd import lib
    L = lib.load()
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(lib.EXPORTS)


@pytest.mark.parametrize("name,struct", [("tnml_dev_batch", "DevBatch"), ("tnml_dev_out", "DevOut")])
def test_ctypes_structs_match_the_header(name, struct):
    from tnml_amd import lib
    S = getattr(lib, struct)
    out = (C.c_int64 * 16)()
    k = lib.load().tnml_abi_layout(name.encode(), out)
    assert k == 1 + len(S._fields_)
    assert out[0] == C.sizeof(S)
    assert list(out[1:k]) == [getattr(S, f).offset for f, _ in S._fields_]
    assert lib.load().tnml_abi_layout(b"tnml_nothing", out) == -1


def test_field_names_are_the_headers():
    import os
    import re
    from tnml_amd import lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tnml.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = hdr[hdr.index("int64_t        n;"):hdr.index("} tnml_dev_batch;")]
    assert re.findall(r"(\w+);", body) == [f for f, _ in lib.DevBatch._fields_]
    out = re.search(r"typedef struct \{([^}]*)\} tnml_dev_out;", hdr).group(1)
    assert re.findall(r"(\w+);", out) == [f for f, _ in lib.DevOut._fields_]


class _OnDevice(torch.Tensor):
    """a CPU tensor that reports a CUDA device: enough for the dispatch, which must decide before it touches any data"""
    index = 0

    @property
    def is_cuda(self):
        return True

    @property
    def device(self):
        return torch.device("cuda", self.index)


class _OnDevice1(_OnDevice):
    index = 1


class _Recorder:
    """stands where the ctypes library stands: records the entry points called, every call succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _uncreated(N=6):
    from tnml_amd.fixedl import TrainStates
    ts = TrainStates.__new__(TrainStates)
    ts._L, ts._h = _Recorder(), C.c_void_p()
    ts.N, ts.nl, ts.device, ts._bytes_per_image, ts.single = N, 10, 0, N, False
    return ts


def _fake(a, cls=_OnDevice):
    return torch.from_numpy(np.ascontiguousarray(a)).as_subclass(cls)


def test_wrappers_reject_a_mix_and_a_wrong_device_before_calling_c():
    ts = _uncreated()
    phi, labels, coef = np.zeros((3, 6, 2)), np.zeros(3, dtype=np.int32), np.zeros((3, 10))
    with pytest.raises(ValueError, match="all be device tensors, or none"):
        ts.evaluate(labels, phi=_fake(phi))
    with pytest.raises(ValueError, match="all be device tensors, or none"):
        ts.backward(coef=_fake(coef), phi=torch.from_numpy(phi))
    with pytest.raises(ValueError, match="all be device tensors, or none"):
        ts.gradient_step(labels=_fake(labels), pixels=np.zeros((3, 6), dtype=np.uint8), lr=1e-3)
    with pytest.raises(ValueError, match="all be device tensors, or none"):
        ts.site_response(phi=phi, which=_fake(labels))
    with pytest.raises(ValueError, match="device 1, the context is on device 0"):
        ts.predict(phi=_fake(phi, _OnDevice1))
    with pytest.raises(ValueError, match="device 1, the context is on device 0"):
        ts.site_gradient(labels=_fake(labels), phi=_fake(phi, _OnDevice1))
    with pytest.raises(ValueError, match="device 1, the context is on device 0"):
        ts.set_site(1, _fake(np.zeros((1, 2, 2)), _OnDevice1))
    assert ts._L.calls == []
    ts._h = None                                                                       # (nothing to destroy)


def test_numpy_arrays_and_cpu_tensors_take_the_host_path():
    ts = _uncreated()
    phi, labels = np.zeros((3, 6, 2)), np.zeros(3, dtype=np.int32)
    assert ts._on_device(phi, labels) is False and ts._on_device(torch.from_numpy(phi), None, torch.from_numpy(labels)) is False
    assert ts._on_device(_fake(phi), _fake(labels)) is True
    w, pred = ts.predict(phi=phi)
    assert isinstance(w, np.ndarray) and w.shape == (3, 10) and pred.dtype == np.int32
    w, pred = ts.predict(phi=torch.from_numpy(phi))
    assert isinstance(w, np.ndarray)
    ts.evaluate(torch.from_numpy(labels), pixels=torch.zeros((3, 6), dtype=torch.uint8))
    ts.site_response(phi=phi, which=labels)
    assert ts._L.calls == ["tnml_predict_phi", "tnml_predict_phi", "tnml_evaluate_u8", "tnml_response_phi"]
    ts._h = None
