"""ctypes binding of libtnml.so (include/tnml.h) -- the only way Python reaches the HIP path.

`import torch` happens first on purpose: the PyTorch wheel bundles its own ROCm runtime
(libamdhip64.so.7, librccl.so.1, librocblas.so.5, librocsolver.so.0 -- same SONAMEs as
/opt/rocm/lib), and a process must never hold two HIP runtimes.  Loading torch first makes
libtnml.so bind to the copies torch already mapped.  The library fails loudly when it is missing
or when no HIP device is usable: there is no CPU fallback on the product path.
"""
import ctypes as C
import os

import numpy as np
import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

NL = 10
MAX_PASS = 64
DTYPES = {"f32": 0, "f64_e32": 1, "f64": 2, "bf16": 3, "bf16x3": 4}    # TNML_F32 / TNML_F64_E32 / TNML_F64 / TNML_BF16 / TNML_BF16X3 (include/tnml.h)
GRADIENT_CHUNK_DEFAULT = 512             # TNML_GRADIENT_CHUNK_DEFAULT
LOSSES = {"quadratic": 0, "softmax": 1}    # TNML_LOSS_QUADRATIC / TNML_LOSS_SOFTMAX: option loss
PREDICT_DTYPES = {"f64": 0, "f32": 1}    # TNML_PREDICT_F64 / TNML_PREDICT_F32: option predict_dtype
GRADIENT_DTYPES = {"f64": 0, "f32": 1}   # TNML_GRADIENT_F64 / TNML_GRADIENT_F32: option gradient_dtype
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtnml.so")

EXPORTS = [
    "tnml_create", "tnml_destroy", "tnml_last_error", "tnml_comm_unique_id", "tnml_comm_init",
    "tnml_set_data_u8", "tnml_set_data_phi", "tnml_set_site", "tnml_site_dims", "tnml_get_site",
    "tnml_env_init", "tnml_set_bond", "tnml_shift_env", "tnml_env_dims", "tnml_get_env",
    "tnml_bond_dims", "tnml_bond_tensor", "tnml_forward", "tnml_gradient", "tnml_quadcost",
    "tnml_cgrad", "tnml_svd_split", "tnml_bond_update", "tnml_truncate", "tnml_sweepnext",
    "tnml_shard_bounds", "tnml_profile_enable", "tnml_profile_select", "tnml_profile_count", "tnml_profile_get",
    "tnml_profile_reset", "tnml_synchronize", "tnml_device_bytes", "tnml_svd_stats", "tnml_classify", "tnml_replica_check",
    "tnml_estimate_bytes", "tnml_device_memory", "tnml_plan_maxm", "tnml_set_option", "tnml_comm_init_local", "tnml_comm_init_oneshot", "tnml_collective_mode", "tnml_bond_update_begin", "tnml_bond_update_end", "tnml_replica_repairs", "tnml_pAp", "tnml_collective_stats", "tnml_last_warning",
    "tnml_exact", "tnml_set_option_real", "tnml_pinv", "tnml_env_stats", "tnml_oneshot_export", "tnml_oneshot_connect", "tnml_oneshot_mem_kind", "tnml_split_stats", "tnml_oneshot_region_bytes", "tnml_shift_skip_stats", "tnml_fwd_skip_stats",
    "tnml_spec_predict_stats", "tnml_truncate_device", "tnml_cg_state",
    "tnml_lin_create", "tnml_lin_destroy", "tnml_lin_last_error", "tnml_lin_set_data_u8", "tnml_lin_set_data_f64", "tnml_lin_set_labels",
    "tnml_lin_cg_start", "tnml_lin_cg_run", "tnml_lin_get_v", "tnml_lin_evaluate",
    "tnml_heldout_attach", "tnml_heldout_detach", "tnml_heldout_read",
    "tnml_mps_place", "tnml_mps_compress", "tnml_mps_overlap",
    "tnml_predict_u8", "tnml_predict_phi", "tnml_evaluate_u8", "tnml_evaluate_phi",
    "tnml_set_input_map", "tnml_get_input_map",
    "tnml_response_u8", "tnml_response_phi",
    "tnml_site_gradient_size", "tnml_site_gradient_u8", "tnml_site_gradient_phi",
    "tnml_site_step_u8", "tnml_site_step_phi", "tnml_site_step_reset", "tnml_site_step_state",
    "tnml_site_gradient_coef",
    "tnml_backward_u8", "tnml_backward_phi",
    "tnml_predict_dev", "tnml_evaluate_dev", "tnml_response_dev", "tnml_backward_dev", "tnml_site_step_dev",
    "tnml_set_site_dev", "tnml_get_site_dev", "tnml_abi_layout",
    "tnml_forward_taped_u8", "tnml_forward_taped_phi", "tnml_forward_taped_dev", "tnml_backward_taped", "tnml_backward_taped_dev",
    "tnml_tape_ticket", "tnml_set_sites_dev",
]


class Config(C.Structure):
    _fields_ = [("device", C.c_int), ("rank", C.c_int), ("nranks", C.c_int), ("N", C.c_int),
                ("NT_local", C.c_int), ("NT_total", C.c_int64), ("maxm", C.c_int), ("dtype", C.c_int),
                ("svd_backend", C.c_int), ("mode", C.c_int), ("target_label", C.c_int)]


class CgTrace(C.Structure):
    _fields_ = [("npass_done", C.c_int), ("converged", C.c_int), ("cost", C.c_double * MAX_PASS),
                ("rnorm", C.c_double * MAX_PASS), ("pAp", C.c_double * MAX_PASS), ("alpha", C.c_double * MAX_PASS)]


class SweepParams(C.Structure):
    _fields_ = [("maxm", C.c_int), ("minm", C.c_int), ("cutoff", C.c_double), ("npass", C.c_int),
                ("lambda_", C.c_double), ("lambda_cost", C.c_double), ("cconv", C.c_double), ("report_costs", C.c_int)]


class BondReport(C.Structure):
    _fields_ = [("bond", C.c_int), ("half", C.c_int), ("c", C.c_int), ("mL", C.c_int), ("mR", C.c_int),
                ("label_on_B", C.c_int), ("origm", C.c_int), ("newm", C.c_int),
                ("truncerr", C.c_double), ("norm_newB", C.c_double), ("diff_B_newB", C.c_double),
                ("cost_after_svd", C.c_double), ("label_cost", C.c_double * NL), ("reg_cost", C.c_double),
                ("ncorrect", C.c_int64), ("cg", CgTrace), ("cost_old", C.c_double), ("cost_cg", C.c_double),
                ("reg_cost_cg", C.c_double), ("norm_oB", C.c_double)]


class HeldoutReport(C.Structure):
    _fields_ = [("bond", C.c_int), ("half", C.c_int), ("count", C.c_int64), ("ncorrect", C.c_int64),
                ("cost", C.c_double), ("label_cost", C.c_double * NL)]


class EvalReport(C.Structure):
    _fields_ = [("n", C.c_int64), ("ncorrect", C.c_int64), ("cost", C.c_double), ("label_cost", C.c_double * NL),
                ("count", C.c_int64 * NL), ("nincorrect", C.c_int64 * NL), ("confusion", (C.c_int64 * NL) * NL)]


STEP_METHODS = {"sgd": 0, "adam": 1}    # TNML_STEP_SGD / TNML_STEP_ADAM


class StepParams(C.Structure):
    _fields_ = [("method", C.c_int), ("lr", C.c_double), ("momentum", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("clip", C.c_double), ("scale", C.c_double)]


class StepReport(C.Structure):
    _fields_ = [("t", C.c_int64), ("grad_norm", C.c_double), ("factor", C.c_double), ("clipped", C.c_int), ("eval", EvalReport)]


class CompressReport(C.Structure):
    _fields_ = [("maxm_before", C.c_int), ("maxm_after", C.c_int), ("nbonds", C.c_int), ("truncerr_sum", C.c_double),
                ("fallbacks", C.c_int64), ("newm", C.POINTER(C.c_int)), ("truncerr", C.POINTER(C.c_double))]


class InputMapStruct(C.Structure):
    _fields_ = [("src_rows", C.c_int), ("src_cols", C.c_int), ("block", C.c_int), ("row0", C.c_int), ("col0", C.c_int),
                ("out_rows", C.c_int), ("out_cols", C.c_int), ("ncodes", C.c_int), ("table", C.POINTER(C.c_double))]


class DevBatch(C.Structure):
    """tnml_dev_batch: the arrays of a device-resident call (device addresses; 0 / None: not given)"""
    _fields_ = [("n", C.c_int64), ("pixels", C.c_void_p), ("phi", C.c_void_p), ("phi32", C.c_void_p), ("labels", C.c_void_p),
                ("coef", C.c_void_p), ("which", C.c_void_p), ("stream", C.c_void_p)]


class DevOut(C.Structure):
    """tnml_dev_out: where a device-resident call leaves its results (device addresses)"""
    _fields_ = [("weights", C.c_void_p), ("pred", C.c_void_p), ("resp", C.c_void_p), ("grad", C.c_void_p), ("dphi", C.c_void_p),
                ("dphi32", C.c_void_p)]


_lib = None


def load():
    """Load libtnml.so; raises (never falls back) when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C tnml_amd/csrc` (the HIP extension is mandatory, there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    L.tnml_create.argtypes = [C.POINTER(vp), C.POINTER(Config)]
    L.tnml_destroy.argtypes = [vp]
    L.tnml_last_error.restype = C.c_char_p
    L.tnml_last_error.argtypes = [vp]
    L.tnml_comm_unique_id.argtypes = [vp]
    L.tnml_comm_init.argtypes = [vp, vp]
    L.tnml_set_data_u8.argtypes = [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]
    L.tnml_set_data_phi.argtypes = [vp, dp, C.POINTER(C.c_int32)]
    L.tnml_set_site.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    L.tnml_site_dims.argtypes = [vp, C.c_int, ip, ip, ip]
    L.tnml_get_site.argtypes = [vp, C.c_int, dp]
    L.tnml_env_init.argtypes = [vp]
    L.tnml_set_bond.argtypes = [vp, C.c_int]
    L.tnml_shift_env.argtypes = [vp, C.c_int, C.c_int]
    L.tnml_env_dims.argtypes = [vp, C.c_int, ip, ip]
    L.tnml_get_env.argtypes = [vp, C.c_int, dp]
    L.tnml_env_stats.argtypes = [vp] + [C.POINTER(C.c_int64)] * 4
    L.tnml_bond_dims.argtypes = [vp, C.c_int, ip, ip, ip]
    L.tnml_bond_tensor.argtypes = [vp, C.c_int, dp]
    L.tnml_forward.argtypes = [vp, dp, dp]
    L.tnml_gradient.argtypes = [vp, dp, dp]
    L.tnml_quadcost.argtypes = [vp, dp, C.c_double, dp, dp, dp, C.POINTER(C.c_int64)]
    L.tnml_cgrad.argtypes = [vp, dp, C.c_int, C.c_double, C.c_double, C.POINTER(CgTrace)]
    L.tnml_cg_state.argtypes = [vp, C.c_char_p, dp, C.c_int64]
    L.tnml_exact.argtypes = [vp, dp, C.c_double, C.c_double]
    L.tnml_pinv.argtypes = [vp, dp, C.c_int, C.c_int, C.c_double, C.c_double, dp, dp, C.POINTER(C.c_int), dp]
    L.tnml_set_option_real.argtypes = [vp, C.c_char_p, C.c_double]
    L.tnml_svd_split.argtypes = [vp, dp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, dp, ip, dp, ip]
    L.tnml_bond_update.argtypes = [vp, C.c_int, C.c_int, C.POINTER(SweepParams), C.POINTER(BondReport)]
    L.tnml_bond_update_begin.argtypes = [vp, C.c_int, C.c_int, C.POINTER(SweepParams)]
    L.tnml_bond_update_end.argtypes = [vp, C.POINTER(BondReport)]
    L.tnml_truncate.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.c_double, dp]
    L.tnml_sweepnext.argtypes = [ip, ip, C.c_int]
    L.tnml_sweepnext.restype = None
    L.tnml_shard_bounds.argtypes = [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.tnml_shard_bounds.restype = None
    L.tnml_profile_enable.argtypes = [vp, C.c_int]
    L.tnml_profile_select.argtypes = [vp, C.c_char_p]
    L.tnml_profile_count.argtypes = [vp]
    L.tnml_profile_get.argtypes = [vp, C.c_int, C.c_char_p, C.POINTER(C.c_int64), dp]
    L.tnml_profile_reset.argtypes = [vp]
    L.tnml_synchronize.argtypes = [vp]
    L.tnml_svd_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), dp, dp]
    L.tnml_device_bytes.argtypes = [vp]
    L.tnml_classify.argtypes = [vp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.tnml_device_bytes.restype = C.c_int64
    L.tnml_predict_u8.argtypes = [vp, C.c_int64, C.POINTER(C.c_uint8), dp, C.POINTER(C.c_int32)]
    L.tnml_predict_phi.argtypes = [vp, C.c_int64, dp, dp, C.POINTER(C.c_int32)]
    L.tnml_evaluate_u8.argtypes = [vp, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(EvalReport), dp, C.POINTER(C.c_int32)]
    L.tnml_evaluate_phi.argtypes = [vp, C.c_int64, dp, C.POINTER(C.c_int32), C.POINTER(EvalReport), dp, C.POINTER(C.c_int32)]
    L.tnml_response_u8.argtypes = [vp, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), dp, dp, C.POINTER(C.c_int32)]
    L.tnml_response_phi.argtypes = [vp, C.c_int64, dp, C.POINTER(C.c_int32), dp, dp, C.POINTER(C.c_int32)]
    L.tnml_site_gradient_size.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.tnml_site_gradient_u8.argtypes = [vp, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), dp, dp, dp, C.POINTER(C.c_int32)]
    L.tnml_site_gradient_phi.argtypes = [vp, C.c_int64, dp, C.POINTER(C.c_int32), dp, dp, dp, C.POINTER(C.c_int32)]
    L.tnml_site_step_u8.argtypes = [vp, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), dp, C.POINTER(StepParams), C.POINTER(StepReport)]
    L.tnml_site_step_phi.argtypes = [vp, C.c_int64, dp, C.POINTER(C.c_int32), dp, C.POINTER(StepParams), C.POINTER(StepReport)]
    L.tnml_site_step_reset.argtypes = [vp]
    L.tnml_site_step_state.argtypes = [vp, C.c_char_p, dp, C.c_int64]
    L.tnml_site_gradient_coef.argtypes = [vp, dp, C.c_int64]
    L.tnml_backward_u8.argtypes = [vp, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), dp, dp, dp, dp, C.POINTER(C.c_int32)]
    L.tnml_backward_phi.argtypes = [vp, C.c_int64, dp, C.POINTER(C.c_int32), dp, dp, dp, dp, C.POINTER(C.c_int32)]
    L.tnml_predict_dev.argtypes = [vp, C.POINTER(DevBatch), C.POINTER(DevOut)]
    L.tnml_evaluate_dev.argtypes = [vp, C.POINTER(DevBatch), C.POINTER(DevOut), C.POINTER(EvalReport)]
    L.tnml_response_dev.argtypes = [vp, C.POINTER(DevBatch), C.POINTER(DevOut)]
    L.tnml_backward_dev.argtypes = [vp, C.POINTER(DevBatch), C.POINTER(DevOut)]
    L.tnml_site_step_dev.argtypes = [vp, C.POINTER(DevBatch), C.POINTER(StepParams), C.POINTER(StepReport)]
    L.tnml_set_site_dev.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.tnml_get_site_dev.argtypes = [vp, C.c_int, vp, vp]
    i64p = C.POINTER(C.c_int64)
    L.tnml_forward_taped_u8.argtypes = [vp, C.c_int64, C.POINTER(C.c_uint8), dp, C.POINTER(C.c_int32), i64p]
    L.tnml_forward_taped_phi.argtypes = [vp, C.c_int64, dp, dp, C.POINTER(C.c_int32), i64p]
    L.tnml_forward_taped_dev.argtypes = [vp, C.POINTER(DevBatch), C.POINTER(DevOut), i64p]
    L.tnml_backward_taped.argtypes = [vp, C.c_int64, dp, dp, dp]
    L.tnml_backward_taped_dev.argtypes = [vp, C.c_int64, vp, C.POINTER(DevOut), vp]
    L.tnml_tape_ticket.argtypes = [vp, i64p, i64p]
    L.tnml_set_sites_dev.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), C.POINTER(vp), vp]
    L.tnml_abi_layout.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
    L.tnml_set_input_map.argtypes = [vp, C.POINTER(InputMapStruct)]
    L.tnml_get_input_map.argtypes = [vp, C.POINTER(InputMapStruct)]
    L.tnml_replica_check.argtypes = [vp, ip]
    L.tnml_replica_repairs.argtypes = [vp]
    L.tnml_replica_repairs.restype = C.c_int64
    L.tnml_collective_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.tnml_pAp.argtypes = [vp, dp, C.c_double, dp]
    L.tnml_last_warning.argtypes = [vp]
    L.tnml_last_warning.restype = C.c_char_p
    L.tnml_comm_init_local.argtypes = [C.POINTER(vp), C.c_int]
    L.tnml_comm_init_oneshot.argtypes = [C.POINTER(vp), C.c_int]
    L.tnml_collective_mode.argtypes = [vp]
    L.tnml_oneshot_export.argtypes = [vp, C.c_char_p]
    L.tnml_oneshot_connect.argtypes = [vp, C.c_char_p]
    L.tnml_oneshot_mem_kind.argtypes = [vp]
    L.tnml_split_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.tnml_spec_predict_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.tnml_truncate_device.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, ip, ip]
    L.tnml_shift_skip_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.tnml_fwd_skip_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.tnml_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.tnml_estimate_bytes.argtypes = [C.POINTER(Config)]
    L.tnml_estimate_bytes.restype = C.c_int64
    L.tnml_oneshot_region_bytes.argtypes = [C.POINTER(Config)]
    L.tnml_oneshot_region_bytes.restype = C.c_int64
    L.tnml_device_memory.argtypes = [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.tnml_plan_maxm.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int64]
    L.tnml_heldout_attach.argtypes = [vp, vp]
    L.tnml_heldout_detach.argtypes = [vp]
    L.tnml_heldout_read.argtypes = [vp, C.POINTER(HeldoutReport)]
    L.tnml_mps_place.argtypes = [vp] + [C.c_int] * 8 + [dp]
    L.tnml_mps_compress.argtypes = [vp, C.c_double, C.c_int, C.POINTER(CompressReport)]
    L.tnml_mps_overlap.argtypes = [vp, dp]
    L.tnml_lin_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    L.tnml_lin_destroy.argtypes = [vp]
    L.tnml_lin_last_error.restype = C.c_char_p
    L.tnml_lin_last_error.argtypes = [vp]
    L.tnml_lin_set_data_u8.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]
    L.tnml_lin_set_data_f64.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_int32)]
    L.tnml_lin_set_labels.argtypes = [vp, C.c_int, C.POINTER(C.c_int32)]
    L.tnml_lin_cg_start.argtypes = [vp, dp, C.c_double]
    L.tnml_lin_cg_run.argtypes = [vp, C.c_int, dp]
    L.tnml_lin_get_v.argtypes = [vp, dp]
    L.tnml_lin_evaluate.argtypes = [vp, dp, C.POINTER(C.c_int64), dp]
    _lib = L
    return L


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def flat(a):
    """fp64 copy flattened in ITensor (first-index-fastest) order"""
    return np.array(np.asarray(a, dtype=np.float64).ravel(order="F"), copy=True)


def truncate(p, maxm, minm, cutoff):
    p = np.ascontiguousarray(p, dtype=np.float64)
    te = C.c_double()
    m = load().tnml_truncate(dptr(p), len(p), maxm, minm, cutoff, C.byref(te))
    return m, te.value


def sweepnext(b, ha, N):
    bb, hh = C.c_int(b), C.c_int(ha)
    load().tnml_sweepnext(C.byref(bb), C.byref(hh), N)
    return bb.value, hh.value


def plan_maxm(N, NT_local, wanted, floor_m=1, dtype="f64", device=None, single=False, budget_bytes=None):
    """largest bond dimension <= wanted that an N-site MPS can reach and whose context fits the device (or budget_bytes)"""
    L = load()
    cfg = Config(device or 0, 0, 1, N, NT_local, NT_local, wanted, DTYPES[dtype], 0, 1 if single else 0, 0)
    if budget_bytes is None:
        budget_bytes = 0
        if device is not None:
            f, t = C.c_int64(), C.c_int64()
            if L.tnml_device_memory(device, C.byref(f), C.byref(t)) == 0:
                budget_bytes = int(f.value * 0.97)
    return L.tnml_plan_maxm(C.byref(cfg), wanted, floor_m, budget_bytes)


def estimate_bytes(N, NT_local, maxm, dtype="f64", single=False):
    cfg = Config(0, 0, 1, N, NT_local, NT_local, maxm, DTYPES[dtype], 0, 1 if single else 0, 0)
    return load().tnml_estimate_bytes(C.byref(cfg))


def shard_bounds(NT_total, nranks, rank):
    b, e = C.c_int64(), C.c_int64()
    load().tnml_shard_bounds(NT_total, nranks, rank, C.byref(b), C.byref(e))
    return b.value, e.value
