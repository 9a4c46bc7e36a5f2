"""ctypes binding of libseld_hip.so (the C ABI declared in include/seld_hip.h).

There is deliberately NO fallback: if the shared library is missing or a launch fails the
call raises.  The library is built in-tree by `__graft_entry__.build()` (hipcc, gfx950).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SELD_HIP_LIB: another build of the same library (tools/hcq_ablate.sh timing variants); there is still no fallback
LIB_PATH = os.environ.get("SELD_HIP_LIB") or os.path.join(_HERE, "csrc", "libseld_hip.so")

SELD_OK = 0
_ERRORS = {-1: "SELD_EINVAL", -2: "SELD_EWORKSPACE", -3: "SELD_ELAUNCH", -4: "SELD_EUNSUPPORTED"}

SELD_EPI_NONE, SELD_EPI_ACCUMULATE, SELD_EPI_ADD, SELD_EPI_STATS = 0, 1, 2, 4
SELD_ACT_NONE, SELD_ACT_RELU, SELD_ACT_TANH, SELD_ACT_SIGMOID = 0, 1, 2, 3
SELD_LIN_REAL, SELD_LIN_QUAT, SELD_LIN_DUALQ = 1, 4, 8
SELD_ROT_LAYOUT_CONV, SELD_ROT_LAYOUT_LINEAR = 0, 1
SELD_QUAT_LAYOUT_INPUT, SELD_QUAT_LAYOUT_CAT1 = 0, 1
SELD_DECODE_F32, SELD_DECODE_F64 = 0, 1


class SeldHipError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    _fields_ = [("algebra", ctypes.c_int32), ("ndim", ctypes.c_int32), ("N", ctypes.c_int32),
                ("Cin", ctypes.c_int32), ("Cout", ctypes.c_int32), ("in_", ctypes.c_int32 * 2),
                ("k", ctypes.c_int32 * 2), ("stride", ctypes.c_int32 * 2), ("pad", ctypes.c_int32 * 2),
                ("dil", ctypes.c_int32 * 2), ("groups", ctypes.c_int32)]


class Conv3dDesc(ctypes.Structure):
    """seld_conv3d_desc (include/seld_hip.h): per-axis arrays are (D, H, W)."""
    _fields_ = [("algebra", ctypes.c_int32), ("N", ctypes.c_int32), ("Cin", ctypes.c_int32), ("Cout", ctypes.c_int32),
                ("in_", ctypes.c_int32 * 3), ("k", ctypes.c_int32 * 3), ("stride", ctypes.c_int32 * 3),
                ("pad", ctypes.c_int32 * 3), ("dil", ctypes.c_int32 * 3), ("groups", ctypes.c_int32)]


class QuatShape(ctypes.Structure):
    """seld_quat_shape (include/seld_hip.h): the contiguous input as (dim0, mid, comp, inner), comp the component axis."""
    _fields_ = [("dim0", ctypes.c_int32), ("mid", ctypes.c_int32), ("comp", ctypes.c_int32), ("inner", ctypes.c_int32)]


class WgradJob(ctypes.Structure):
    """seld_wgrad_job (include/seld_hip.h): one convolution of a grouped weight-gradient call."""
    _fields_ = [("desc", ConvDesc), ("x", ctypes.c_void_p), ("dy", ctypes.c_void_p), ("dw", ctypes.c_void_p * 8)]


_lib = None


def lib():
    """Load (once) and return the ctypes handle.  Raises if the HIP library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SeldHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                "This package has no CPU/eager fallback by design.")
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.seld_build_arch.restype = ctypes.c_char_p
        # every query that returns a size_t: without its restype ctypes truncates the answer to a C int
        for name in ("seld_hc_conv_bwd_data_workspace", "seld_hc_conv_bwd_weight_workspace",
                     "seld_hc_conv_bwd_weight_det_workspace", "seld_hcq_pack_floats", "seld_hcq_pack_entry_bytes",
                     "seld_hcq_wgrad_row_workspace", "seld_hcq_wgrad_group_workspace",
                     "seld_hc_conv_transpose_bwd_weight_workspace", "seld_hc_conv3d_bwd_weight_workspace",
                     "seld_hc_conv3d_transpose_bwd_weight_workspace", "seld_dwconv_bwd_weight_workspace",
                     "seld_first_stage_gram_workspace", "seld_first_stage_bwd_workspace", "seld_hc_linear_bwd_workspace",
                     "seld_mha_bwd_workspace", "seld_mha_bwd_ex_workspace", "seld_stft_workspace",
                     "seld_quat_reduce_workspace", "seld_decode_workspace"):
            getattr(_lib, name).restype = ctypes.c_size_t
        _lib.seld_decode_workspace.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
        i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
        _lib.seld_decode_count.argtypes = [vp, i32, i64, i32, i32, i32, vp, ctypes.c_size_t, vp]
        _lib.seld_decode_write.argtypes = [vp, i32, i64, i32, i32, i32, ctypes.c_double, vp, ctypes.c_size_t, vp, vp, i64, vp, vp]
    return _lib


_reload_hooks = []


def reload_env():
    """Make the library re-read its SELD_* environment switches (it reads them once, at first use); host-side caches
    of kernel choices (hip_ops._core.memo) are dropped with it."""
    check(lib().seld_env_reload(), "seld_env_reload")
    for fn in _reload_hooks:
        fn()


def check(rc, what):
    if rc != SELD_OK:
        extra = ""
        if rc == -3:
            extra = f" (hipError {lib().seld_last_hip_error()})"
        raise SeldHipError(f"{what} failed: {_ERRORS.get(rc, rc)}{extra}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def ptr_array8(tensors):
    arr = (ctypes.c_void_p * 8)()
    for i in range(8):
        arr[i] = tensors[i].data_ptr() if i < len(tensors) and tensors[i] is not None else 0
    return arr


def current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
