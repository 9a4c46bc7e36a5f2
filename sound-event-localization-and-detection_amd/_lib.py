"""ctypes binding of libseld_hip.so (the C ABI declared in include/seld_hip.h).

There is deliberately NO fallback: if the shared library is missing or a launch fails the
call raises.  The library is built in-tree by `__graft_entry__.build()` (hipcc, gfx950).

The header is the one place a signature is written down: `lib()` reads it and sets `restype` and `argtypes` on every
entry point, so callers pass plain Python numbers and ctypes gives each its declared width (`int64_t`, `size_t`,
`float` against `double`).  A prototype the parser cannot type, or the library does not export, is an error at load.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# SELD_HIP_LIB: another build of the same library (tools/hcq_ablate.sh timing variants); there is still no fallback
LIB_PATH = os.environ.get("SELD_HIP_LIB") or os.path.join(_HERE, "csrc", "libseld_hip.so")
HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "seld_hip.h")      # csrc/common.h includes it by the same path

SELD_OK = 0
_ERRORS = {-1: "SELD_EINVAL", -2: "SELD_EWORKSPACE", -3: "SELD_ELAUNCH", -4: "SELD_EUNSUPPORTED"}

SELD_EPI_NONE, SELD_EPI_ACCUMULATE, SELD_EPI_ADD, SELD_EPI_STATS = 0, 1, 2, 4
SELD_ACT_NONE, SELD_ACT_RELU, SELD_ACT_TANH, SELD_ACT_SIGMOID = 0, 1, 2, 3
SELD_LIN_REAL, SELD_LIN_QUAT, SELD_LIN_DUALQ = 1, 4, 8
SELD_ROT_LAYOUT_CONV, SELD_ROT_LAYOUT_LINEAR = 0, 1
SELD_QUAT_LAYOUT_INPUT, SELD_QUAT_LAYOUT_CAT1 = 0, 1
SELD_DECODE_F32, SELD_DECODE_F64 = 0, 1
(SELD_NORM_BN_BWD_FUSED, SELD_NORM_BN_BWD_REDUCE, SELD_NORM_BN_BWD_APPLY, SELD_NORM_GATE_FWD, SELD_NORM_GATE_BWD_FUSED,
 SELD_NORM_GATE_BWD_REDUCE, SELD_NORM_GATE_BWD_APPLY) = range(7)       # seld_norm_kernel_label(op, ...)
SELD_BN_ONE_PASS_MAX, SELD_GATE_ONE_PASS_MAX = 32768, 16384             # largest N*S of the one-pass backward kernels


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


_C_TYPES = {"int32_t": ctypes.c_int32, "int": ctypes.c_int32, "int64_t": ctypes.c_int64, "long long": ctypes.c_int64,
            "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
_C_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"^([^\n;{}()]*?)\b(seld_\w+)\s*\(([^()]*)\)\s*;", re.M)


def prototypes(header):
    """{name: (restype, argtypes)} of every `<ret> seld_name(<params>);` in the text of include/seld_hip.h.  Anything
    with `*` or `[` travels as a pointer; a by-value type outside the closed map above raises, naming the function."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _C_RETURNS:
            raise SeldHipError(f"seld_hip.h: {name} returns `{ret}`, which the binding does not know")
        argtypes = []
        for par in ([] if params.strip() in ("", "void") else params.split(",")):
            ctype = " ".join(par.replace("const ", " ").split()[:-1])      # the last word is the parameter's name
            if "*" in par or "[" in par:
                argtypes.append(ctypes.c_void_p)
            elif ctype in _C_TYPES:
                argtypes.append(_C_TYPES[ctype])
            else:
                raise SeldHipError(f"seld_hip.h: {name} has the parameter `{par.strip()}`, which the binding does not know")
        out[name] = (_C_RETURNS[ret], argtypes)
    unread = sorted(set(re.findall(r"\b(seld_\w+)\s*\(", text)) - set(out))
    if unread:      # e.g. a return type on a line of its own: never left untyped
        raise SeldHipError(f"seld_hip.h: the binding cannot read the prototype of {', '.join(unread)}")
    return out


_lib = None


def lib():
    """Load (once) and return the ctypes handle, every entry point declared with the restype and argtypes that
    include/seld_hip.h gives it.  Raises if the HIP library is not built or lacks a declared entry point."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SeldHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                "This package has no CPU/eager fallback by design.")
        handle = ctypes.CDLL(LIB_PATH)
        with open(HEADER_PATH) as f:
            declared = prototypes(f.read())
        for name, (restype, argtypes) in declared.items():
            fn = getattr(handle, name, None)
            if fn is None:
                raise SeldHipError(f"{LIB_PATH} does not export {name}, which {HEADER_PATH} declares")
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
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
