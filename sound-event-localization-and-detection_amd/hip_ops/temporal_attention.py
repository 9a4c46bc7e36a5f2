"""Temporal attention core (csrc/temporal_attention.hip): single-head flash attention on one projected tensor
qkv (N, 2K + V, T) = [q | k | v] with an index mask (none | causal | band) and optional per-sample valid lengths.
include/seld_hip.h has the definition; one launch forward, three backward, no atomics."""
import torch

from .. import _lib as L
from ._core import kernel_label, timed

__all__ = ["at_core", "at_kernel_label", "AtCoreFn", "AT_MASKS", "AT_MAX_WIDTH"]

AT_MASKS = {"none": 0, "causal": 1, "band": 2}      # SELD_AT_NONE / SELD_AT_CAUSAL / SELD_AT_BAND
AT_MAX_WIDTH = 64                                   # SELD_AT_MAX_WIDTH
_OPS = {"fwd": 0, "bwd_dq": 1, "bwd_dkv": 2}        # SELD_AT_*


def at_kernel_label(op, T, key_size, value_size):
    """The kernel form a call on (N, 2K + V, T) launches (tensors on a 16-byte boundary); op: fwd | bwd_dq | bwd_dkv."""
    return kernel_label(L.lib().seld_at_kernel_label, _OPS[op], int(T), int(key_size), int(value_size))


def _check(qkv, K, V, mask, band, lengths):
    """Host-side validation (nothing here touches the device); returns (N, T, mask kind)."""
    what = "at_core"
    if not torch.is_tensor(qkv) or not qkv.is_cuda:
        raise L.SeldHipError(f"{what}: qkv: expected a HIP device tensor (this package has no CPU path)")
    if qkv.dtype != torch.float32:
        raise L.SeldHipError(f"{what}: qkv: expected float32, got {qkv.dtype}")
    if not qkv.is_contiguous():
        raise L.SeldHipError(f"{what}: qkv: expected a contiguous tensor")
    for name, w in (("key_size", K), ("value_size", V)):
        if isinstance(w, bool) or not isinstance(w, int) or w < 1:
            raise L.SeldHipError(f"{what}: {name} must be a positive integer, got {w!r}")
        if w > AT_MAX_WIDTH:
            raise L.SeldHipError(f"{what}: {name} {w} > {AT_MAX_WIDTH} is not supported")
    if qkv.dim() != 3 or qkv.numel() == 0 or qkv.shape[1] != 2 * K + V:
        raise L.SeldHipError(f"{what}: qkv must be (N, 2 * {K} + {V}, T) with every extent positive, got {tuple(qkv.shape)}")
    if mask not in AT_MASKS:
        raise L.SeldHipError(f"{what}: mask must be one of {', '.join(AT_MASKS)}, got {mask!r}")
    if isinstance(band, bool) or not isinstance(band, int) or band < 0:
        raise L.SeldHipError(f"{what}: band must be a non-negative integer, got {band!r}")
    N, _, T = qkv.shape
    if N >= 2 ** 31 or T >= 2 ** 31 or band >= 2 ** 31:
        raise L.SeldHipError(f"{what}: N = {N}, T = {T}, band = {band} are more than the entry points' 32-bit extents")
    if lengths is not None:
        if not torch.is_tensor(lengths) or lengths.device != qkv.device:
            raise L.SeldHipError(f"{what}: lengths: expected a tensor on {qkv.device}")
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (N,) or not lengths.is_contiguous():
            raise L.SeldHipError(f"{what}: lengths must be a contiguous int32 tensor of {N} entries, got {lengths.dtype} "
                                 f"{tuple(lengths.shape)}")
    return N, T, AT_MASKS[mask]


def _work(N, T, K, V, products):
    """(flops, bytes) of a dense call: `products` T x T products of width K or V each way, the tensors once."""
    return lambda: (2.0 * N * T * T * (K + V) * products / 2, 4.0 * N * T * (2 * (2 * K + V) + 2 * V + 2))


class AtCoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, K, V, mask, band, lengths):
        N, T, kind = _check(qkv, K, V, mask, band, lengths)
        read = torch.empty((N, V, T), device=qkv.device, dtype=torch.float32)
        lse = torch.empty((N, T), device=qkv.device, dtype=torch.float32)
        with torch.cuda.device(qkv.device):
            with timed(lambda: at_kernel_label("fwd", T, K, V), _work(N, T, K, V, 2)):
                L.check(L.lib().seld_at_fwd(L.ptr(qkv), N, T, K, V, kind, band, L.ptr(lengths), L.ptr(read), L.ptr(lse),
                                            L.current_stream()), "seld_at_fwd")
        ctx.geom = (N, T, K, V, kind, band)
        ctx.save_for_backward(qkv, read, lse, lengths)
        ctx.mark_non_differentiable(lse)
        return read, lse

    @staticmethod
    def backward(ctx, dread, _dlse):
        qkv, read, lse, lengths = ctx.saved_tensors
        N, T, K, V, kind, band = ctx.geom
        if dread.dtype != torch.float32 or not dread.is_cuda:
            raise L.SeldHipError("at_core: dread: expected a float32 HIP device tensor")
        dread = dread.contiguous()
        dqkv = torch.empty_like(qkv)
        lib = L.lib()
        nbytes = lib.seld_at_bwd_workspace(N, T)
        wsb = torch.empty((nbytes + 3) // 4, device=qkv.device, dtype=torch.float32)
        with torch.cuda.device(qkv.device):
            with timed(lambda: at_kernel_label("bwd_dkv", T, K, V), _work(N, T, K, V, 7)):
                L.check(lib.seld_at_bwd(L.ptr(qkv), L.ptr(read), L.ptr(dread), L.ptr(lse), N, T, K, V, kind, band,
                                        L.ptr(lengths), L.ptr(dqkv), L.ptr(wsb), nbytes, L.current_stream()), "seld_at_bwd")
        return dqkv, None, None, None, None, None


def at_core(qkv, key_size, value_size, mask="causal", band=0, lengths=None, return_lse=False):
    """read (N, V, T) = softmax(q^T k / sqrt(K), over the allowed keys) v for qkv (N, 2K + V, T) = [q | k | v]; mask: none |
    causal (s <= t) | band (|t - s| <= band); lengths: optional int32 device tensor of N valid lengths (keys at or behind
    a sample's length are excluded).  Excluded keys weigh exactly 0; a row with no allowed key reads 0.  Differentiable in
    qkv.  return_lse: also the (N, T) log-sum-exp (no gradient).  Everything is validated on the host first."""
    read, lse = AtCoreFn.apply(qkv, key_size, value_size, mask, band, lengths)
    return (read, lse) if return_lse else read
