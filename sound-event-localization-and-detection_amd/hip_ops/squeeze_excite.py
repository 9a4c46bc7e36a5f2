"""Squeeze-and-excitation (csrc/squeeze_excite.hip): y = x * sigmoid(W2 relu(W1 mean(x) + b1) + b2), one gate per
hypercomplex channel and sample.  include/seld_hip.h has the definition; seven launches forward + backward, no atomics."""
import torch

from .. import _lib as L
from ._core import _req, kernel_label, timed
from .norm_act import _claim_grad_slots, _ncs

__all__ = ["squeeze_excite", "se_gates", "se_kernel_label", "SqueezeExciteFn", "SE_MAX_GATED", "SE_MAX_HIDDEN",
           "SE_BLOCK_MIN_S", "SE_COMPONENTS"]

SE_MAX_GATED = 4096         # SELD_SE_MAX_GATED: gated channels C / components
SE_MAX_HIDDEN = 1024        # SELD_SE_MAX_HIDDEN
SE_BLOCK_MIN_S = 1024       # SELD_SE_BLOCK_MIN_S: the kernels that sum give a row to a workgroup from this length on, below to a wave
SE_COMPONENTS = (1, 4, 8)
_OPS = {"squeeze": 0, "scale": 1, "bwd_reduce": 2, "bwd_apply": 3}       # SELD_SE_*


def _same_phase(*ts):
    """Every tensor at the same offset from a 16-byte boundary: the streaming kernels then use 16-byte accesses."""
    return int(len({t.data_ptr() & 15 for t in ts}) == 1)


def se_kernel_label(op, S, same_phase=1):
    """The kernel form a streaming call of rows of S floats launches; op: squeeze | scale | bwd_reduce | bwd_apply."""
    return kernel_label(L.lib().seld_se_kernel_label, _OPS[op], int(S), int(same_phase))


def _check(what, x, w1, b1, w2, b2, components):
    """Host-side validation (nothing here touches the device); returns (N, C, S, Cg, Hd)."""
    for t, name in ((x, "x"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.SeldHipError(f"{what}: {name}: expected a HIP device tensor (this package has no CPU path)")
        if t.dtype != torch.float32:
            raise L.SeldHipError(f"{what}: {name}: expected float32, got {t.dtype}")
        if not t.is_contiguous():
            raise L.SeldHipError(f"{what}: {name}: expected a contiguous tensor")
        if t.device != x.device:
            raise L.SeldHipError(f"{what}: {name} is on {t.device}, x on {x.device}")
    if components not in SE_COMPONENTS:
        raise L.SeldHipError(f"{what}: components must be one of {SE_COMPONENTS}, got {components!r}")
    if x.dim() < 3 or x.numel() == 0:
        raise L.SeldHipError(f"{what}: x must be (N, C, *spatial) with every extent positive, got {tuple(x.shape)}")
    N, C, S = _ncs(x)
    if C % components:
        raise L.SeldHipError(f"{what}: {C} channels are not a multiple of {components} components")
    Cg = C // components
    if w1.dim() != 2 or w1.shape[1] != Cg or w1.shape[0] < 1:
        raise L.SeldHipError(f"{what}: w1 must be (hidden, {Cg}), got {tuple(w1.shape)}")
    Hd = int(w1.shape[0])
    if tuple(b1.shape) != (Hd,) or tuple(w2.shape) != (Cg, Hd) or tuple(b2.shape) != (Cg,):
        raise L.SeldHipError(f"{what}: expected b1 ({Hd},), w2 ({Cg}, {Hd}), b2 ({Cg},), got {tuple(b1.shape)}, "
                             f"{tuple(w2.shape)}, {tuple(b2.shape)}")
    if Cg > SE_MAX_GATED or Hd > SE_MAX_HIDDEN:
        raise L.SeldHipError(f"{what}: {Cg} gated channels / {Hd} hidden units; the kernels hold at most {SE_MAX_GATED} / "
                             f"{SE_MAX_HIDDEN} in LDS")
    if S >= 2 ** 31 or N * C >= 2 ** 31:
        raise L.SeldHipError(f"{what}: {N} x {C} rows of {S} elements are more than the entry points' 32-bit extents")
    return N, C, S, Cg, Hd


def _excite(x, w1, b1, w2, b2, A, N, C, S, Cg, Hd):
    """squeeze + excite: (z (N, Cg), h (N, Hd), s (N, Cg))."""
    lib, st, dev = L.lib(), L.current_stream(), x.device
    rowsum = torch.empty(N * C, device=dev, dtype=torch.float32)
    z, s = (torch.empty((N, Cg), device=dev, dtype=torch.float32) for _ in range(2))
    h = torch.empty((N, Hd), device=dev, dtype=torch.float32)
    with timed(lambda: se_kernel_label("squeeze", S), lambda: (float(N * C * S), 4.0 * (N * C * S + N * C))):
        L.check(lib.seld_se_squeeze(L.ptr(x), N * C, S, L.ptr(rowsum), st), "seld_se_squeeze")
    with timed("se_excite_fwd_kernel", lambda: (4.0 * N * Cg * Hd, 4.0 * (N * C + 2 * Cg * Hd + 2 * N * Cg + N * Hd))):
        L.check(lib.seld_se_excite_fwd(L.ptr(rowsum), N, C, S, A, Hd, L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2),
                                       L.ptr(z), L.ptr(h), L.ptr(s), st), "seld_se_excite_fwd")
    return z, h, s


class SqueezeExciteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, A):
        N, C, S, Cg, Hd = _check("squeeze_excite", x, w1, b1, w2, b2, A)
        with torch.cuda.device(x.device):
            z, h, s = _excite(x, w1, b1, w2, b2, A, N, C, S, Cg, Hd)
            y = torch.empty_like(x)
            with timed(lambda: se_kernel_label("scale", S, _same_phase(x, y)), lambda: (float(N * C * S), 8.0 * N * C * S)):
                L.check(L.lib().seld_se_scale(L.ptr(x), N, C, S, A, L.ptr(s), L.ptr(y), L.current_stream()), "seld_se_scale")
        ctx.dims = (N, C, S, Cg, Hd, A)
        ctx.params = (w1, b1, w2, b2)
        ctx.save_for_backward(x, z, h, s)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, z, h, s = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        N, C, S, Cg, Hd, A = ctx.dims
        dy = _req(dy, "dy")
        lib, st, dev = L.lib(), L.current_stream(), x.device
        slot, _ = _claim_grad_slots((w1, b1, w2, b2), adjacent=False)
        if slot is not None:        # the optimiser's flat gradient buffer: the sums are added to the slots in place
            grads = [p.grad for p in (w1, b1, w2, b2)]
        else:
            grads = [torch.empty_like(p) for p in (w1, b1, w2, b2)]
        q = torch.empty(N * C, device=dev, dtype=torch.float32)
        dp2, dz = (torch.empty((N, Cg), device=dev, dtype=torch.float32) for _ in range(2))
        dh = torch.empty((N, Hd), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            with timed(lambda: se_kernel_label("bwd_reduce", S, _same_phase(dy, x)),
                       lambda: (2.0 * N * C * S, 4.0 * (2 * N * C * S + N * C))):
                L.check(lib.seld_se_bwd_reduce(L.ptr(dy), L.ptr(x), N * C, S, L.ptr(q), st), "seld_se_bwd_reduce")
            with timed("se_excite_bwd_kernel", lambda: (8.0 * N * Cg * Hd, 4.0 * (N * C + 4 * Cg * Hd + 5 * N * Cg + 3 * N * Hd))):
                L.check(lib.seld_se_excite_bwd(L.ptr(q), N, C, A, Hd, L.ptr(w1), L.ptr(w2), L.ptr(z), L.ptr(h), L.ptr(s),
                                               L.ptr(dp2), L.ptr(dh), L.ptr(dz), *(L.ptr(g) for g in grads),
                                               int(slot is not None), st), "seld_se_excite_bwd")
            dx = None
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                with timed(lambda: se_kernel_label("bwd_apply", S, _same_phase(dy, dx)),
                           lambda: (2.0 * N * C * S, 8.0 * N * C * S)):
                    L.check(lib.seld_se_bwd_apply(L.ptr(dy), N, C, S, A, L.ptr(s), L.ptr(dz), L.ptr(dx), st),
                            "seld_se_bwd_apply")
        if slot is not None:
            return dx, None, None, None, None, None
        return (dx, *grads, None)


def squeeze_excite(x, w1, b1, w2, b2, components=1):
    """y[n, c] = x[n, c] * s[n, c mod Cg] for x (N, C, *spatial), Cg = C / components; w1 (Hd, Cg), b1 (Hd), w2 (Cg, Hd),
    b2 (Cg).  Differentiable in x and the four parameters; parameters an optimiser owns (`FlatAdam`) get their gradient
    added straight into their slots.  Everything is validated on the host first."""
    return SqueezeExciteFn.apply(x, w1, b1, w2, b2, components)


def se_gates(x, w1, b1, w2, b2, components=1):
    """The gates s (N, Cg) alone (no gradient)."""
    N, C, S, Cg, Hd = _check("se_gates", x, w1, b1, w2, b2, components)
    with torch.no_grad(), torch.cuda.device(x.device):
        return _excite(x.detach(), w1.detach(), b1.detach(), w2.detach(), b2.detach(), components, N, C, S, Cg, Hd)[2]
