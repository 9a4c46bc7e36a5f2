"""Around the network in a training step: loss, Adam, the step state, STFT, dataset normalisation, metrics, decoding."""

import torch

from .. import _lib as L
from ._core import _req, scratch, timed


# ======================================================================================
# loss, Adam, STFT
# ======================================================================================
class SeldLossFn(torch.autograd.Function):
    """BCELoss(sed, t_sed) * w_sed + MSELoss(doa, t_doa) * w_doa  (train.py:186-204)."""

    @staticmethod
    def forward(ctx, sed, doa, target, w_sed, w_doa):
        sed2 = _req(sed.reshape(-1, sed.shape[-1]), "sed")
        doa2 = _req(doa.reshape(-1, doa.shape[-1]), "doa")
        tgt = _req(target.reshape(-1, target.shape[-1]), "target")
        rows, n_sed = sed2.shape
        n_doa = doa2.shape[1]
        loss = torch.empty(1, device=sed.device, dtype=torch.float32)       # written, not accumulated (ticketed reduction)
        dsed, ddoa = torch.empty_like(sed2), torch.empty_like(doa2)
        L.check(L.lib().seld_loss_fwd_bwd(L.ptr(sed2), L.ptr(doa2), L.ptr(tgt), rows, n_sed, n_doa, w_sed, w_doa,
                                          L.ptr(loss), L.ptr(dsed), L.ptr(ddoa),
                                          L.current_stream()), "seld_loss_fwd_bwd")
        ctx.shapes = (tuple(sed.shape), tuple(doa.shape))
        ctx.save_for_backward(dsed, ddoa)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dsed, ddoa = ctx.saved_tensors
        s1, s2 = ctx.shapes
        if g.data_ptr() == unit_gradient(g.device).data_ptr():       # backward_from_loss(): d loss / d loss = 1
            return dsed.reshape(s1), ddoa.reshape(s2), None, None, None
        return (dsed * g).reshape(s1), (ddoa * g).reshape(s2), None, None, None


_unit_gradients = {}


def unit_gradient(device):
    """The constant 1.0 the training step seeds the backward pass with: one cached tensor per device, so neither the
    autograd engine (ones_like -> fill) nor SeldLossFn.backward (gradient * 1.0) launches a kernel for it."""
    device = torch.device(device)
    t = _unit_gradients.get(device)
    if t is None:
        t = _unit_gradients[device] = torch.ones((), device=device, dtype=torch.float32)
    return t


def backward_from_loss(loss):
    """The backward pass from `loss`, seeded with the cached unit gradient."""
    loss.backward(unit_gradient(loss.device))


def seld_loss(sed, doa, target, w_sed=1.0, w_doa=5.0):
    return SeldLossFn.apply(sed, doa, target, float(w_sed), float(w_doa))


def _pit_call(sed, doa, target, overlaps, w_sed, w_doa, grads, perm, parts):
    """One seld_loss_pit_fwd_bwd launch on (.., n_sed) / (.., n_doa) / (.., n_sed + n_doa) tensors.  Returns
    (loss (1,), dsed, ddoa, perm, parts), each of the last four None unless asked for."""
    sed2 = _req(sed.reshape(-1, sed.shape[-1]), "sed")
    doa2 = _req(doa.reshape(-1, doa.shape[-1]), "doa")
    tgt = _req(target.reshape(-1, target.shape[-1]), "target")
    rows, n_sed = sed2.shape
    overlaps = int(overlaps)
    if overlaps < 1 or n_sed % overlaps:
        raise L.SeldHipError(f"seld_loss_pit: {n_sed} SED outputs are not a multiple of overlaps = {overlaps}")
    if tuple(doa2.shape) != (rows, 3 * n_sed) or tuple(tgt.shape) != (rows, 4 * n_sed):
        raise L.SeldHipError(f"seld_loss_pit: shapes {tuple(sed2.shape)} / {tuple(doa2.shape)} / {tuple(tgt.shape)} do not match "
                             f"(rows, {n_sed}) / (rows, {3 * n_sed}) / (rows, {4 * n_sed})")
    classes = n_sed // overlaps
    dev = sed2.device
    loss = torch.empty(1, device=dev, dtype=torch.float32)              # written, not accumulated (ticketed reduction)
    dsed, ddoa = (torch.empty_like(sed2), torch.empty_like(doa2)) if grads else (None, None)
    perm_t = torch.empty((rows, classes), device=dev, dtype=torch.int32) if perm else None
    parts_t = torch.empty(2, device=dev, dtype=torch.float32) if parts else None
    L.check(L.lib().seld_loss_pit_fwd_bwd(L.ptr(sed2), L.ptr(doa2), L.ptr(tgt), rows, classes, overlaps, w_sed, w_doa,
                                          L.ptr(loss), L.ptr(dsed), L.ptr(ddoa), L.ptr(perm_t), L.ptr(parts_t),
                                          L.current_stream()), "seld_loss_pit_fwd_bwd")
    return loss, dsed, ddoa, perm_t, parts_t


class SeldLossPitFn(torch.autograd.Function):
    """SeldLossFn with, per (frame, class) cell, the pairing of the `overlaps` prediction slots with the target slots
    that costs least (include/seld_hip.h: seld_loss_pit_fwd_bwd); the choice is a constant of the backward pass.
    Returns (loss, perm): perm is the (rows, classes) int32 index of the chosen permutation, or None."""

    @staticmethod
    def forward(ctx, sed, doa, target, overlaps, w_sed, w_doa, return_perm):
        loss, dsed, ddoa, perm, _ = _pit_call(sed, doa, target, overlaps, w_sed, w_doa, True, return_perm, False)
        ctx.shapes = (tuple(sed.shape), tuple(doa.shape))
        ctx.save_for_backward(dsed, ddoa)
        if perm is not None:
            ctx.mark_non_differentiable(perm)
        return loss.reshape(()), perm

    @staticmethod
    def backward(ctx, g, _gperm=None):
        dsed, ddoa = ctx.saved_tensors
        s1, s2 = ctx.shapes
        if g.data_ptr() == unit_gradient(g.device).data_ptr():       # backward_from_loss(): d loss / d loss = 1
            return dsed.reshape(s1), ddoa.reshape(s2), None, None, None, None, None
        return (dsed * g).reshape(s1), (ddoa * g).reshape(s2), None, None, None, None, None


def seld_loss_pit(sed, doa, target, overlaps, w_sed=1.0, w_doa=5.0, return_perm=False):
    """The permutation-invariant SELD loss over the `overlaps` (1..3) same-class track slots: one launch, forward and
    backward.  return_perm: (loss, perm) with perm (rows, classes) int32, the chosen permutation's lexicographic index."""
    loss, perm = SeldLossPitFn.apply(sed, doa, target, int(overlaps), float(w_sed), float(w_doa), bool(return_perm))
    return (loss, perm) if return_perm else loss


def seld_loss_pit_parts(sed, doa, target, overlaps, w_sed=1.0, w_doa=5.0):
    """(loss, parts, perm) without autograd and without gradients, for logging and analysis: parts = the w_sed * BCE and
    w_doa * MSE shares of the chosen pairing (2 floats on the device), perm as in seld_loss_pit."""
    with torch.no_grad():
        loss, _, _, perm, parts = _pit_call(sed.detach(), doa.detach(), target, overlaps, float(w_sed), float(w_doa), False,
                                            True, True)
    return loss.reshape(()), parts, perm


def adam_flat_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                   weight_decay=0.0, grad_scale=1.0):
    L.check(L.lib().seld_adam_flat(L.ptr(param), L.ptr(grad), L.ptr(exp_avg), L.ptr(exp_avg_sq), param.numel(), lr,
                                   beta1, beta2, eps, weight_decay, int(step), grad_scale,
                                   L.current_stream()), "seld_adam_flat")


def step_begin(flat_grad, state=None):
    """Zero the flat gradient buffer and (state given) advance the device-resident step state (seld_step_begin)."""
    L.check(L.lib().seld_step_begin(L.ptr(flat_grad), flat_grad.numel(), L.ptr(state), L.current_stream()),
            "seld_step_begin")


def adam_flat_step_state(param, grad, exp_avg, exp_avg_sq, state, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                         grad_scale=1.0):
    """seld_adam_flat with the step number and learning rate taken from the device-resident step state."""
    L.check(L.lib().seld_adam_flat_state(L.ptr(param), L.ptr(grad), L.ptr(exp_avg), L.ptr(exp_avg_sq), param.numel(),
                                         beta1, beta2, eps, weight_decay, grad_scale, L.ptr(state),
                                         L.current_stream()), "seld_adam_flat_state")


def _flat(t, name, what, n=None):
    """A flat fp32 device buffer of the optimiser (of n elements when given), or a SeldHipError naming it."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise L.SeldHipError(f"{what}: {name} must be a contiguous float32 HIP device tensor (this package has no CPU path)")
    if n is not None and t.numel() != n:
        raise L.SeldHipError(f"{what}: {name} holds {t.numel()} elements, expected {n}")
    return t


def grad_norm(grad, grad_scale, max_norm, clip):
    """One launch, nothing read back (seld_grad_norm): clip (4 floats on the device) receives ||grad * grad_scale||_2,
    torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)), the running largest norm and the
    running count of clipped steps.  Returns clip."""
    _flat(grad, "grad", "grad_norm")
    _flat(clip, "clip", "grad_norm", 4)
    if not float(max_norm) > 0.0:
        raise L.SeldHipError(f"grad_norm: max_norm must be greater than 0, got {max_norm!r}")
    L.check(L.lib().seld_grad_norm(L.ptr(grad), grad.numel(), grad_scale, max_norm, L.ptr(clip), L.current_stream()),
            "seld_grad_norm")
    return clip


def _adam_ex_buffers(what, param, grad, exp_avg, exp_avg_sq, ema, clip, ema_decay):
    n = _flat(param, "param", what).numel()
    for t, name in ((grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _flat(t, name, what, n)
    if ema is not None:
        _flat(ema, "ema", what, n)
        if not 0.0 <= float(ema_decay) < 1.0:
            raise L.SeldHipError(f"{what}: ema_decay must lie in [0, 1), got {ema_decay!r}")
    if clip is not None:
        _flat(clip, "clip", what, 4)
    return n


def adam_flat_step_ex(param, grad, exp_avg, exp_avg_sq, step, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                      grad_scale=1.0, decoupled=False, clip=None, ema=None, ema_decay=0.0):
    """adam_flat_step with the extras (seld_adam_flat_ex): the gradient times clip[1] (clip: what grad_norm wrote; None:
    as it is), weight decay decoupled as torch.optim.AdamW has it, and ema <- d ema + (1 - d) param after the update
    with d = min(ema_decay, (1 + step) / (10 + step)).  All three off: the bits of adam_flat_step."""
    n = _adam_ex_buffers("adam_flat_step_ex", param, grad, exp_avg, exp_avg_sq, ema, clip, ema_decay)
    L.check(L.lib().seld_adam_flat_ex(L.ptr(param), L.ptr(grad), L.ptr(exp_avg), L.ptr(exp_avg_sq), L.ptr(ema), n, lr,
                                      beta1, beta2, eps, weight_decay, int(bool(decoupled)), int(step), grad_scale,
                                      L.ptr(clip), ema_decay, L.current_stream()), "seld_adam_flat_ex")


def adam_flat_step_state_ex(param, grad, exp_avg, exp_avg_sq, state, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                            grad_scale=1.0, decoupled=False, clip=None, ema=None, ema_decay=0.0):
    """adam_flat_step_ex with the step number and learning rate taken from the device-resident step state; the end of
    the step, as adam_flat_step_state."""
    n = _adam_ex_buffers("adam_flat_step_state_ex", param, grad, exp_avg, exp_avg_sq, ema, clip, ema_decay)
    L.check(L.lib().seld_adam_flat_state_ex(L.ptr(param), L.ptr(grad), L.ptr(exp_avg), L.ptr(exp_avg_sq), L.ptr(ema), n,
                                            beta1, beta2, eps, weight_decay, int(bool(decoupled)), grad_scale,
                                            L.ptr(clip), ema_decay, L.ptr(state), L.current_stream()),
            "seld_adam_flat_state_ex")


def stft_magphase(x, nperseg=512, noverlap=128, output_phase=True):
    """x: (C, L) float32 device tensor -> (C or 2C, nperseg/2, frames) (utility_functions.py:129-155)."""
    x = _req(x, "x")
    C, Ln = x.shape
    frames = L.lib().seld_stft_frames(Ln, nperseg, noverlap)
    if frames <= 0:
        raise L.SeldHipError("seld_stft_frames: invalid segment parameters")
    from ..utility_functions import MAX_NPERSEG, stft_workspace
    if nperseg > MAX_NPERSEG:
        raise L.SeldHipError(f"stft_magphase: nperseg={nperseg} is longer than the longest segment the HIP STFT "
                             f"transforms ({MAX_NPERSEG})")
    out = torch.empty(((2 if output_phase else 1) * C, nperseg // 2, frames), device=x.device, dtype=torch.float32)
    ws = stft_workspace(nperseg, x.device)
    L.check(L.lib().seld_stft_magphase_ws(L.ptr(x), C, Ln, nperseg, noverlap, int(bool(output_phase)), 1, 1, None,
                                          L.ptr(out), L.ptr(ws), 0 if ws is None else ws.numel(),
                                          L.current_stream()), "seld_stft_magphase_ws")
    return out



def _req_inplace(x, name, min_channels=1):
    if not x.is_cuda:
        raise L.SeldHipError(f"{name}: expected a HIP device tensor (this package has no CPU path)")
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() < 2:
        raise L.SeldHipError(f"{name}: expected a contiguous float32 (items, channels, ...) tensor, got {x.dtype} "
                             f"{tuple(x.shape)} contiguous={x.is_contiguous()}")
    if x.shape[1] < min_channels:
        raise L.SeldHipError(f"{name}: needs at least {min_channels} channels, got {x.shape[1]}")
    items, channels = x.shape[0], x.shape[1]
    hw = x.numel() // max(1, items * channels)
    return items, channels, hw


def dq_unit_norm_(x):
    """In place: channels 0..7 of every (item, f, t) position become a unit dual quaternion
    (train.py:257-275).  x: (items, >=8, F, T) float32 on the device."""
    items, channels, hw = _req_inplace(x, "dq_unit_norm_", 8)
    L.check(L.lib().seld_dq_unit_norm(L.ptr(x), items, channels, hw, L.current_stream()),
            "seld_dq_unit_norm")
    return x


def group_standardize_(x, c0, c1):
    """In place: x[:, c0:c1] <- (x[:, c0:c1] - mean) / std with one scalar mean / population std over the
    whole group (train.py:345-349).  Returns a 2-element device tensor (mean, std) as applied."""
    items, channels, hw = _req_inplace(x, "group_standardize_")
    c0, c1 = int(c0), min(int(c1), channels)        # a numpy slice clips at the channel count
    work = torch.empty(3, device=x.device, dtype=torch.float64)
    mean_std = torch.empty(2, device=x.device, dtype=torch.float32)
    L.check(L.lib().seld_group_standardize(L.ptr(x), items, channels, c0, c1, hw, L.ptr(work), L.ptr(mean_std),
                                           L.current_stream()), "seld_group_standardize")
    return mean_std



METRIC_COUNTERS = ("TP", "FP", "FN", "dc_TP", "dc_FP", "dc_FN", "dc_S", "dc_D", "dc_I", "dc_Nref", "dc_DE_TP", "dc_DE_FP",
                   "dc_DE_FN")


def metrics_new(device):
    """Zeroed accumulators for `metrics_accumulate`: (13 int64 counters, 1 double)."""
    return (torch.zeros(len(METRIC_COUNTERS), device=device, dtype=torch.int64),
            torch.zeros(1, device=device, dtype=torch.float64))


def metrics_accumulate(acc, sed, doa, target, num_frames, num_classes=14, max_overlaps=3, max_loc_value=2.0,
                       spatial_threshold=2.0, doa_threshold=20, frames_per_block=10):
    """Decode + L3DAS21 / DCASE21 counters of a batch of recordings (train.py:100-126), added to `acc`."""
    sed, doa, target = _req(sed, "sed"), _req(doa, "doa"), _req(target, "target")
    n = num_classes * max_overlaps
    if sed.dim() == 2:
        sed, doa, target = sed[None], doa[None], target[None]
    clips, frames = sed.shape[0], sed.shape[1]
    if tuple(sed.shape) != (clips, frames, n) or tuple(doa.shape) != (clips, frames, 3 * n) or \
            tuple(target.shape) != (clips, frames, 4 * n):
        raise L.SeldHipError(f"metrics_accumulate: shapes {tuple(sed.shape)} / {tuple(doa.shape)} / {tuple(target.shape)} do not "
                             f"match (clips, frames, {n}) / (.., {3 * n}) / (.., {4 * n})")
    counters, total_de = acc
    L.check(L.lib().seld_metrics_accumulate(L.ptr(sed), L.ptr(doa), L.ptr(target), clips, frames, int(num_frames),
                                            int(num_classes), int(max_overlaps), max_loc_value, spatial_threshold,
                                            doa_threshold, int(frames_per_block), L.ptr(counters), L.ptr(total_de),
                                            L.current_stream()),
            "seld_metrics_accumulate")
    return acc


def breakdown_out(out, recordings, num_classes, device, what):
    """The (counters (R, C + 2, 16) int64, total_de (R, C + 2) float64) tables of a breakdown call: `out` checked, or new
    ones (uninitialised: the calls write every entry)."""
    if num_classes < 0:
        raise L.SeldHipError(f"{what}: {num_classes} classes")
    shape = (recordings, num_classes + 2)
    if out is None:
        return (torch.empty(shape + (16,), device=device, dtype=torch.int64), torch.empty(shape, device=device, dtype=torch.float64))
    counters, total_de = out
    for t, dtype, want in ((counters, torch.int64, shape + (16,)), (total_de, torch.float64, shape)):
        if not torch.is_tensor(t) or t.device != device or t.dtype != dtype or tuple(t.shape) != want or not t.is_contiguous():
            raise L.SeldHipError(f"{what}: out must be contiguous (int64 {shape + (16,)}, float64 {shape}) tensors on {device}")
    return counters, total_de


def metrics_accumulate_by(sed, doa, target, num_frames, num_classes=14, max_overlaps=3, max_loc_value=2.0,
                          spatial_threshold=2.0, doa_threshold=20, frames_per_block=10, out=None):
    """`metrics_accumulate` broken down by recording and class (seld_metrics_breakdown, include/seld_hip.h).

    Returns (counters (R, C + 2, 16) int64 in EVENT_METRIC_COUNTERS order, total_de (R, C + 2) float64), WRITTEN into `out`
    when given (a slice of a larger table, say): rows 0 .. C - 1 the classes, row C ("other") zero on this path as are
    counters 13..15, row C + 1 ("all") what `metrics_accumulate` adds for that recording.  `class_metrics` turns the tables
    into per-class and macro scores.  Nothing is read back."""
    sed, doa, target = _req(sed, "sed"), _req(doa, "doa"), _req(target, "target")
    n = num_classes * max_overlaps
    if sed.dim() == 2:
        sed, doa, target = sed[None], doa[None], target[None]
    clips, frames = sed.shape[0], sed.shape[1]
    if tuple(sed.shape) != (clips, frames, n) or tuple(doa.shape) != (clips, frames, 3 * n) or \
            tuple(target.shape) != (clips, frames, 4 * n):
        raise L.SeldHipError(f"metrics_accumulate_by: shapes {tuple(sed.shape)} / {tuple(doa.shape)} / {tuple(target.shape)} do "
                             f"not match (clips, frames, {n}) / (.., {3 * n}) / (.., {4 * n})")
    counters, total_de = breakdown_out(out, clips, int(num_classes), sed.device, "metrics_accumulate_by")
    nbytes = L.lib().seld_metrics_breakdown_workspace(clips, frames, int(num_classes), int(frames_per_block))
    with torch.cuda.device(sed.device):
        work = scratch("metrics_breakdown", max(nbytes, 8), sed.device)
        with timed("metrics_breakdown_kernel", lambda: (0.0, float(sed.numel() * 32 + 2 * nbytes))):
            L.check(L.lib().seld_metrics_breakdown(L.ptr(sed), L.ptr(doa), L.ptr(target), clips, frames, int(num_frames),
                                                   int(num_classes), int(max_overlaps), max_loc_value, spatial_threshold,
                                                   doa_threshold, int(frames_per_block), L.ptr(counters), L.ptr(total_de),
                                                   L.ptr(work), work.numel(), L.current_stream()),
                    "seld_metrics_breakdown")
    return counters, total_de


def decode_events(sed, doa, max_loc_value=2., num_classes=14, max_overlaps=3):
    """The submission rows of resident network outputs (utility_functions.py:158-210; csrc/decode.hip).

    sed (T, n) or (R, T, n), doa (T, 3n) or (R, T, 3n), n = num_classes * max_overlaps <= 64: device tensors, both
    float32 or both float64 (a non-contiguous one is copied).  Returns, on the device,
      rows (E, 5) float64 [frame, class, x, y, z], recording-major, frame-major, slot order;
      event (E,) int32, the slot's index inside its class;
      rec_offsets (R + 1,) int64: rows[rec_offsets[r]:rec_offsets[r + 1]] belong to recording r.
    Two launches with one device-to-host read (the row count E) between them."""
    for t, name in ((sed, "sed"), (doa, "doa")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.SeldHipError(f"decode_events: {name}: expected a HIP device tensor (this package has no CPU path)")
    if sed.dtype != doa.dtype or sed.dtype not in (torch.float32, torch.float64):
        raise L.SeldHipError(f"decode_events: sed / doa must both be float32 or both float64, got {sed.dtype} / {doa.dtype}")
    if sed.device != doa.device:
        raise L.SeldHipError(f"decode_events: sed is on {sed.device}, doa on {doa.device}")
    num_classes, max_overlaps = int(num_classes), int(max_overlaps)
    n = num_classes * max_overlaps
    if num_classes <= 0 or max_overlaps <= 0 or n > 64:
        raise L.SeldHipError(f"decode_events: num_classes * max_overlaps = {num_classes} * {max_overlaps} is outside 1..64 "
                             "(one wave's ballot)")
    if sed.dim() not in (2, 3) or doa.dim() != sed.dim():
        raise L.SeldHipError(f"decode_events: expected (T, n) or (R, T, n) tensors, got {tuple(sed.shape)} / {tuple(doa.shape)}")
    if sed.dim() == 2:
        sed, doa = sed[None], doa[None]
    R, T = sed.shape[0], sed.shape[1]
    if tuple(sed.shape) != (R, T, n) or tuple(doa.shape) != (R, T, 3 * n):
        raise L.SeldHipError(f"decode_events: shapes {tuple(sed.shape)} / {tuple(doa.shape)} do not match "
                             f"(recordings, frames, {n}) / (.., {3 * n})")
    dev = sed.device
    if R == 0 or T == 0:
        return (torch.empty((0, 5), device=dev, dtype=torch.float64), torch.empty(0, device=dev, dtype=torch.int32),
                torch.zeros(R + 1, device=dev, dtype=torch.int64))
    sed, doa = sed.contiguous(), doa.contiguous()
    lib = L.lib()
    dtype = L.SELD_DECODE_F32 if sed.dtype == torch.float32 else L.SELD_DECODE_F64
    nbytes = lib.seld_decode_workspace(R, T, num_classes, max_overlaps)
    if nbytes == 0:
        raise L.SeldHipError(f"decode_events: {R} x {T} frames is more than the decode kernels index (2^31 - 1)")
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        L.check(lib.seld_decode_count(L.ptr(sed), dtype, R, T, num_classes, max_overlaps, L.ptr(ws), nbytes,
                                      L.current_stream()), "seld_decode_count")
        total = int(ws[0].item())                       # the one read-back: the outputs' size depends on the data
        rows = torch.empty((total, 5), device=dev, dtype=torch.float64)
        event = torch.empty(total, device=dev, dtype=torch.int32)
        rec_offsets = torch.empty(R + 1, device=dev, dtype=torch.int64)
        L.check(lib.seld_decode_write(L.ptr(doa), dtype, R, T, num_classes, max_overlaps, max_loc_value, L.ptr(ws),
                                      nbytes, L.ptr(rows), L.ptr(event), total, L.ptr(rec_offsets), L.current_stream()),
                "seld_decode_write")
    return rows, event, rec_offsets
