"""Whole-recording inference (csrc/ensemble.hip): the model inputs of a batch of sliding windows, each under one row of
an FOA transform table, cut straight out of the resident recordings; and the members' outputs combined into one track
per recording -- DOAs mapped back through their row, the slots of a (frame, class) aligned to an anchor, a weighted mean
over windows and transforms.  include/seld_hip.h has the definitions."""
import numpy as np
import torch

from .. import _lib as L
from ._core import _req, timed
from .loader import _check_table

__all__ = ["window_batch", "ensemble_combine", "window_count", "ensemble_window", "ensemble_table"]
ENSEMBLE_MAX_SLOTS = 64


def window_count(length, seg_len, hop):
    """max(1, ceil((length - seg_len) / hop) + 1): the fewest windows of seg_len frames every hop frames that cover
    `length` frames.  NOT `segment`'s default len(range(0, length, hop)), the reference's count, which goes on to
    windows that start inside the recording but hold mostly padding (length 4800, seg_len 512, hop 256: 18 against 19)."""
    length, seg_len, hop = int(length), int(seg_len), int(hop)
    if length < 1 or seg_len < 1 or hop < 1:
        raise L.SeldHipError(f"window_count: length, seg_len and hop must be positive, got {length}, {seg_len}, {hop}")
    return max(1, -(-(length - seg_len) // hop) + 1)


def ensemble_table(table, device, channels=None):
    """A transform table (K, 2 * C + 6), e.g. `foa_transforms(...)`, validated on the host and uploaded once: the int32
    device tensor that `window_batch` and `ensemble_combine` then take without looking at its content again."""
    if torch.is_tensor(table) and getattr(table, "_seld_table_checked", False) and table.device == torch.device(device):
        if channels is not None and (table.shape[1] - 6) // 2 != int(channels):
            raise L.SeldHipError(f"the transform table is for {(table.shape[1] - 6) // 2} channels, not {channels}")
        return table
    t = torch.from_numpy(_check_table(table, channels)).to(device)
    t._seld_table_checked = True
    return t


def _table_on(table, channels, device):
    """(int32 device tensor or None, K, C) of a transform table given as None, an array or a tensor."""
    if table is None:
        return None, 0, 0
    t = ensemble_table(table, device, channels)
    return t, t.shape[0], (t.shape[1] - 6) // 2


def window_batch(x, out, *, seg_len, hop, segments, table=None, first=0, count=None):
    """out[b] = the model input of member first + b for b < count, in ONE launch (seld_window_batch).

    x (R, C, F, L): the resident recordings; out (B, C, F, seg_len): the batch buffer, both contiguous fp32 on one device.
    Members are numbered m = (r * segments + s) * K + k: window s of recording r (frames s * hop ... s * hop + seg_len,
    zero past L) under row k of `table` (K, 2 * C + 6), e.g. `foa_transforms(...)`; None: the identity, K = 1.  The
    result is byte for byte `segment` followed by the training transform of `gather_rows_aug`.  count defaults to
    min(B, members - first); rows [count, B) of `out` are left alone."""
    what = "window_batch"
    if _req(x, f"{what}: x") is not x or x.dim() != 4:
        raise L.SeldHipError(f"{what}: x must be a contiguous (R, C, F, L) array")
    R, C, F, length = x.shape
    seg_len, hop, segments, first = int(seg_len), int(hop), int(segments), int(first)
    if _req(out, f"{what}: out") is not out or out.dim() != 4 or tuple(out.shape[1:]) != (C, F, seg_len):
        raise L.SeldHipError(f"{what}: out must be a contiguous (B, {C}, {F}, {seg_len}) array, got {tuple(out.shape)}")
    if out.device != x.device:
        raise L.SeldHipError(f"{what}: tensors on different devices")
    table, K, _ = _table_on(table, C, x.device)
    B = out.shape[0]
    members = R * segments * max(K, 1)
    count = min(B, members - first) if count is None else int(count)
    with torch.cuda.device(x.device):
        with timed("window_batch_kernel", lambda: (0.0, float(8 * count * C * F * seg_len))):
            L.check(L.lib().seld_window_batch(L.ptr(x), R, C, F, length, seg_len, hop, segments, L.ptr(table), K, first, B,
                                              count, L.ptr(out), L.current_stream()), "seld_window_batch")
    return out


def ensemble_window(window, t_out, device):
    """The T_out weights of `ensemble_combine` as a fp32 device tensor: "uniform" (ones), "triangular"
    (win[j] = min(j + 1, T_out - j)) or a tensor / array of T_out positive finite weights, validated on the host."""
    t_out = int(t_out)
    if isinstance(window, str):
        if window == "uniform":
            w = np.ones(t_out, dtype=np.float32)
        elif window == "triangular":
            j = np.arange(t_out)
            w = np.minimum(j + 1, t_out - j).astype(np.float32)
        else:
            raise L.SeldHipError(f"ensemble_combine: window must be 'uniform', 'triangular' or {t_out} weights, got {window!r}")
        return torch.from_numpy(w).to(device)
    host = np.asarray(window.detach().cpu() if torch.is_tensor(window) else window, dtype=np.float32).reshape(-1)
    if host.shape[0] != t_out:
        raise L.SeldHipError(f"ensemble_combine: {host.shape[0]} window weights for {t_out} output frames")
    if not (np.isfinite(host).all() and (host > 0).all()):
        raise L.SeldHipError("ensemble_combine: window weights must be positive and finite")
    if torch.is_tensor(window) and window.is_cuda and window.dtype == torch.float32 and window.is_contiguous() and \
            window.dim() == 1 and window.device == torch.device(device):
        return window
    return torch.from_numpy(np.ascontiguousarray(host)).to(device)


def ensemble_combine(sed, doa, *, recordings, segments, hop_out, frames, classes=14, overlaps=3, table=None,
                     window="triangular", align=True, return_perm=False):
    """One track per recording out of the members' outputs, in ONE launch (seld_ensemble_combine).

    sed (M, T_out, n), doa (M, T_out, 3 * n): what the model gave for the members m = (r * segments + s) * K + k of
    `window_batch`, M = recordings * segments * K, n = classes * overlaps <= 64.  hop_out: the hop in output frames;
    frames: output frames per recording.  Every (frame, class) takes the windows that cover it under every row of
    `table` (None: K = 1), maps the DOAs back through the row, with `align` (at most 3 overlaps) pairs each member's slots
    with those of the anchor (the covering window of the largest weight, row 0) at the least squared distance, and
    writes the mean weighted by `window`: "uniform", "triangular" or T_out positive finite weights.  Frames no window
    covers are zeros.  Returns (sed (recordings, frames, n), doa (recordings, frames, 3 * n)) and with return_perm the
    chosen permutation indices (M, T_out, classes) int32, -1 past `frames`."""
    what = "ensemble_combine"
    if _req(sed, f"{what}: sed") is not sed or _req(doa, f"{what}: doa") is not doa:
        raise L.SeldHipError(f"{what}: sed and doa must be contiguous")
    R, S, hop_out, frames, classes, overlaps = (int(v) for v in (recordings, segments, hop_out, frames, classes, overlaps))
    n = classes * overlaps
    table, K, C = _table_on(table, None, sed.device)
    M = R * S * max(K, 1)
    if sed.dim() != 3 or sed.shape[0] != M or sed.shape[2] != n or tuple(doa.shape) != (M, sed.shape[1], 3 * n) or \
            doa.device != sed.device:
        raise L.SeldHipError(f"{what}: expected sed ({M}, T_out, {n}) and doa ({M}, T_out, {3 * n}) on one device, got "
                             f"{tuple(sed.shape)} / {tuple(doa.shape)}")
    T_out = sed.shape[1]
    if min(R, S, hop_out, frames, classes, overlaps, T_out) < 1:
        raise L.SeldHipError(f"{what}: a non-positive extent")
    if n > ENSEMBLE_MAX_SLOTS:
        raise L.SeldHipError(f"{what}: classes * overlaps = {n} is above {ENSEMBLE_MAX_SLOTS}")
    if align and overlaps > 3:
        raise L.SeldHipError(f"{what}: the alignment searches the pairings of at most 3 slots per class, got {overlaps}")
    win = ensemble_window(window, T_out, sed.device)
    out_sed = torch.empty((R, frames, n), device=sed.device)
    out_doa = torch.empty((R, frames, 3 * n), device=sed.device)
    perm = torch.empty((M, T_out, classes), device=sed.device, dtype=torch.int32) if return_perm else None
    nbytes = 4 * (sed.numel() + doa.numel() + out_sed.numel() + out_doa.numel() + (perm.numel() if return_perm else 0))
    with torch.cuda.device(sed.device):
        with timed("ensemble_combine_kernel", lambda: (0.0, float(nbytes))):
            L.check(L.lib().seld_ensemble_combine(L.ptr(sed), L.ptr(doa), R, S, K, T_out, hop_out, frames, classes, overlaps,
                                                  L.ptr(win), L.ptr(table), C, int(bool(align)), L.ptr(out_sed),
                                                  L.ptr(out_doa), L.ptr(perm), L.current_stream()),
                    "seld_ensemble_combine")
    return (out_sed, out_doa, perm) if return_perm else (out_sed, out_doa)
