"""Scoring event lists (csrc/event_metrics.hip): the counters of location_sensitive_detection, sed_score_computation and
SELDMetrics from rows [frame, class, x, y, z] with per-recording offsets, as decode_events returns them, or from rows
[frame, class, azimuth, elevation] in degrees; and the track association alone (assign_doas)."""
import numpy as np
import torch

from .. import _lib as L
from ._core import scratch, timed
from .train_ops import METRIC_COUNTERS, breakdown_out

__all__ = ["EVENT_METRIC_COUNTERS", "EVENT_METRICS_MAX_TRACKS", "EVENT_METRICS_MAX_TRACKS_EX", "assign_doas",
           "event_metrics_new", "score_events", "score_events_by", "sort_events"]

EVENT_METRIC_COUNTERS = METRIC_COUNTERS + ("sed_TP", "sed_FP", "sed_FN")
EVENT_METRICS_MAX_TRACKS = 3        # SELD_EVENT_METRICS_MAX_TRACKS: events of one class in one frame the association takes
EVENT_METRICS_MAX_TRACKS_EX = 8     # SELD_EVENT_METRICS_MAX_TRACKS_EX: the most `max_tracks` can ask for


def event_metrics_new(device):
    """Zeroed accumulators for `score_events`: (16 int64 counters in EVENT_METRIC_COUNTERS order, 1 double).  The first 13
    are METRIC_COUNTERS, so `evaluate.test_results_from_counters` reads them unchanged."""
    return (torch.zeros(len(EVENT_METRIC_COUNTERS), device=device, dtype=torch.int64),
            torch.zeros(1, device=device, dtype=torch.float64))


def _check_side(rows, offsets, side, coords=3):
    for t, name in ((rows, "rows"), (offsets, "offsets")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.SeldHipError(f"score_events: {side}_{name}: expected a HIP device tensor (this package has no CPU path)")
    if rows.dtype != torch.float64:
        raise L.SeldHipError(f"score_events: {side}_rows must be float64, got {rows.dtype}")
    if offsets.dtype != torch.int64:
        raise L.SeldHipError(f"score_events: {side}_offsets must be int64, got {offsets.dtype}")
    if rows.numel() and (rows.dim() != 2 or rows.shape[1] != 2 + coords):
        what = "[frame, class, x, y, z]" if coords == 3 else "[frame, class, azimuth, elevation]"
        raise L.SeldHipError(f"score_events: {side}_rows must be (E, {2 + coords}) {what}, got {tuple(rows.shape)}")
    if offsets.dim() != 1 or offsets.shape[0] < 1:
        raise L.SeldHipError(f"score_events: {side}_offsets must hold recordings + 1 entries, got {tuple(offsets.shape)}")
    return rows.reshape(-1, 2 + coords).contiguous(), offsets.contiguous()


def sort_events(rows, offsets):
    """`rows` reordered so that every recording's rows ascend by frame, stably: rows of one frame keep their order, which
    is their track order.  Device ops only, nothing is read back.  For lists that did not come from decode_events.
    Rows of 5 (Cartesian) or 4 (spherical) columns."""
    rows = rows.reshape(-1, rows.shape[-1] if rows.dim() == 2 and rows.shape[-1] in (4, 5) else 5)
    E = rows.shape[0]
    if E < 2:
        return rows
    by_frame = torch.sort(rows[:, 0], stable=True).indices
    rec = torch.searchsorted(offsets[1:].contiguous(), by_frame, right=True)
    return rows[by_frame[torch.sort(rec, stable=True).indices]].contiguous()


def _check_lists(pred_rows, pred_offsets, true_rows, true_offsets, coords, max_tracks):
    """The checks score_events and score_events_by share; returns the four tensors as the library takes them."""
    if coords not in (2, 3):
        raise L.SeldHipError(f"score_events: coords must be 3 (x, y, z) or 2 (azimuth, elevation in degrees), got {coords!r}")
    if isinstance(max_tracks, bool) or not isinstance(max_tracks, (int, np.integer)) \
            or not 1 <= max_tracks <= EVENT_METRICS_MAX_TRACKS_EX:
        raise L.SeldHipError(f"score_events: max_tracks must be an integer in 1 .. {EVENT_METRICS_MAX_TRACKS_EX}, "
                             f"got {max_tracks!r}")
    pred_rows, pred_offsets = _check_side(pred_rows, pred_offsets, "pred", coords)
    true_rows, true_offsets = _check_side(true_rows, true_offsets, "true", coords)
    if pred_offsets.shape[0] != true_offsets.shape[0]:
        raise L.SeldHipError(f"score_events: {pred_offsets.shape[0] - 1} predicted recordings against "
                             f"{true_offsets.shape[0] - 1} reference recordings")
    return pred_rows, pred_offsets, true_rows, true_offsets


def _check_flags(flags, dev):
    """(flags, read_back): a new pair of flags that the call reads back itself, or the caller's, checked."""
    if flags is None:
        return torch.empty(2, device=dev, dtype=torch.int64), True
    if (not torch.is_tensor(flags) or flags.device != dev or flags.dtype != torch.int64 or flags.numel() != 2
            or not flags.is_contiguous()):
        raise L.SeldHipError("score_events: flags must be a contiguous int64 device tensor of two entries")
    return flags, False


def _raise_if_refused(flags, max_tracks):
    cells = int(flags[1].item())                        # the one read-back
    if cells:
        raise L.SeldHipError(f"score_events: {cells} (recording, frame, class) cells hold more than "
                             f"{max_tracks} events; the track association takes "
                             f"{max_tracks} x {max_tracks} at most (max_tracks = {max_tracks}, up to "
                             f"{EVENT_METRICS_MAX_TRACKS_EX} can be asked for)")


def score_events(acc, pred_rows, pred_offsets, true_rows, true_offsets, n_frames, nb_classes=14, spatial_threshold=2.,
                 doa_threshold=20, frames_per_block=10, coords=3, max_tracks=EVENT_METRICS_MAX_TRACKS, flags=None):
    """Score predicted against reference event rows of a batch of recordings and add the counters to `acc`
    (seld_event_metrics_accumulate_ex, include/seld_hip.h).

    pred_rows / true_rows: (E, 5) float64 device tensors [frame, class, x, y, z], recording-major, inside a recording
    ascending by frame (decode_events' `rows` are; sort_events orders any other list); *_offsets: (R + 1,) int64, rows
    offsets[r]:offsets[r + 1] belong to recording r (decode_events' `rec_offsets`).  A list without rows may have any
    shape with no element.  nb_classes = 0 computes the location-sensitive detection counters alone.
    coords = 2: the rows are (E, 4) [frame, class, azimuth, elevation] in degrees; the DCASE21 counters (3-12) and the
    class-only detection (13-15) are computed, and nothing is added to the Euclidean counters 0-2.
    max_tracks (1 .. EVENT_METRICS_MAX_TRACKS_EX = 8): the events of one class in one frame the track association takes.
    Returns `acc`.

    The one device-to-host read of this function is the refusal check: the two int64 flags are read after the launch, and
    a (frame, class) cell with more than `max_tracks` events raises SeldHipError; such a call has added nothing to `acc`.  Rows whose
    frame is no integer in [0, n_frames) are left out of the detection counters and are not an error here (the drop-in
    metrics module turns them into the reference's KeyError).  With `flags` given (a device int64 tensor of two entries)
    nothing is read back and nothing is raised: the caller reads [rows with a frame out of range, overflowing cells]."""
    pred_rows, pred_offsets, true_rows, true_offsets = _check_lists(pred_rows, pred_offsets, true_rows, true_offsets, coords,
                                                                    max_tracks)
    counters, total_de = acc
    dev = counters.device
    if any(t.device != dev for t in (total_de, pred_rows, pred_offsets, true_rows, true_offsets)):
        raise L.SeldHipError("score_events: the accumulators and the event lists are on different devices")
    if counters.dtype != torch.int64 or counters.numel() != len(EVENT_METRIC_COUNTERS) or total_de.dtype != torch.float64:
        raise L.SeldHipError(f"score_events: acc must come from event_metrics_new ({len(EVENT_METRIC_COUNTERS)} int64, 1 double)")
    flags, read_back = _check_flags(flags, dev)
    R = pred_offsets.shape[0] - 1
    Ep, Et = pred_rows.shape[0], true_rows.shape[0]
    with torch.cuda.device(dev):
        with timed("event_metrics_kernel", lambda: (0.0, float((Ep + Et) * (8 * (2 + coords) + 16) + 2 * (R + 1) * 8))):
            L.check(L.lib().seld_event_metrics_accumulate_ex(
                L.ptr(pred_rows), L.ptr(pred_offsets), Ep, L.ptr(true_rows), L.ptr(true_offsets), Et, R, int(n_frames),
                int(nb_classes), int(frames_per_block), coords, int(max_tracks), float(spatial_threshold), float(doa_threshold),
                L.ptr(counters), L.ptr(total_de), L.ptr(flags), L.current_stream()), "seld_event_metrics_accumulate_ex")
        if read_back:
            _raise_if_refused(flags, max_tracks)
    return acc


def score_events_by(pred_rows, pred_offsets, true_rows, true_offsets, n_frames, nb_classes=14, spatial_threshold=2.,
                    doa_threshold=20, frames_per_block=10, coords=3, max_tracks=EVENT_METRICS_MAX_TRACKS, flags=None, out=None):
    """`score_events` broken down by recording and class (seld_event_metrics_breakdown, include/seld_hip.h): the lists, the
    checks, the flags and the refusal rule are score_events'.

    Returns (counters (R, C + 2, 16) int64 in EVENT_METRIC_COUNTERS order, total_de (R, C + 2) float64), C = nb_classes,
    WRITTEN (not added to) into `out` when given, so successive batches can go to successive slices of one table.  Rows
    0 .. C - 1: what each class contributes (S, D, I class-wise, the detection counters row by row); row C ("other"): the
    rows whose class is no integer in [0, C), which only the detection counters see; row C + 1 ("all"): what
    `score_events` adds to `acc` for that recording.  A call refused for an overflowing cell has written zeros.
    `class_metrics` turns the tables into per-class scores, macro averages and leave-one-recording-out estimates."""
    pred_rows, pred_offsets, true_rows, true_offsets = _check_lists(pred_rows, pred_offsets, true_rows, true_offsets, coords,
                                                                    max_tracks)
    dev = pred_rows.device
    if any(t.device != dev for t in (pred_offsets, true_rows, true_offsets)):
        raise L.SeldHipError("score_events_by: the event lists are on different devices")
    R = pred_offsets.shape[0] - 1
    counters, total_de = breakdown_out(out, R, int(nb_classes), dev, "score_events_by")
    flags, read_back = _check_flags(flags, dev)
    Ep, Et = pred_rows.shape[0], true_rows.shape[0]
    nbytes = L.lib().seld_metrics_breakdown_workspace(R, int(n_frames), int(nb_classes), int(frames_per_block))
    with torch.cuda.device(dev):
        work = scratch("metrics_breakdown", max(nbytes, 8), dev)
        with timed("event_breakdown_kernel",
                   lambda: (0.0, float((Ep + Et) * (8 * (2 + coords) + 16) + 2 * (R + 1) * 8 + 2 * nbytes))):
            L.check(L.lib().seld_event_metrics_breakdown(
                L.ptr(pred_rows), L.ptr(pred_offsets), Ep, L.ptr(true_rows), L.ptr(true_offsets), Et, R, int(n_frames),
                int(nb_classes), int(frames_per_block), coords, int(max_tracks), float(spatial_threshold), float(doa_threshold),
                L.ptr(counters), L.ptr(total_de), L.ptr(work), work.numel(), L.ptr(flags), L.current_stream()),
                "seld_event_metrics_breakdown")
        if read_back:
            _raise_if_refused(flags, max_tracks)
    return counters, total_de


def assign_doas(gt, pred, gt_counts, pred_counts, spherical=False):
    """The reference's least_distance_between_gt_pred for a batch of B problems on the device (seld_least_distance,
    include/seld_hip.h), with the device functions of the scoring kernel.

    gt / pred: (B, 8, C) float64 device tensors, C = 3 (x, y, z) or, with spherical=True, C = 2 (azimuth, elevation in
    radians); gt_counts / pred_counts: (B,) int32 device tensors, how many of the 8 DOAs of each problem are there (forced
    into 0 .. 8 on the device).  Returns device tensors (cost (B, 8) float64, row (B, 8) int32, col (B, 8) int32, pairs
    (B,) int32): the first pairs[b] = min(g, q) entries of a problem are its matched pairs, rows ascending as scipy
    returns them; the others are 0 / -1 / -1.  Nothing is read back."""
    C = 2 if spherical else 3
    for t, name in ((gt, "gt"), (pred, "pred")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.SeldHipError(f"assign_doas: {name}: expected a HIP device tensor (this package has no CPU path)")
        if t.dtype != torch.float64 or t.dim() != 3 or t.shape[1] != EVENT_METRICS_MAX_TRACKS_EX or t.shape[2] != C:
            raise L.SeldHipError(f"assign_doas: {name} must be (B, {EVENT_METRICS_MAX_TRACKS_EX}, {C}) float64, got "
                                 f"{tuple(t.shape)} {t.dtype}")
    B, dev = gt.shape[0], gt.device
    if pred.shape[0] != B or pred.device != dev:
        raise L.SeldHipError("assign_doas: gt and pred differ in their problem count or device")
    for t, name in ((gt_counts, "gt_counts"), (pred_counts, "pred_counts")):
        if not torch.is_tensor(t) or t.device != dev or t.dtype != torch.int32 or tuple(t.shape) != (B,):
            raise L.SeldHipError(f"assign_doas: {name} must be a ({B},) int32 tensor on {dev}")
    gt, pred, gt_counts, pred_counts = (t.contiguous() for t in (gt, pred, gt_counts, pred_counts))
    cost = torch.empty((B, EVENT_METRICS_MAX_TRACKS_EX), device=dev, dtype=torch.float64)
    row = torch.empty((B, EVENT_METRICS_MAX_TRACKS_EX), device=dev, dtype=torch.int32)
    col = torch.empty_like(row)
    pairs = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        with timed("least_distance_kernel", lambda: (0.0, float(B * (2 * 8 * 8 * C + 8 * 16 + 12)))):
            L.check(L.lib().seld_least_distance(L.ptr(gt), L.ptr(gt_counts), L.ptr(pred), L.ptr(pred_counts), B, C,
                                                L.ptr(cost), L.ptr(row), L.ptr(col), L.ptr(pairs), L.current_stream()),
                    "seld_least_distance")
    return cost, row, col, pairs
