"""Scoring event lists (csrc/event_metrics.hip): the counters of location_sensitive_detection, sed_score_computation and
SELDMetrics from rows [frame, class, x, y, z] with per-recording offsets, as decode_events returns them."""
import torch

from .. import _lib as L
from ._core import timed
from .train_ops import METRIC_COUNTERS

__all__ = ["EVENT_METRIC_COUNTERS", "EVENT_METRICS_MAX_TRACKS", "event_metrics_new", "score_events", "sort_events"]

EVENT_METRIC_COUNTERS = METRIC_COUNTERS + ("sed_TP", "sed_FP", "sed_FN")
EVENT_METRICS_MAX_TRACKS = 3        # SELD_EVENT_METRICS_MAX_TRACKS: events of one class in one frame the association takes


def event_metrics_new(device):
    """Zeroed accumulators for `score_events`: (16 int64 counters in EVENT_METRIC_COUNTERS order, 1 double).  The first 13
    are METRIC_COUNTERS, so `train.test_results_from_counters` reads them unchanged."""
    return (torch.zeros(len(EVENT_METRIC_COUNTERS), device=device, dtype=torch.int64),
            torch.zeros(1, device=device, dtype=torch.float64))


def _check_side(rows, offsets, side):
    for t, name in ((rows, "rows"), (offsets, "offsets")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.SeldHipError(f"score_events: {side}_{name}: expected a HIP device tensor (this package has no CPU path)")
    if rows.dtype != torch.float64:
        raise L.SeldHipError(f"score_events: {side}_rows must be float64, got {rows.dtype}")
    if offsets.dtype != torch.int64:
        raise L.SeldHipError(f"score_events: {side}_offsets must be int64, got {offsets.dtype}")
    if rows.numel() and (rows.dim() != 2 or rows.shape[1] != 5):
        raise L.SeldHipError(f"score_events: {side}_rows must be (E, 5) [frame, class, x, y, z], got {tuple(rows.shape)}")
    if offsets.dim() != 1 or offsets.shape[0] < 1:
        raise L.SeldHipError(f"score_events: {side}_offsets must hold recordings + 1 entries, got {tuple(offsets.shape)}")
    return rows.reshape(-1, 5).contiguous(), offsets.contiguous()


def sort_events(rows, offsets):
    """`rows` reordered so that every recording's rows ascend by frame, stably: rows of one frame keep their order, which
    is their track order.  Device ops only, nothing is read back.  For lists that did not come from decode_events."""
    rows = rows.reshape(-1, 5)
    E = rows.shape[0]
    if E < 2:
        return rows
    by_frame = torch.sort(rows[:, 0], stable=True).indices
    rec = torch.searchsorted(offsets[1:].contiguous(), by_frame, right=True)
    return rows[by_frame[torch.sort(rec, stable=True).indices]].contiguous()


def score_events(acc, pred_rows, pred_offsets, true_rows, true_offsets, n_frames, nb_classes=14, spatial_threshold=2.,
                 doa_threshold=20, frames_per_block=10, flags=None):
    """Score predicted against reference event rows of a batch of recordings and add the counters to `acc`
    (seld_event_metrics_accumulate, include/seld_hip.h).

    pred_rows / true_rows: (E, 5) float64 device tensors [frame, class, x, y, z], recording-major, inside a recording
    ascending by frame (decode_events' `rows` are; sort_events orders any other list); *_offsets: (R + 1,) int64, rows
    offsets[r]:offsets[r + 1] belong to recording r (decode_events' `rec_offsets`).  A list without rows may have any
    shape with no element.  nb_classes = 0 computes the location-sensitive detection counters alone.
    Returns `acc`.

    The one device-to-host read of this function is the refusal check: the two int64 flags are read after the launch, and
    a (frame, class) cell with more than 3 events raises SeldHipError; such a call has added nothing to `acc`.  Rows whose
    frame is no integer in [0, n_frames) are left out of the detection counters and are not an error here (the drop-in
    metrics module turns them into the reference's KeyError).  With `flags` given (a device int64 tensor of two entries)
    nothing is read back and nothing is raised: the caller reads [rows with a frame out of range, overflowing cells]."""
    pred_rows, pred_offsets = _check_side(pred_rows, pred_offsets, "pred")
    true_rows, true_offsets = _check_side(true_rows, true_offsets, "true")
    if pred_offsets.shape[0] != true_offsets.shape[0]:
        raise L.SeldHipError(f"score_events: {pred_offsets.shape[0] - 1} predicted recordings against "
                             f"{true_offsets.shape[0] - 1} reference recordings")
    counters, total_de = acc
    dev = counters.device
    if any(t.device != dev for t in (total_de, pred_rows, pred_offsets, true_rows, true_offsets)):
        raise L.SeldHipError("score_events: the accumulators and the event lists are on different devices")
    if counters.dtype != torch.int64 or counters.numel() != len(EVENT_METRIC_COUNTERS) or total_de.dtype != torch.float64:
        raise L.SeldHipError(f"score_events: acc must come from event_metrics_new ({len(EVENT_METRIC_COUNTERS)} int64, 1 double)")
    read_back = flags is None
    if read_back:
        flags = torch.empty(2, device=dev, dtype=torch.int64)
    elif (not torch.is_tensor(flags) or flags.device != dev or flags.dtype != torch.int64 or flags.numel() != 2
          or not flags.is_contiguous()):
        raise L.SeldHipError("score_events: flags must be a contiguous int64 device tensor of two entries")
    R = pred_offsets.shape[0] - 1
    Ep, Et = pred_rows.shape[0], true_rows.shape[0]
    with torch.cuda.device(dev):
        with timed("event_metrics_kernel", lambda: (0.0, float((Ep + Et) * (40 + 16) + 2 * (R + 1) * 8))):
            L.check(L.lib().seld_event_metrics_accumulate(
                L.ptr(pred_rows), L.ptr(pred_offsets), Ep, L.ptr(true_rows), L.ptr(true_offsets), Et, R, int(n_frames),
                int(nb_classes), int(frames_per_block), float(spatial_threshold), float(doa_threshold), L.ptr(counters),
                L.ptr(total_de), L.ptr(flags), L.current_stream()), "seld_event_metrics_accumulate")
        if read_back:
            cells = int(flags[1].item())                # the one read-back
            if cells:
                raise L.SeldHipError(f"score_events: {cells} (recording, frame, class) cells hold more than "
                                     f"{EVENT_METRICS_MAX_TRACKS} events; the track association takes "
                                     f"{EVENT_METRICS_MAX_TRACKS} x {EVENT_METRICS_MAX_TRACKS} at most")
    return acc
