"""Track post-processing (csrc/smooth.hip): a median filter on the activity, two thresholds with hysteresis, gap filling,
a minimum duration and one DOA per event, applied to a resident track between the network (or `ensemble_combine`) and
`decode_events` / `metrics_accumulate`; and the event list of any track.  include/seld_hip.h has the definitions."""
import dataclasses
import math

import torch

from .. import _lib as L
from ._core import _req, timed

__all__ = ["PostProcess", "smooth_tracks", "track_events", "SMOOTH_MAX_MEDIAN", "SMOOTH_MAX_FRAMES", "SMOOTH_DOA_MODES"]

SMOOTH_MAX_MEDIAN = 31              # SELD_SMOOTH_MAX_MEDIAN
SMOOTH_MAX_FRAMES = 16384           # SELD_SMOOTH_MAX_FRAMES: frames of a column the kernel holds in LDS
SMOOTH_DOA_MODES = {"frame": 0, "mean": 1, "weighted": 2}       # SELD_SMOOTH_DOA_*


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


@dataclasses.dataclass(frozen=True)
class PostProcess:
    """The six settings of `smooth_tracks`, validated when made (host only: nothing here touches the device).
    median: odd window of the activity's median filter (1: none); on / off: the hysteresis thresholds, a stretch of
    p > off is an event iff it holds a frame with p > on; min_frames: shorter events are dropped; max_gap: inactive
    stretches of at most so many frames between two events are filled; doa: "frame" (as given), "mean" or "weighted"
    (by the filtered activity) -- one DOA per event."""
    median: int = 1
    on: float = 0.5
    off: float = 0.5
    min_frames: int = 1
    max_gap: int = 0
    doa: str = "frame"

    def __post_init__(self):
        if not _is_int(self.median) or self.median % 2 == 0 or not 1 <= self.median <= SMOOTH_MAX_MEDIAN:
            raise ValueError(f"median must be an odd integer in 1 .. {SMOOTH_MAX_MEDIAN}, got {self.median!r}")
        for name in ("on", "off"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not 0.0 <= v <= 1.0:
                raise ValueError(f"{name} must be a finite number in [0, 1], got {v!r}")
        if self.off > self.on:
            raise ValueError(f"off ({self.off}) must not be above on ({self.on})")
        if not _is_int(self.min_frames) or self.min_frames < 1:
            raise ValueError(f"min_frames must be an integer of at least 1, got {self.min_frames!r}")
        if not _is_int(self.max_gap) or self.max_gap < 0:
            raise ValueError(f"max_gap must be a non-negative integer, got {self.max_gap!r}")
        if self.doa not in SMOOTH_DOA_MODES:
            raise ValueError(f"doa must be one of {', '.join(SMOOTH_DOA_MODES)}, got {self.doa!r}")

    @property
    def is_identity(self):
        """True when `decode_events` / `metrics_accumulate` see the same events with and without these settings for
        activities in [0, 1]: callers skip the launch."""
        return (self.median == 1 and self.on == 0.5 and self.off == 0.5 and self.min_frames == 1 and self.max_gap == 0
                and self.doa == "frame")

    def kwargs(self):
        return dataclasses.asdict(self)


def _track(what, sed, doa):
    """(sed (R, T, n), doa (R, T, 3n), squeeze) contiguous fp32 on one device, of (T, n) or (R, T, n) inputs."""
    for t, name in ((sed, "sed"), (doa, "doa")):
        if not torch.is_tensor(t):
            raise L.SeldHipError(f"{what}: {name}: expected a HIP device tensor (this package has no CPU path)")
    sed, doa = _req(sed, f"{what}: sed"), _req(doa, f"{what}: doa")
    if sed.device != doa.device:
        raise L.SeldHipError(f"{what}: sed is on {sed.device}, doa on {doa.device}")
    if sed.dim() not in (2, 3) or doa.dim() != sed.dim():
        raise L.SeldHipError(f"{what}: expected (T, n) or (R, T, n) tensors, got {tuple(sed.shape)} / {tuple(doa.shape)}")
    squeeze = sed.dim() == 2
    if squeeze:
        sed, doa = sed[None], doa[None]
    R, T, n = sed.shape
    if min(R, T, n) < 1 or tuple(doa.shape) != (R, T, 3 * n):
        raise L.SeldHipError(f"{what}: shapes {tuple(sed.shape)} / {tuple(doa.shape)} do not match (recordings, frames, n) / "
                             "(.., 3 n) with every extent positive")
    return sed, doa, squeeze


def smooth_tracks(sed, doa_in, /, *, median=1, on=0.5, off=0.5, min_frames=1, max_gap=0, doa="frame", return_prob=False):
    """Post-process a resident track in ONE launch (seld_smooth_tracks): per column (recording, slot) the activity's
    median over `median` frames (edges replicated), hysteresis (a stretch of p > off is kept iff it holds a frame with
    p > on; both strict, compared in fp32), inactive stretches of at most `max_gap` frames between two events filled,
    then events shorter than `min_frames` dropped; doa="mean" / "weighted" gives every event the (activity-weighted)
    mean of its frames' DOAs, summed in double, "frame" copies them.

    smooth_tracks(sed, doa, *, ...): the two tensors are positional, sed (T, n) or (R, T, n), doa (T, 3n) or (R, T, 3n),
    fp32 on the device, T <= SMOOTH_MAX_FRAMES.  Returns (out_sed of 0.0 / 1.0, out_doa) in the input's shape on the
    device, and with return_prob the filtered activity as a third.  Everything is validated on the host first (the rules
    of `PostProcess`); no host read, so the call can be recorded in a graph."""
    what = "smooth_tracks"
    try:
        post = PostProcess(median=median, on=on, off=off, min_frames=min_frames, max_gap=max_gap, doa=doa)
    except ValueError as err:
        raise L.SeldHipError(f"{what}: {err}") from None
    doa = doa_in
    sed, doa, squeeze = _track(what, sed, doa)
    R, T, n = sed.shape
    if T > SMOOTH_MAX_FRAMES:
        raise L.SeldHipError(f"{what}: {T} frames; the kernel holds a column of at most {SMOOTH_MAX_FRAMES} in LDS")
    out_sed, out_doa = torch.empty_like(sed), torch.empty_like(doa)
    prob = torch.empty_like(sed) if return_prob else None
    nbytes = 4 * (sed.numel() + doa.numel()) * 2 + (4 * sed.numel() if return_prob else 0)
    with torch.cuda.device(sed.device):
        with timed("smooth_tracks_kernel", lambda: (0.0, float(nbytes))):
            L.check(L.lib().seld_smooth_tracks(L.ptr(sed), L.ptr(doa), R, T, n, post.median, post.on, post.off, post.min_frames,
                                               post.max_gap, SMOOTH_DOA_MODES[post.doa], L.ptr(out_sed), L.ptr(out_doa),
                                               L.ptr(prob), L.current_stream()), "seld_smooth_tracks")
    outs = (out_sed, out_doa) + ((prob,) if return_prob else ())
    return tuple(t[0] for t in outs) if squeeze else outs


def track_events(sed, doa, max_loc_value=2., num_classes=14, max_overlaps=3):
    """The event list of a resident track (seld_track_events_*): every maximal stretch of frames with sed > 0.5 in a column
    is one event.  For the 0 / 1 output of `smooth_tracks` and for activities in [0, 1] this is `decode_events`' rule;
    outside [0, 1] it is not its rint, and its frame-sum rule is not applied.

    sed (T, n) or (R, T, n), doa (T, 3n) or (R, T, 3n), n = num_classes * max_overlaps: fp32 device tensors.  Returns, on
    the device,
      events (E, 8) float64 [recording, class, slot, onset, offset (exclusive), x, y, z], x, y, z the mean of the event's
        DOAs (summed in double) times max_loc_value; ordered by recording, then column, then onset;
      rec_offsets (R + 1,) int64: events[rec_offsets[r]:rec_offsets[r + 1]] belong to recording r.
    Two calls with one device-to-host read (the event count E) between them."""
    what = "track_events"
    sed, doa, _ = _track(what, sed, doa)
    R, T, n = sed.shape
    num_classes, max_overlaps = int(num_classes), int(max_overlaps)
    if num_classes < 1 or max_overlaps < 1 or num_classes * max_overlaps != n:
        raise L.SeldHipError(f"{what}: {n} columns are not {num_classes} classes x {max_overlaps} overlaps")
    lib, dev = L.lib(), sed.device
    nbytes = lib.seld_track_events_workspace(R, T, n)
    if nbytes == 0:
        raise L.SeldHipError(f"{what}: {R} x {T} x {n} is more than the kernels index (2^31 - 1 segments of 64 frames)")
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        L.check(lib.seld_track_events_count(L.ptr(sed), R, T, n, L.ptr(ws), nbytes, L.current_stream()),
                "seld_track_events_count")
        total = int(ws[0].item())                       # the one read-back: the output's size depends on the data
        events = torch.empty((total, 8), device=dev, dtype=torch.float64)
        rec_offsets = torch.empty(R + 1, device=dev, dtype=torch.int64)
        L.check(lib.seld_track_events_write(L.ptr(sed), L.ptr(doa), R, T, num_classes, max_overlaps, float(max_loc_value),
                                            L.ptr(ws), nbytes, L.ptr(events), total, L.ptr(rec_offsets), L.current_stream()),
                "seld_track_events_write")
    return events, rec_offsets
