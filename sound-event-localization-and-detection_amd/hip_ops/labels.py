"""Target encoding and segmentation (csrc/labels.hip): event rows -> dense [activity | location] target, and the
overlapping zero-padded cut of features, targets and waveforms into training segments."""
import numpy as np
import torch

from .. import _lib as L
from ._core import timed

__all__ = ["event_frames", "encode_events", "segment", "ENCODE_MAX_EVENTS"]

ENCODE_MAX_EVENTS = 4096            # SELD_ENCODE_MAX_EVENTS: events of one recording the kernel stages in LDS


def event_frames(start, end, dur=60, step=0.1):
    """First and last frame (inclusive, int64 numpy arrays) of events given by their start and end times in seconds:
    the reference's `quantize` and `get_frame` (utility_functions.py:226-228) -- round(x / step) * step, half to even,
    then int(np.interp(x, (0, dur), (0, num_frames - 1))) -- over whole arrays.  Host-side on purpose: it runs over
    tens of events, and np.interp's rounding is the contract."""
    num_frames = int(dur / step)

    def frame(x):
        x = np.asarray(x, dtype=np.float64)
        q = np.rint(x / step) * step
        return np.interp(q, (0, dur), (0, num_frames - 1)).astype(np.int64)
    return frame(start), frame(end)


def _device():
    if not torch.cuda.is_available():
        raise L.SeldHipError("encode_events: no HIP device (this package has no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def encode_events(first, last, cls, xyz, rec_offsets, frames, classes=14, overlaps=3, max_loc_value=2., no_overlaps=False,
                  dtype=torch.float64, out=None, counters=None):
    """The dense target of a batch of recordings from their event rows (utility_functions.py:219-267; csrc/labels.hip),
    the inverse of decode_events.

    first, last (E,): inclusive frame range of every event; cls (E,): class id; xyz (E, 3): position; rec_offsets
    (R + 1,): events rec_offsets[r]:rec_offsets[r + 1] belong to recording r.  Either all host data (numpy arrays,
    lists), which is checked here before anything is launched, or all device tensors, which the kernel checks.
    Returns the (R, frames, 4 * classes * overlaps) device tensor -- (R, frames, 4 * classes) with no_overlaps -- of
    `dtype` (torch.float64 or torch.float32): per frame [cl | loc], loc = xyz / max_loc_value divided in double.
    `out`: a contiguous device tensor of that shape and dtype to fill instead (every element is written).
    Raises IndexError where more than `overlaps` events of one class share a frame, as the reference does, and
    SeldHipError for a frame or class out of range, after ONE read-back of two integers.  `counters`: a device int32
    tensor of two entries; given, nothing is read back (the call can be recorded in a graph) and the caller inspects
    [overflowing cells, invalid events] itself."""
    frames, classes, overlaps = int(frames), int(classes), int(overlaps)
    if dtype not in (torch.float32, torch.float64):
        raise L.SeldHipError(f"encode_events: dtype must be torch.float32 or torch.float64, got {dtype}")
    if frames <= 0 or classes <= 0 or overlaps <= 0:
        raise L.SeldHipError(f"encode_events: frames, classes and overlaps must be positive, got {frames}, {classes}, {overlaps}")
    if classes * overlaps > 64:
        raise L.SeldHipError(f"encode_events: classes * overlaps = {classes} * {overlaps} is more than 64")
    args = (first, last, cls, xyz, rec_offsets)
    on_device = [torch.is_tensor(a) and a.is_cuda for a in args]
    if any(on_device) and not all(on_device):
        raise L.SeldHipError("encode_events: the event arrays must all be host data or all device tensors")
    if not any(on_device):
        first, last, cls = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (first, last, cls))
        xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
        offs = np.asarray(rec_offsets, dtype=np.int64).reshape(-1)
        E = first.shape[0]
        if not (last.shape[0] == cls.shape[0] == xyz.shape[0] == E):
            raise L.SeldHipError("encode_events: first, last, cls and xyz must hold one entry per event")
        if offs.shape[0] < 2 or offs[0] != 0 or offs[-1] != E or (np.diff(offs) < 0).any():
            raise L.SeldHipError(f"encode_events: rec_offsets must ascend from 0 to the number of events ({E})")
        if ((cls < 0) | (cls >= classes)).any():
            raise L.SeldHipError(f"encode_events: class id outside [0, {classes})")
        covered = last >= first
        if (covered & ((first < 0) | (last >= frames))).any():
            raise L.SeldHipError(f"encode_events: frame index outside [0, {frames})")
        max_rec = int(np.diff(offs).max())
        if max_rec > ENCODE_MAX_EVENTS:
            raise L.SeldHipError(f"encode_events: {max_rec} events in one recording; the kernel stages {ENCODE_MAX_EVENTS}")
        dev = out.device if out is not None else _device()
        i32 = np.iinfo(np.int32)
        first, last = np.clip(first, i32.min, i32.max), np.clip(last, i32.min, i32.max)
        first, last, cls = (torch.from_numpy(a.astype(np.int32)).to(dev) for a in (first, last, cls))
        xyz, offs = torch.from_numpy(np.ascontiguousarray(xyz)).to(dev), torch.from_numpy(offs).to(dev)
    else:
        dev = first.device
        first, last, cls = (a.reshape(-1).to(torch.int32).contiguous() for a in (first, last, cls))
        xyz = xyz.to(torch.float64).reshape(-1, 3).contiguous()
        offs = rec_offsets.reshape(-1).to(torch.int64).contiguous()
        E = first.shape[0]
        if not (last.shape[0] == cls.shape[0] == xyz.shape[0] == E) or offs.shape[0] < 2:
            raise L.SeldHipError("encode_events: first, last, cls and xyz must hold one entry per event, rec_offsets two or more")
        if any(a.device != dev for a in (last, cls, xyz, offs)):
            raise L.SeldHipError("encode_events: the event arrays are on different devices")
        max_rec = min(E, ENCODE_MAX_EVENTS)     # a recording with more is counted invalid by the kernel
    R = offs.shape[0] - 1
    width = 4 * classes * (1 if no_overlaps else overlaps)
    if out is None:
        out = torch.empty((R, frames, width), device=dev, dtype=dtype)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.device != dev or out.dtype != dtype
          or tuple(out.shape) != (R, frames, width) or not out.is_contiguous()):
        raise L.SeldHipError(f"encode_events: out must be a contiguous {dtype} device tensor of shape {(R, frames, width)}")
    read_back = counters is None
    if read_back:
        counters = torch.empty(2, device=dev, dtype=torch.int32)
    elif (not torch.is_tensor(counters) or counters.device != dev or counters.dtype != torch.int32 or counters.numel() != 2
          or not counters.is_contiguous()):
        raise L.SeldHipError("encode_events: counters must be a contiguous int32 device tensor of two entries")
    code = L.SELD_DECODE_F32 if dtype == torch.float32 else L.SELD_DECODE_F64
    with torch.cuda.device(dev):
        with timed("encode_events_kernel", lambda: (0.0, float(out.numel() * out.element_size() + E * 36))):
            L.check(L.lib().seld_encode_events(L.ptr(first), L.ptr(last), L.ptr(cls), L.ptr(xyz), L.ptr(offs), E, max_rec, R,
                                               frames, classes, overlaps, float(max_loc_value), int(bool(no_overlaps)), code,
                                               L.ptr(out), L.ptr(counters), L.current_stream()), "seld_encode_events")
        if read_back:
            overflow, invalid = counters.tolist()               # the one read-back
            if invalid:
                raise L.SeldHipError(f"encode_events: {invalid} invalid events or recordings (a frame outside [0, {frames}), a "
                                     f"class outside [0, {classes}), offsets that do not ascend, or more than "
                                     f"{ENCODE_MAX_EVENTS} events in one recording)")
            if overflow:
                raise IndexError(f"encode_events: {overflow} (recording, frame, class) cells hold more than {overlaps} "
                                 "simultaneous events")
    return out


def segment(x, seg_len, hop, time_first=False, segments=None):
    """Overlapping, zero-padded segments of a device tensor, stacked (csrc/labels.hip seld_segment).

    time_first=False: x (..., length) -> (segments, ..., seg_len), out[s, ..., j] = x[..., s * hop + j];
    time_first=True:  x (length, ...) -> (segments, seg_len, ...), out[s, j] = x[s * hop + j];
    zero where s * hop + j >= length.  float32 or float64.  segments defaults to len(range(0, length, hop)), the
    reference's np.arange(0, length, hop) count."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise L.SeldHipError("segment: expected a HIP device tensor (this package has no CPU path)")
    if x.dtype not in (torch.float32, torch.float64):
        raise L.SeldHipError(f"segment: expected float32 or float64, got {x.dtype}")
    if x.dim() < 1 or x.numel() == 0:
        raise L.SeldHipError(f"segment: empty input of shape {tuple(x.shape)}")
    seg_len, hop = int(seg_len), int(hop)
    if seg_len <= 0 or hop < 1:
        raise L.SeldHipError(f"segment: seg_len must be positive and hop at least 1, got {seg_len}, {hop}")
    x = x.contiguous()
    length = x.shape[0] if time_first else x.shape[-1]
    rest = tuple(x.shape[1:]) if time_first else tuple(x.shape[:-1])
    rows = x.numel() // length
    segments = len(range(0, length, hop)) if segments is None else int(segments)
    if segments <= 0:
        raise L.SeldHipError(f"segment: segments must be positive, got {segments}")
    out = torch.empty((segments, seg_len) + rest if time_first else (segments,) + rest + (seg_len,), device=x.device,
                      dtype=x.dtype)
    code = L.SELD_DECODE_F32 if x.dtype == torch.float32 else L.SELD_DECODE_F64
    with torch.cuda.device(x.device):
        with timed("segment_kernel", lambda: (0.0, float((out.numel() + min(x.numel(), out.numel())) * x.element_size()))):
            L.check(L.lib().seld_segment(L.ptr(x), code, int(bool(time_first)), rows, length, seg_len, hop, segments, L.ptr(out),
                                         L.current_stream()), "seld_segment")
    return out
