"""Drop-in for the parts of the reference's utility_functions.py that are on the hot path: `spectrum_fast`
(utility_functions.py:129-155, called at model.py:562), the STFT magnitude / phase feature extractor, and
`gen_submission_list_task2` / `gen_submission_list_task2_OLD` (utility_functions.py:158-210, called at train.py:110-116),
which turn the network's outputs into the challenge's submission rows, and `csv_to_matrix_task2` / `segment_waveforms` /
`segment_task2` (utility_functions.py:212-342), which build the dense target from a label file and cut features, targets
and waveforms into training segments.

`stft_complex` and `seld_features` go beyond the reference: the complex spectra themselves, and the log-(mel-)power /
FOA intensity-vector features of them (csrc/spatial_features.hip through hip_ops.spatial_features).

Same names, same arguments, same result layout.  The transform runs on the GPU (csrc/stft.hip, csrc/stft_any.hip through
seld_stft_magphase_ws) for every segment length 2 <= nperseg <= 4096, the decoding through csrc/decode.hip
(hip_ops.decode_events), the target encoding and the segmentation through csrc/labels.hip (hip_ops.encode_events,
hip_ops.segment); there is no CPU path -- a missing device or library raises.
"""

import numpy as np
import torch

from . import _lib as L
from . import hip_ops as H


MAX_NPERSEG = 4096        # longest segment the device transforms (one workgroup's LDS)


def stft_workspace(nperseg, device):
    """The device workspace seld_stft_magphase_ws needs for this segment length (None when it needs none)."""
    nbytes = L.lib().seld_stft_workspace(int(nperseg))
    return torch.empty(nbytes, device=device, dtype=torch.uint8) if nbytes else None


def _window_values(window, nperseg, device):
    """Window divided by its sum (scipy.signal.stft's scaling='spectrum'), or None for the kernel's built-in periodic
    Hamming.  Other windows need scipy.signal.get_window (host side, a constant table of nperseg values)."""
    if isinstance(window, str) and window == 'hamming':
        return None
    if isinstance(window, (str, tuple)):
        from scipy.signal import get_window
        w = get_window(window, nperseg)
    else:
        w = np.asarray(window, dtype=np.float64)
        if w.shape != (nperseg,):
            raise ValueError('window must have length of nperseg')
    return torch.from_numpy((w / w.sum()).astype(np.float32)).to(device)


def spectrum_fast(x, nperseg=512, noverlap=128, window='hamming', cut_dc=True, output_phase=True,
                  cut_last_timeframe=True):
    '''
    Compute magnitude (and phase) spectra of a multichannel signal -- utility_functions.py:129-155:
    scipy.signal.stft(x, window, nperseg, noverlap) -> |Z| [-> concatenated with angle(Z) on the channel axis]
    [-> DC bin dropped] [-> last frame dropped].

    x: (channels, samples).  A numpy array gives a numpy array of the reference's dtype -- float32 for float32 input
    (scipy's stft returns complex64 then), float64 for anything else; the transform itself is computed in float32 on
    the device -- and a torch tensor gives a float32 tensor on the GPU.
    Returns (channels or 2*channels, nperseg/2 + 1 - cut_dc, frames - cut_last_timeframe).

    Batched input (..., channels, samples) follows the reference literally: the transform runs over the last axis, phase
    is concatenated on axis -3, and the two cuts are the reference's `output[:, 1:, :]` / `output[:, :, :-1]` -- which on
    a batched array act on axes 1 and 2 (channels and frequency), not on the DC bin and the last frame.
    '''
    is_numpy = not torch.is_tensor(x)
    if is_numpy:
        x = np.asarray(x)
        out_dtype = np.float32 if x.dtype == np.float32 else np.float64
    if (x.ndim if is_numpy else x.dim()) > 2:
        lead, C = tuple(x.shape[:-2]), x.shape[-2]
        flat = x.reshape((-1, x.shape[-1]))
        if is_numpy:
            flat = torch.as_tensor(np.ascontiguousarray(flat, dtype=np.float32))
        rows = flat.shape[0]
        both = spectrum_fast(flat, nperseg, noverlap, window, False, output_phase, False)   # [|Z| rows ; angle rows]
        output = both[:rows].reshape(lead + (C,) + tuple(both.shape[1:]))
        if output_phase:
            output = torch.cat((output, both[rows:].reshape(output.shape)), dim=-3)
        if cut_dc:
            output = output[:, 1:, :]
        if cut_last_timeframe:
            output = output[:, :, :-1]
        return output.cpu().numpy().astype(out_dtype) if is_numpy else output
    t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)) if is_numpy else x
    if t.dim() != 2:
        raise ValueError(f"spectrum_fast expects (channels, samples), got shape {tuple(t.shape)}")
    out = _stft_planes("spectrum_fast", t, nperseg, noverlap, window, cut_dc, cut_last_timeframe, int(bool(output_phase)))
    if is_numpy:
        return out.cpu().numpy().astype(out_dtype)
    return out


def _launch_device(what, t):
    if not torch.cuda.is_available():
        raise L.SeldHipError(f"{what}: no HIP device (this package has no CPU path)")
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _stft_planes(what, t, nperseg, noverlap, window, cut_dc, cut_last_timeframe, form):
    """What every transform here shares: the argument checks, the window table, the workspace and the launch.
    t (rows, samples), a tensor on the host or the device; form 0: |Z|, 1: |Z| then angle(Z) (seld_stft_magphase_ws),
    'complex': Re Z then Im Z (seld_stft_complex_ws).  Returns the float32 device tensor (rows or 2 rows, bins, frames)."""
    dev = _launch_device(what, t)
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    C, n = t.shape
    nperseg, noverlap = int(nperseg), int(noverlap)
    if noverlap >= nperseg:
        raise ValueError('noverlap must be less than nperseg.')          # scipy's message
    if nperseg > MAX_NPERSEG:
        raise L.SeldHipError(f"{what}: nperseg={nperseg} is longer than the longest segment the HIP STFT "
                             f"transforms ({MAX_NPERSEG})")
    lib = L.lib()
    frames = lib.seld_stft_frames_ex(n, nperseg, noverlap, int(bool(cut_last_timeframe)))
    if frames <= 0:
        raise L.SeldHipError(f"{what}: invalid segment parameters")
    bins = nperseg // 2 + 1 - int(bool(cut_dc))
    win = _window_values(window, nperseg, dev)
    out = torch.empty(((1 if form == 0 else 2) * C, bins, frames), device=dev, dtype=torch.float32)
    ws = stft_workspace(nperseg, dev)
    tail = (int(bool(cut_dc)), int(bool(cut_last_timeframe)), L.ptr(win), L.ptr(out), L.ptr(ws),
            0 if ws is None else ws.numel(), L.current_stream())
    with torch.cuda.device(dev):
        if form == 'complex':
            L.check(lib.seld_stft_complex_ws(L.ptr(t), C, n, nperseg, noverlap, *tail), "seld_stft_complex_ws")
        else:
            L.check(lib.seld_stft_magphase_ws(L.ptr(t), C, n, nperseg, noverlap, int(form), *tail), "seld_stft_magphase_ws")
    return out


def _rows(what, x):
    """x (..., channels, samples), a numpy array or a tensor -> (float32 tensor (rows, samples) with the leading axes
    flattened onto the channel axis, the shape of those axes channels included, whether x was numpy)."""
    is_numpy = not torch.is_tensor(x)
    if is_numpy:
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
    if x.dim() < 2 or x.is_complex():
        raise ValueError(f"{what} expects real (..., channels, samples), got shape {tuple(x.shape)}")
    return x.reshape((-1, x.shape[-1])), tuple(x.shape[:-1]), is_numpy


def stft_complex(x, nperseg=512, noverlap=128, window='hamming', cut_dc=True, cut_last_timeframe=True):
    '''
    The complex spectra spectrum_fast takes the modulus and angle of: scipy.signal.stft(x, window, nperseg, noverlap)
    [-> DC bin dropped] [-> last frame dropped], the window divided by its sum, for every 2 <= nperseg <= 4096.

    x: (..., channels, samples), numpy array or tensor; leading axes are batch (flattened onto the channel axis for the
    launch; unlike spectrum_fast's literal batched form, the two cuts always act on the bin and frame axes).  Returns a
    complex64 tensor (..., channels, nperseg/2 + 1 - cut_dc, frames - cut_last_timeframe) on the device.  The kernels
    write planes of real and imaginary parts; they are interleaved once here.
    '''
    rows, lead, _ = _rows("stft_complex", x)
    planes = _stft_planes("stft_complex", rows, nperseg, noverlap, window, cut_dc, cut_last_timeframe, 'complex')
    R = rows.shape[0]
    return torch.complex(planes[:R], planes[R:]).view(lead + tuple(planes.shape[1:]))


def seld_features(x, kind='logpower_iv', layout='grouped', nperseg=512, noverlap=128, window='hamming', n_mels=0,
                  sr=32000, fmin=0.0, fmax=None, cut_dc=True, cut_last_timeframe=True, eps=1e-10):
    '''
    Log-(mel-)power and first-order-Ambisonics intensity-vector features of a multichannel recording, in two launches:
    the STFT in its complex form (stft_complex's transform) and hip_ops.spatial_features' kernel on its planes.

    x: (..., channels, samples); every four channels are one FOA microphone [W, D1, D2, D3].  kind, layout, eps:
    hip_ops.spatial_features.  n_mels=0 keeps linear frequency; otherwise the bins are projected onto
    hip_ops.mel_filterbank(sr, nperseg, n_mels, fmin, fmax) (Slaney scale and normalisation; its DC column dropped with
    cut_dc).  Returns (..., C_out, n_mels or bins, frames): a float32 numpy array for numpy input, a float32 device
    tensor for a tensor.  layout='quaternion' turns the eight channels of two FOA microphones into eight feature
    channels [log-power of W, I1, I2, I3] x 2: one dual quaternion, the input of domain='DQ'.
    '''
    what = "seld_features"
    rows, lead, is_numpy = _rows(what, x)
    k, l = H._feature_form(what, kind, layout, lead[-1], eps)
    n_mels = int(n_mels)
    if n_mels < 0:
        raise ValueError(f"{what}: n_mels must be 0 (linear frequency) or positive, got {n_mels}")
    dev = _launch_device(what, rows)
    tables = None
    if n_mels:
        tables = H._mel_tables(float(sr), int(nperseg), n_mels, float(fmin), None if fmax is None else float(fmax),
                               bool(cut_dc), dev)
    planes = _stft_planes(what, rows, nperseg, noverlap, window, cut_dc, cut_last_timeframe, 'complex')
    out = H._features_of_planes(what, planes, lead[:-1], lead[-1], k, l, tables, eps)
    return out.cpu().numpy() if is_numpy else out


def _decode_one(sed, doa, max_loc_value, num_classes, max_overlaps):
    """(rows, event) of one recording as numpy arrays, one read-back each.

    The reference rounds `sed` in sed's dtype and multiplies `doa` in doa's, so doa decides the arithmetic: float32 stays
    float32 (one float32 multiply, widened), every other real dtype is computed in float64.  `sed` is brought to that
    dtype where the conversion cannot move a rounding: float32 or integer sed with float64 doa, integer / bool sed with
    float32 doa (exact below 2^24).  float64 sed with float32 doa is refused, since narrowing can carry a value across
    a tie; float16 is refused as well."""
    def as_array(a, name):
        if torch.is_tensor(a):
            return a
        a = np.asarray(a)
        if a.dtype.kind not in "fiub" or a.dtype == np.float16:
            raise L.SeldHipError(f"gen_submission_list_task2: {name}: unsupported dtype {a.dtype}")
        return a
    sed, doa = as_array(sed, "sed"), as_array(doa, "doa")
    if torch.is_tensor(sed) != torch.is_tensor(doa):
        raise L.SeldHipError("gen_submission_list_task2: sed and doa must both be numpy arrays or both device tensors")
    if not torch.is_tensor(sed):
        if doa.dtype != np.float32:
            doa = doa.astype(np.float64)
        if sed.dtype != doa.dtype:
            if sed.dtype == np.float64:
                raise L.SeldHipError("gen_submission_list_task2: float64 sed with float32 doa is not supported "
                                     "(narrowing sed can move a value across a rounding tie); pass doa as float64")
            sed = sed.astype(doa.dtype)
        if not torch.cuda.is_available():
            raise L.SeldHipError("gen_submission_list_task2: no HIP device (this package has no CPU path)")
        dev = torch.device("cuda", torch.cuda.current_device())
        sed = torch.from_numpy(np.ascontiguousarray(sed)).to(dev)
        doa = torch.from_numpy(np.ascontiguousarray(doa)).to(dev)
    elif sed.dtype == torch.float32 and doa.dtype == torch.float64:
        sed = sed.double()
    if sed.dim() != 2:
        raise L.SeldHipError(f"gen_submission_list_task2: expected one recording (T, n), got shape {tuple(sed.shape)}")
    rows, event, _ = H.decode_events(sed, doa, max_loc_value, num_classes, max_overlaps)
    return rows.cpu().numpy(), event.cpu().numpy()


def gen_submission_list_task2_OLD(sed, doa, max_loc_value=2., num_frames=600, num_classes=14, max_overlaps=3):
    '''
    Process sed and doa output matrices (model's output) and generate the list of active sounds and their location for
    every frame, in the format of the Challenge results submission -- utility_functions.py:158-181.

    sed (T, num_classes * max_overlaps), doa (T, 3 * num_classes * max_overlaps): numpy arrays or device tensors.
    doa's dtype decides the arithmetic as in the reference (float32, else float64); sed may differ from it except
    float64 sed with float32 doa, which is refused.
    Returns the float64 array of [time_frame, sound_class, x, y, z] rows, frame-major and in slot order; without any
    active slot the reference's `np.array([])`, shape (0,).  `num_frames` is accepted and ignored, as in the reference.
    '''
    rows, _ = _decode_one(sed, doa, max_loc_value, num_classes, max_overlaps)
    return rows if rows.shape[0] else np.array([])


def gen_submission_list_task2(sed, doa, max_loc_value=2., num_frames=600, num_classes=14, max_overlaps=3):
    '''
    utility_functions.py:184-210: the rows of gen_submission_list_task2_OLD and the dictionary
    {time_frame: [[sound_class, x, y, z, num_event], ...]} the DCASE21 metrics read, with Python int / float entries
    and the frames in order of first appearance.  The dictionary is host work by nature; it is built from one
    read-back of the rows and the event indices.
    '''
    rows, event = _decode_one(sed, doa, max_loc_value, num_classes, max_overlaps)
    output_dict = {}
    cols = [rows[:, k].tolist() for k in range(5)]
    for f, c, x, y, z, e in zip(cols[0], cols[1], cols[2], cols[3], cols[4], event.tolist()):
        output_dict.setdefault(int(f), []).append([int(c), x, y, z, e])
    return (rows if rows.shape[0] else np.array([])), output_dict


def csv_to_matrix_task2(path, class_dict, dur=60, step=0.1, max_loc_value=2., no_overlaps=False):
    '''
    Read a task-2 label csv file and output the matrix of 100-msec frames, each filled with the activity of every
    sound class present and its location coordinates -- utility_functions.py:212-269.

    The file is read with pandas.read_csv as in the reference (its float parser is part of the result), the columns
    Start / End are turned into frames on the host (hip_ops.event_frames) and the matrix is filled on the device
    (hip_ops.encode_events, csrc/labels.hip).  Returns the (int(dur / step), 4 * len(class_dict) * 3) float64 numpy
    array [cl | loc] -- (.., 4 * len(class_dict)) with no_overlaps -- and raises IndexError where more than three
    sounds of one class overlap, as the reference does.
    '''
    try:
        import pandas as pd
    except ImportError as e:
        raise ImportError("csv_to_matrix_task2 reads the label file with pandas.read_csv, as the reference does: "
                          "install pandas") from e
    max_overlap = 3
    num_frames = int(dur / step)
    df = pd.read_csv(path)
    first, last = H.event_frames(df['Start'].to_numpy(dtype=np.float64), df['End'].to_numpy(dtype=np.float64), dur, step)
    cls = np.asarray([class_dict[c] for c in df['Class']], dtype=np.int64)
    xyz = df[['X', 'Y', 'Z']].to_numpy(dtype=np.float64)
    out = H.encode_events(first, last, cls, xyz, [0, len(df)], num_frames, len(class_dict), max_overlap, max_loc_value,
                          no_overlaps, torch.float64)
    return out[0].cpu().numpy()


def _segment_inputs(name, predictors, target):
    """(predictors, target, is_numpy) as contiguous device tensors: numpy arrays go to the current device, device tensors
    stay where they are.  float32 and float64 only."""
    if torch.is_tensor(predictors) != torch.is_tensor(target):
        raise L.SeldHipError(f"{name}: predictors and target must both be numpy arrays or both device tensors")
    is_numpy = not torch.is_tensor(predictors)
    if is_numpy:
        predictors, target = np.asarray(predictors), np.asarray(target)
        for a, what in ((predictors, "predictors"), (target, "target")):
            if a.dtype not in (np.float32, np.float64):
                raise L.SeldHipError(f"{name}: {what}: unsupported dtype {a.dtype} (float32 or float64)")
        if not torch.cuda.is_available():
            raise L.SeldHipError(f"{name}: no HIP device (this package has no CPU path)")
        dev = torch.device("cuda", torch.cuda.current_device())
        predictors = torch.from_numpy(np.ascontiguousarray(predictors)).to(dev)
        target = torch.from_numpy(np.ascontiguousarray(target)).to(dev)
    return predictors, target, is_numpy


def _segment_lists(X, Y, is_numpy):
    if is_numpy:
        X, Y = X.cpu().numpy(), Y.cpu().numpy()
        return [X[i] for i in range(X.shape[0])], [Y[i] for i in range(Y.shape[0])]
    return list(X.unbind(0)), list(Y.unbind(0))


def segment_waveforms(predictors, target, length):
    '''
    Segment input waveforms into shorter frames of predefined length (in samples), the last one zero-padded --
    utility_functions.py:272-299.  predictors (channels, samples), target (channels', samples).

    numpy arrays in give lists of numpy arrays, through the device; device tensors in give lists of views into the two
    stacked device results (hip_ops.segment, csrc/labels.hip), without a host copy.  Every chunk has the input's dtype
    (the reference returns its padded last chunk in float64; the values are equal).  A target shorter than the
    predictors, for which the reference returns ragged chunks, raises ValueError.
    '''
    predictors, target, is_numpy = _segment_inputs("segment_waveforms", predictors, target)
    if predictors.dim() != 2 or target.dim() != 2:
        raise ValueError(f"segment_waveforms: expected (channels, samples) arrays, got {tuple(predictors.shape)} and "
                         f"{tuple(target.shape)}")
    length, n = int(length), predictors.shape[-1]
    if length < 1:
        raise ValueError(f"segment_waveforms: length must be positive, got {length}")
    if target.shape[-1] < n:
        raise ValueError(f"segment_waveforms: the target ({target.shape[-1]} samples) is shorter than the predictors ({n})")
    count = len(range(0, n, length))
    X = H.segment(predictors, length, length, segments=count)
    Y = H.segment(target[:, :n], length, length, segments=count)
    return _segment_lists(X, Y, is_numpy)


def segment_task2(predictors, target, predictors_len_segment=50*8, target_len_segment=50, overlap=0.5):
    '''
    Segment input stft and target matrix of task 2 into shorter, overlapping chunks, the last ones zero-padded; the
    default parameters cut 5-second frames -- utility_functions.py:302-342.  predictors (channels, bins, frames),
    target (frames', width).

    The reference's target path is kept bit for bit, quirk included: it RESHAPES the (frames', width) target to
    (1, width, frames') -- a reinterpretation of the buffer, not a transpose --, cuts the last axis and reshapes each
    cut to (target_len_segment, width).  hip_ops.segment(target, ..., time_first=True) gives the cut by rows.
    Input convention, dtype and list results as segment_waveforms.  Raises the reference's ValueError when the two
    cut counts differ, and ValueError for a chunk that lies inside the predictors but extends past the target (where
    the reference returns a short chunk) or is padded in the predictors but longer than a segment in the target
    (where the reference's pad fails).
    '''
    predictors, target, is_numpy = _segment_inputs("segment_task2", predictors, target)
    if predictors.dim() != 3 or target.dim() != 2:
        raise ValueError(f"segment_task2: expected (channels, bins, frames) predictors and a (frames, width) target, got "
                         f"{tuple(predictors.shape)} and {tuple(target.shape)}")
    len_p, len_t = int(predictors_len_segment), int(target_len_segment)
    hop_p, hop_t = int(len_p * overlap), int(len_t * overlap)
    if len_p < 1 or len_t < 1 or hop_p < 1 or hop_t < 1:
        raise ValueError(f"segment_task2: segment lengths {len_p}, {len_t} with overlap {overlap} give no positive hop")
    frames_p, (frames_t, width) = predictors.shape[-1], target.shape
    count = len(range(0, frames_p, hop_p))
    if count != len(range(0, frames_t, hop_t)):
        raise ValueError('Predictors and test frames should be selected to produce the same amount of frames')
    starts = np.arange(count, dtype=np.int64)
    padded = starts * hop_p + len_p > frames_p
    left = frames_t - starts * hop_t
    if (np.where(padded, left > len_t, left < len_t)).any():
        raise ValueError('segment_task2: the target chunks do not follow the predictor chunks: a chunk inside the '
                         'predictors extends past the target, or a padded one is longer than target_len_segment')
    X = H.segment(predictors, len_p, hop_p, segments=count)
    # target.reshape(1, width, frames'): the same buffer read as `width` rows of frames' entries
    Y = H.segment(target.contiguous().view(width, frames_t), len_t, hop_t, segments=count).view(count, len_t, width)
    return _segment_lists(X, Y, is_numpy)
