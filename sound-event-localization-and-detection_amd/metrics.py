"""Drop-in for the task-2 part of the reference's metrics.py: same names, signatures and return types, the counting done by
hip_ops.score_events (csrc/event_metrics.hip) on the device.  The task-1 speech functions are out of scope.

`pred` and `true` are numpy arrays of any real dtype, (E, 5) device tensors, or, with from_csv=True, paths of header-less
CSV files whose class column is numeric or holds class names; rows are [frame, class, x, y, z].  An empty list is
np.array([]) of shape (0,), as gen_submission_list_task2 returns it."""
import csv
import os
import sys

import numpy as np
import torch

from . import _lib as L
from . import hip_ops as H

sound_classes_dict_task2 = {'Chink_and_clink': 0,
                            'Computer_keyboard': 1,
                            'Cupboard_open_or_close': 2,
                            'Drawer_open_or_close': 3,
                            'Female_speech_and_woman_speaking': 4,
                            'Finger_snapping': 5,
                            'Keys_jangling': 6,
                            'Knock': 7,
                            'Laughter': 8,
                            'Male_speech_and_man_speaking': 9,
                            'Printer': 10,
                            'Scissors': 11,
                            'Telephone': 12,
                            'Writing': 13}


def _device():
    if not torch.cuda.is_available():
        raise L.SeldHipError("metrics: no HIP device (this package has no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def _read_csv(path, names):
    """(E, 5) float64 of a header-less CSV.  A class that is no number is a name: `names` (shared by the files of one
    call) gives it an id, the task's own for the 14 known names and a fresh negative one otherwise, so that two rows
    have equal ids exactly where the reference finds equal strings."""
    rows = []
    with open(path, newline="") as f:
        for rec in csv.reader(f):
            if not rec:
                continue
            vals = []
            for k, cell in enumerate(rec):
                cell = cell.strip()
                try:
                    vals.append(float(cell))
                except ValueError:
                    if k != 1:
                        raise
                    vals.append(float(names.setdefault(cell, -len(names))))
            rows.append(vals)
    return np.asarray(rows, dtype=np.float64).reshape(-1, 5)


def _lists(lists, dev):
    """One side's recordings -> (rows (E, 5) float64 on the device, offsets (R + 1,) int64 on the device, a device scalar
    that counts the recordings whose rows do not ascend by frame).  Nothing is read back here."""
    parts = []
    for x in lists:
        if not torch.is_tensor(x):
            x = np.asarray(x)
            x = torch.from_numpy(np.ascontiguousarray(x.astype(np.float64))) if x.size else torch.zeros((0, 5), dtype=torch.float64)
        parts.append(x.to(device=dev, dtype=torch.float64).reshape(-1, 5))
    rows = torch.cat(parts) if len(parts) != 1 else parts[0].contiguous()
    counts = [p.shape[0] for p in parts]
    offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(counts, dtype=np.int64))).astype(np.int64)).to(dev)
    unsorted = torch.zeros((), device=dev, dtype=torch.int64)
    for p in parts:
        if p.shape[0] > 1:
            unsorted = unsorted + (p[1:, 0] < p[:-1, 0]).any()
    return rows, offsets, unsorted


def _score(pred_lists, true_lists, n_frames, spatial_threshold):
    """The six detection counters [TP, FP, FN | class-only TP, FP, FN] of a batch of recordings in ONE device call with
    ONE read-back (counters, flags and whether a list was out of order, together).  Only where a list does not ascend by
    frame, which decode_events rows and the challenge's files do, it is ordered by hip_ops.sort_events and scored again."""
    n_frames = int(n_frames)
    on_device = [t for t in list(pred_lists) + list(true_lists) if torch.is_tensor(t) and t.is_cuda]
    dev = on_device[0].device if on_device else _device()
    pr, po, pu = _lists(pred_lists, dev)
    tr, to, tu = _lists(true_lists, dev)
    n = len(H.EVENT_METRIC_COUNTERS)
    while True:
        buf = torch.zeros(n + 4, device=dev, dtype=torch.int64)
        acc = (buf[:n], torch.zeros(1, device=dev, dtype=torch.float64))
        # nb_classes = 0: detection only, which has no limit on the events of a frame
        H.score_events(acc, pr, po, tr, to, n_frames, nb_classes=0, spatial_threshold=spatial_threshold, flags=buf[n:n + 2])
        buf[n + 2] = pu
        buf[n + 3] = tu
        out = buf.tolist()                              # the one read-back
        if not (out[n + 2] or out[n + 3]):
            break
        if out[n + 2]:
            pr, pu = H.sort_events(pr, po), torch.zeros_like(pu)
        if out[n + 3]:
            tr, tu = H.sort_events(tr, to), torch.zeros_like(tu)
    if out[n]:
        raise KeyError(f"{out[n]} rows with a frame outside range({n_frames})")
    return out[0:3], out[13:16]


def _inputs(pred, true, from_csv):
    if from_csv:
        names = dict(sound_classes_dict_task2)
        return _read_csv(pred, names), _read_csv(true, names)
    return pred, true


def _f_score(TP, FP, FN):
    precision = TP / (TP + FP + sys.float_info.epsilon)
    recall = TP / (TP + FN + sys.float_info.epsilon)
    return precision, recall, 2 * ((precision * recall) / (precision + recall + sys.float_info.epsilon))


def location_sensitive_detection(pred, true, n_frames=100, spatial_threshold=2.,
                                 from_csv=False, verbose=False):
    '''
    Compute TP, FP, FN of a single data point using
    location sensitive detection
    '''
    pred, true = _inputs(pred, true, from_csv)
    (TP, FP, FN), _ = _score([pred], [true], n_frames, spatial_threshold)
    precision, recall, F_score = _f_score(TP, FP, FN)
    if verbose:
        print('true positives: ', TP)
        print('false positives: ', FP)
        print('false negatives: ', FN)
        print('---------------------')
        print('*******************************')
        print('F score: ', F_score)
        print('Precision: ', precision)
        print('Recall: ', recall)
        print('TP: ', TP)
        print('FP: ', FP)
        print('FN: ', FN)
    return TP, FP, FN, F_score


def sed_score_computation(pred, true, n_frames=100, spatial_threshold=2.,
                          from_csv=False, verbose=False):
    '''
    Compute TP, FP, FN of a single data point matching on the class alone, and the SED score
    '''
    pred, true = _inputs(pred, true, from_csv)
    _, (TP, FP, FN) = _score([pred], [true], n_frames, spatial_threshold)
    precision, recall, F_score = _f_score(TP, FP, FN)
    Nref = TP + FN
    Nsys = TP + FP
    ER_score = (max(Nref, Nsys) - TP) / (Nref + 0.0)       # ZeroDivisionError without a reference event, as the reference
    sed_score = np.mean([1 - F_score, ER_score])
    if verbose:
        print('SED score: ', sed_score)
    return TP, FP, FN, sed_score


def compute_seld_metrics(predicted_folder, truth_folder, n_frames=100, spatial_threshold=0.3):
    '''
    compute F1 score from results folder of submitted results based on the
    location sensitive detection metric

    The reference's body cannot run (it unpacks four return values into three and reads the paths as arrays); this is
    its evident intent: the counters of every predicted .csv against the truth file of the same name, summed.  All
    files are scored in one device call.
    '''
    predicted_list = [s for s in os.listdir(predicted_folder) if '.csv' in s]
    names = dict(sound_classes_dict_task2)
    pred = [_read_csv(os.path.join(predicted_folder, s), names) for s in predicted_list]
    true = [_read_csv(os.path.join(truth_folder, s), names) for s in predicted_list]
    TP = FP = FN = 0
    if predicted_list:
        (TP, FP, FN), _ = _score(pred, true, n_frames, spatial_threshold)

    precision = TP / (TP + FP + sys.float_info.epsilon)
    recall = TP / (TP + FN + sys.float_info.epsilon)

    print('*******************************')
    F_score = (2 * precision * recall) / (precision + recall + sys.float_info.epsilon)
    print('F score: ', F_score)
    print('Precision: ', precision)
    print('Recall: ', recall)

    return F_score
