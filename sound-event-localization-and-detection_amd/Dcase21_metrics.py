"""Drop-in for the reference's Dcase21_metrics.py: same names, signatures and return types.  SELDMetrics counts on the
device (hip_ops.score_events, csrc/event_metrics.hip) and least_distance_between_gt_pred associates there
(hip_ops.assign_doas); segment_labels, the distance functions and early_stopping_metric are host functions on Python and
numpy values, as in the reference.

Limits of the device path: events are Cartesian (x, y, z) or spherical (azimuth, elevation in degrees), one form per
call; at most `max_tracks` events of one class in one frame (3 unless SELDMetrics is given more, 8 at most); at most 64
classes; least_distance_between_gt_pred takes at most 8 DOAs a side.  Where several associations of a frame cost the
same, the first row -> column map in lexicographic order is taken (scipy's choice among equals is its own)."""
import functools

import numpy as np
import torch

from . import _lib as L
from . import class_metrics as CM
from . import hip_ops as H

eps = np.finfo(float).eps


def _takes_average(init):
    """SELDMetrics(..., average='micro' | 'macro'): a keyword of this package beside the reference's constructor, whose own
    parameter list (what inspect.signature reports) stays the reference's plus max_tracks."""
    @functools.wraps(init)
    def __init__(self, *args, average="micro", **kwargs):
        if average not in ("micro", "macro"):
            raise L.SeldHipError(f"SELDMetrics: average must be 'micro' or 'macro', got {average!r}")
        init(self, *args, **kwargs)
        self._average = average
        self._tables = []                               # 'macro': the (counters, total_de) tables of update_from_events
    return __init__


class SELDMetrics(object):
    @_takes_average
    def __init__(self, doa_threshold=20, nb_classes=14, max_tracks=3):
        '''
            This class implements both the class-sensitive localization and location-sensitive detection metrics.

        :param nb_classes: Number of sound classes.
        :param doa_thresh: DOA threshold for location sensitive detection.
        :param max_tracks: events of one class in one frame the device association takes (1 .. 8).
        '''
        self._nb_classes = nb_classes
        self._max_tracks = max_tracks

        # Variables for Location-senstive detection performance
        self._TP = 0
        self._FP = 0
        self._FN = 0

        self._S = 0
        self._D = 0
        self._I = 0
        self._Nref = 0

        self._spatial_T = doa_threshold

        # Variables for Class-sensitive localization performance
        self._total_DE = 0

        self._DE_TP = 0
        self._DE_FP = 0
        self._DE_FN = 0

    def compute_seld_scores(self):
        '''
        Collect the final SELD scores

        :return: returns both location-sensitive detection scores and class-sensitive localization scores
        (average='macro': their class-wise macro averages over the classes of the reference, class_metrics.macro_scores)
        '''
        if self._average == "macro":
            m = CM.macro_scores(*self.table())
            return m["ER"], m["F"], m["LE"], m["LR"]
        # Location-sensitive detection performance
        ER = (self._S + self._D + self._I) / float(self._Nref + eps)
        F = self._TP / (eps + self._TP + 0.5 * (self._FP + self._FN))

        # Class-sensitive localization performance
        LE = self._total_DE / float(self._DE_TP + eps) if self._DE_TP else 180     # When the total number of prediction is zero
        LR = self._DE_TP / (eps + self._DE_TP + self._DE_FN)
        return ER, F, LE, LR

    def _add(self, acc):
        """One read-back of the device accumulators, added to the attributes."""
        c = acc[0].tolist()
        for name, k in (("_TP", 3), ("_FP", 4), ("_FN", 5), ("_S", 6), ("_D", 7), ("_I", 8), ("_Nref", 9), ("_DE_TP", 10),
                        ("_DE_FP", 11), ("_DE_FN", 12)):
            setattr(self, name, getattr(self, name) + c[k])
        self._total_DE += float(acc[1].item())

    def table(self):
        """average='macro': the breakdown of everything scored so far, (counters (R, C + 2, 16), total_de (R, C + 2)) numpy
        arrays, one slab per recording in the order they were given."""
        if self._average != "macro":
            raise L.SeldHipError("SELDMetrics: the per-class table is kept under average='macro' only")
        if not self._tables:
            return np.zeros((0, self._nb_classes + 2, 16), dtype=np.int64), np.zeros((0, self._nb_classes + 2))
        return np.concatenate([t[0] for t in self._tables]), np.concatenate([t[1] for t in self._tables])

    def class_scores(self):
        """average='macro': class_metrics.class_scores of everything scored so far."""
        return CM.class_scores(*self.table())

    def jackknife(self, score=CM.macro_score_vector):
        """average='macro': class_metrics.jackknife over the recordings scored so far (at least two)."""
        return CM.jackknife(*self.table(), score)

    def update_from_events(self, pred_rows, pred_offsets, true_rows, true_offsets, max_frames, frames_per_block=10):
        '''
        The fast form of segment_labels + update_seld_scores for callers who hold rows: (E, 5) float64 device tensors
        [frame, class, x, y, z] with (R + 1,) int64 offsets, as hip_ops.decode_events returns them, every recording of
        `max_frames` frames.  No dictionary is built.  Rows of 4 columns are [frame, class, azimuth, elevation] in degrees.
        '''
        widths = {t.shape[1] for t in (pred_rows, true_rows) if torch.is_tensor(t) and t.dim() == 2 and t.numel()}
        if len(widths) > 1:
            raise L.SeldHipError(f"update_from_events: rows of {sorted(widths)} columns in one call")
        coords = 2 if widths == {4} else 3              # any other width is score_events' to refuse
        on_device = torch.is_tensor(pred_rows) and pred_rows.is_cuda      # otherwise score_events' own checks raise
        if self._average == "macro":
            counters, total_de = H.score_events_by(pred_rows, pred_offsets, true_rows, true_offsets, max_frames,
                                                   nb_classes=self._nb_classes, doa_threshold=self._spatial_T,
                                                   frames_per_block=frames_per_block, coords=coords,
                                                   max_tracks=self._max_tracks)
            counters, total_de = counters.cpu().numpy(), total_de.cpu().numpy()      # one read-back
            self._tables.append((counters, total_de))
            self._add((counters[:, -1].sum(0), total_de[:, -1].sum()))               # the attributes stay the micro totals
            return
        acc = H.event_metrics_new(pred_rows.device if on_device else torch.device("cuda", torch.cuda.current_device()))
        H.score_events(acc, pred_rows, pred_offsets, true_rows, true_offsets, max_frames, nb_classes=self._nb_classes,
                       doa_threshold=self._spatial_T, frames_per_block=frames_per_block, coords=coords,
                       max_tracks=self._max_tracks)
        self._add(acc)

    def update_seld_scores(self, pred, gt):
        '''
        Implements the spatial error averaging according to equation 5 in the paper [1] (see papers in the title of the code).
        Adds the multitrack extensions proposed in paper [2]

        :param pred: dictionary containing class-wise prediction results for each N-seconds segment block
        :param gt: dictionary containing class-wise groundtruth for each N-seconds segment block
        (what segment_labels returns; all events Cartesian, or all azimuth and elevation in degrees)
        '''
        if self._average == "macro":
            raise L.SeldHipError("update_seld_scores: the dictionary form keeps no per-recording table; under "
                                 "average='macro' score rows with update_from_events")
        nb_blocks = len(gt.keys())
        for block_cnt in range(nb_blocks):
            gt[block_cnt], pred[block_cnt]              # the reference's KeyError for a missing block
        # A frame key only matters by identity inside its block: block * K + key with K above the largest key keeps that.
        keys = [k for d in (pred, gt) for b in range(nb_blocks) for c in d[b] for k in d[b][c][0][0]]
        if any(int(k) != k or k < 0 for k in keys):
            raise L.SeldHipError("update_seld_scores: frame keys must be non-negative integers")
        K = int(max(keys)) + 1 if keys else 1
        if not torch.cuda.is_available():
            raise L.SeldHipError("update_seld_scores: no HIP device (this package has no CPU path)")
        dev = torch.device("cuda", torch.cuda.current_device())
        sides = []
        coords = None                                   # of the first event seen; every other must agree
        for d in (pred, gt):
            rows = []
            for b in range(nb_blocks):
                for c in range(self._nb_classes):
                    if c not in d[b]:
                        continue
                    frame_keys, frame_vals = d[b][c][0]
                    for k, vals in zip(frame_keys, frame_vals):
                        for v in vals:
                            doa = list(v)[:-1]          # the reference's [:, :-1]: everything but the last entry
                            if len(doa) not in (2, 3):
                                raise L.SeldHipError(f"update_seld_scores: {len(doa)} coordinates per event; the device path "
                                                     "takes Cartesian x, y, z or azimuth, elevation in degrees")
                            coords = len(doa) if coords is None else coords
                            if len(doa) != coords:
                                raise L.SeldHipError("update_seld_scores: events of two and of three coordinates in one call")
                            rows.append([b * K + k, c] + doa)
            sides.append(rows)
        coords = 3 if coords is None else coords
        for i, rows in enumerate(sides):
            a = np.asarray(rows, dtype=np.float64).reshape(-1, 2 + coords)
            a = a[np.argsort(a[:, 0], kind="stable")]
            sides[i] = (torch.from_numpy(np.ascontiguousarray(a)).to(dev),
                        torch.tensor([0, a.shape[0]], dtype=torch.int64).to(dev))
        acc = H.event_metrics_new(dev)
        H.score_events(acc, sides[0][0], sides[0][1], sides[1][0], sides[1][1], nb_blocks * K, nb_classes=self._nb_classes,
                       doa_threshold=self._spatial_T, frames_per_block=K, coords=coords, max_tracks=self._max_tracks)
        self._add(acc)
        return


def distance_between_spherical_coordinates_rad(az1, ele1, az2, ele2):
    """
    Angular distance between two spherical coordinates
    MORE: https://en.wikipedia.org/wiki/Great-circle_distance

    :return: angular distance in degrees
    """
    dist = np.sin(ele1) * np.sin(ele2) + np.cos(ele1) * np.cos(ele2) * np.cos(np.abs(az1 - az2))
    dist = np.clip(dist, -1, 1)
    return np.arccos(dist) * 180 / np.pi


def distance_between_cartesian_coordinates(x1, y1, z1, x2, y2, z2):
    """
    Angular distance between two cartesian coordinates
    MORE: https://en.wikipedia.org/wiki/Great-circle_distance

    :return: angular distance in degrees
    """
    N1 = np.sqrt(x1**2 + y1**2 + z1**2 + 1e-10)
    N2 = np.sqrt(x2**2 + y2**2 + z2**2 + 1e-10)
    x1, y1, z1, x2, y2, z2 = x1/N1, y1/N1, z1/N1, x2/N2, y2/N2, z2/N2
    dist = x1*x2 + y1*y2 + z1*z2
    dist = np.clip(dist, -1, 1)
    return np.arccos(dist) * 180 / np.pi


def least_distance_between_gt_pred(gt_list, pred_list):
    """
        Shortest distance between two sets of DOA coordinates: the cost matrix of every reference against every
        predicted DOA and its least-cost association, on the device (hip_ops.assign_doas).
        :param gt_list: (g, 3) Cartesian or (g, 2) spherical coordinates in radians, g <= 8
        :param pred_list: (q, 3) or (q, 2) likewise, q <= 8
        :return: cost - distances of the min(g, q) associated pairs in degrees
        :return: row_ind, col_ind - their reference and predicted indices, rows ascending
    """
    gt_list, pred_list = np.asarray(gt_list, dtype=np.float64), np.asarray(pred_list, dtype=np.float64)
    g, q = gt_list.shape[0], pred_list.shape[0]
    if g == 0 or q == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    M = H.EVENT_METRICS_MAX_TRACKS_EX
    if g > M or q > M:
        raise L.SeldHipError(f"least_distance_between_gt_pred: {g} against {q} DOAs; the device association takes {M} a side")
    C = 3 if len(gt_list[0]) == 3 else 2                # the reference's test
    if gt_list.ndim != 2 or pred_list.ndim != 2 or gt_list.shape[1] != C or pred_list.shape[1] != C:
        raise L.SeldHipError(f"least_distance_between_gt_pred: DOAs of shapes {gt_list.shape} and {pred_list.shape}")
    if not torch.cuda.is_available():
        raise L.SeldHipError("least_distance_between_gt_pred: no HIP device (this package has no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    padded = np.zeros((2, 1, M, C))
    padded[0, 0, :g], padded[1, 0, :q] = gt_list, pred_list
    both = torch.from_numpy(padded).to(dev)
    counts = torch.tensor([[g], [q]], dtype=torch.int32).to(dev)
    cost, row, col, _ = H.assign_doas(both[0], both[1], counts[0], counts[1], spherical=C == 2)
    n = min(g, q)
    return cost[0, :n].cpu().numpy(), row[0, :n].cpu().numpy().astype(np.int64), col[0, :n].cpu().numpy().astype(np.int64)


def early_stopping_metric(sed_error, doa_error):
    """
    Compute early stopping metric from sed and doa errors.

    :param sed_error: [error rate (0 to 1 range), f score (0 to 1 range)]
    :param doa_error: [doa error (in degrees), frame recall (0 to 1 range)]
    :return: early stopping metric result
    """
    return np.mean([sed_error[0], 1 - sed_error[1], doa_error[0]/180, 1 - doa_error[1]])


def segment_labels(_pred_dict, _max_frames, _nb_label_frames_1s=10):
    '''
        Collects class-wise sound event location information in segments of length 1s from reference dataset
    :param _pred_dict: Dictionary containing frame-wise sound event time and location information. Output of SELD method
    :param _max_frames: Total number of frames in the recording
    :return: Dictionary containing class-wise sound event location information in each segment of audio
            dictionary_name[segment-index][class-index] = [[frame-cnt-within-segment ...], [[[x, y, z, event] ...] ...]]
    '''
    nb_blocks = int(np.ceil(_max_frames / float(_nb_label_frames_1s)))
    output_dict = {x: {} for x in range(nb_blocks)}
    for block_cnt, first in enumerate(range(0, _max_frames, _nb_label_frames_1s)):
        by_class = {}                                   # class -> {frame within the block: [event entries]}
        for audio_frame in range(first, first + _nb_label_frames_1s):
            for value in _pred_dict.get(audio_frame, ()):
                by_class.setdefault(value[0], {}).setdefault(audio_frame - first, []).append(value[1:])
        for class_cnt, frames in by_class.items():
            output_dict[block_cnt].setdefault(class_cnt, []).append([list(frames.keys()), list(frames.values())])
    return output_dict
