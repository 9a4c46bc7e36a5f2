"""The test leg: counters to the 16 results, the class report, prediction and scoring of samples and whole recordings."""
import contextlib
import json
import os
import sys

import numpy as np
import torch

from . import class_metrics as CM
from . import hip_ops as H
from .cli import class_report_from_args, postprocess_from_args


def test_results_from_counters(counts, total_de, epoch=0):
    """The 16 numbers of train.py:131-150 (with compute_seld_scores, Dcase21_metrics.py:33-49) from the counters."""
    eps_f, eps = sys.float_info.epsilon, np.finfo(float).eps
    TP, FP, FN = counts["TP"], counts["FP"], counts["FN"]
    precision = TP / (TP + FP + eps_f)
    recall = TP / (TP + FN + eps_f)
    F_score = 2 * ((precision * recall) / (precision + recall + eps_f))
    Nref, Nsys = TP + FN, TP + FP
    ER_score = (max(Nref, Nsys) - TP) / (Nref + 0.0)          # ZeroDivisionError without a reference event, as the reference
    ER_dcase21 = (counts["dc_S"] + counts["dc_D"] + counts["dc_I"]) / float(counts["dc_Nref"] + eps)
    F_dcase21 = counts["dc_TP"] / (eps + counts["dc_TP"] + 0.5 * (counts["dc_FP"] + counts["dc_FN"]))
    LE_dcase21 = total_de / float(counts["dc_DE_TP"] + eps) if counts["dc_DE_TP"] else 180
    LR_dcase21 = counts["dc_DE_TP"] / (eps + counts["dc_DE_TP"] + counts["dc_DE_FN"])
    SELD_dcase21 = np.mean([ER_dcase21, 1 - F_dcase21, LE_dcase21 / 180, 1 - LR_dcase21])
    SELD_L3DAS21_LRLE = np.mean([ER_score, 1 - F_score, LE_dcase21 / 180, 1 - LR_dcase21])
    CSL_score = np.mean([LE_dcase21 / 180, 1 - LR_dcase21])
    LSD_score = np.mean([1 - F_score, ER_score])
    return [epoch, F_score, ER_score, precision, recall, TP, FP, FN, CSL_score, LSD_score, SELD_L3DAS21_LRLE, SELD_dcase21,
            ER_dcase21, F_dcase21, LE_dcase21, LR_dcase21]


def _print_test_results(results):
    print('*******************************\nRESULTS')
    for label, v in (('TP: ', results[5]), ('FP: ', results[6]), ('FN: ', results[7]), ('Global SELD score: ', results[10]),
                     ('LSD score: ', results[9]), ('CSL score: ', results[8]), ('F score: ', results[1]),
                     ('ER score: ', results[2]), ('LE: ', results[14]), ('LR: ', results[15])):
        print(label, v)


def _results_from_row(row, total_de, epoch):
    """The 16 results from one row of counters (a list in hip_ops.METRIC_COUNTERS order) and its localisation error."""
    return test_results_from_counters(dict(zip(H.METRIC_COUNTERS, row)), float(total_de), epoch)


def _results_from_table(counters, total_de, epoch):
    """The 16 results from row "all" of a breakdown table (numpy, all recordings)."""
    all_c, all_de = CM.totals(counters, total_de)
    return _results_from_row(all_c[-1].tolist(), all_de[-1], epoch)


def class_report(counters, total_de, results, epoch=0, average="micro", report=True, results_path=None):
    """The per-class report of a test leg from its breakdown table (numpy (R, C + 2, 16) and (R, C + 2)): printed, returned
    as a dict and, with `results_path`, written to <results_path>/class_report.json.  report=False (metrics_average=macro
    alone): the macro line only, nothing written."""
    scores = CM.class_scores(counters, total_de)
    macro = CM.macro_scores(counters, total_de)
    jack = CM.jackknife(counters, total_de) if counters.shape[0] >= 2 else None
    names = ("ER", "F", "LE", "LR", "early_stopping_metric")
    stderr = dict(zip(names, jack["stderr"].tolist())) if jack is not None else None
    micro = dict(ER=results[12], F=results[13], LE=results[14], LR=results[15], early_stopping_metric=results[11])
    chosen = macro if average == "macro" else micro
    out = dict(epoch=int(epoch), recordings=int(counters.shape[0]), metrics_average=average,
               early_stopping_metric=float(chosen["early_stopping_metric"]),
               micro={k: float(v) for k, v in micro.items()}, macro={k: float(macro[k]) for k in names},
               macro_classes=macro["classes"], macro_jackknife_stderr=stderr,
               classes=[{k: (int(v[c]) if k == "Nref" else float(v[c])) for k, v in scores.items()}
                        for c in range(len(scores["Nref"]))])
    if report:
        print("class  Nref  precision  recall      F1       ER        F       LE       LR")
        for c, row in enumerate(out["classes"]):
            print(f"{c:5d} {row['Nref']:5d} {row['precision']:10.4f} {row['recall']:7.4f} {row['f1']:7.4f} {row['ER']:8.4f} "
                  f"{row['F']:8.4f} {row['LE']:8.3f} {row['LR']:8.4f}")
    print("macro (%d classes): " % macro["classes"]
          + "  ".join(f"{k} {macro[k]:.4f}" + (f" +- {stderr[k]:.4f}" if stderr else "") for k in names))
    print(f"early stopping metric ({average}): {out['early_stopping_metric']}")
    if report and results_path:
        os.makedirs(results_path, exist_ok=True)
        with open(os.path.join(results_path, "class_report.json"), "w") as f:
            json.dump(out, f, indent=1)
    return out


def evaluate_test(model, device, dataloader, epoch=0, max_loc_value=2., num_frames=600, spatial_threshold=2., args=None):
    """train.py:84-166: same arguments, same 16-entry result list.  The network outputs never leave the device: each
    batch's decode + counting is one kernel (hip_ops.metrics_accumulate) and the counters are read back once.
    --class_report / --metrics_average=macro: the counting is hip_ops.metrics_accumulate_by, the results come from row
    "all" of its table (the same numbers) and class_report prints and writes the rest."""
    class_overlaps = args.class_overlaps if args is not None else 3
    doa_threshold = args.Dcase21_metrics_DOA_threshold if args is not None else 20
    post = postprocess_from_args(args) if args is not None else None
    report, average = class_report_from_args(args)
    by = report or average == "macro"
    model.eval()
    acc, tables = H.metrics_new(device), []
    with torch.no_grad():
        for x, target in dataloader:
            sed, doa = model(x.to(device))
            if post is not None:
                sed, doa = H.smooth_tracks(sed, doa, **post.kwargs())
            # gen_submission_list_task2 is called with its default num_classes = 14 (train.py:110-116)
            rest = (target.to(device), num_frames, 14, class_overlaps, max_loc_value, spatial_threshold, doa_threshold)
            if by:
                tables.append(H.metrics_accumulate_by(sed, doa, *rest))
            else:
                H.metrics_accumulate(acc, sed, doa, *rest)
    return _close_test_leg(tables if by else acc, epoch, args, report, average)


def _close_test_leg(counted, epoch, args, report, average):
    """The close of every test leg: one read-back, the 16 results, their print and, for tables, the report.  `counted`: the
    dense accumulator of metrics_accumulate (a tuple), or the list of metrics_accumulate_by's tables in recording order."""
    if isinstance(counted, list):
        counters = torch.cat([t[0] for t in counted]).cpu().numpy()
        total_de = torch.cat([t[1] for t in counted]).cpu().numpy()
        results = _results_from_table(counters, total_de, epoch)
    else:
        results = _results_from_row(counted[0].cpu().tolist(), counted[1].item(), epoch)
    _print_test_results(results)
    if isinstance(counted, list):
        class_report(counters, total_de, results, epoch, average, report, getattr(args, "results_path", None))
    return results


def ema_scope(optimizer):
    """`optimizer.ema_weights()` for a FlatAdam that keeps a moving average of the weights (--ema_decay); a context that
    does nothing for None or any other optimiser.  `with ema_scope(optimizer): predict_test(model, ...)` -- or
    predict_test_post, predict_recordings, evaluate_test, evaluate_recordings -- predicts with the average, as main's
    validation and test leg do; the signatures of those functions stay what they were."""
    return optimizer.ema_weights() if getattr(optimizer, "ema", None) is not None else contextlib.nullcontext()


def predict_test(model, device, dataloader, max_loc_value=2., num_frames=600):
    """The prediction half of evaluate_test (train.py:100-111): the model under no_grad exactly as there, every batch
    decoded on the device (hip_ops.decode_events, with gen_submission_list_task2's default of 14 classes as the
    reference's call has it), and one (E_i, 5) float64 array of [frame, class, x, y, z] rows per recording, in loader
    order.  `num_frames` is accepted and ignored, as gen_submission_list_task2 does."""
    return _predict_test(model, device, dataloader, max_loc_value, None)


def predict_test_post(model, device, dataloader, max_loc_value=2., num_frames=600, post=None):
    """predict_test with post-processing: `post`, a hip_ops.PostProcess (or a dict of its settings), is applied to every
    batch's outputs on the device (hip_ops.smooth_tracks) before they are decoded.  None or the identity: nothing is
    launched and the rows are predict_test's."""
    return _predict_test(model, device, dataloader, max_loc_value, _active_post(post))


def _predict_test(model, device, dataloader, max_loc_value, post):
    model.eval()
    out = []
    with torch.no_grad():
        for x, _ in dataloader:
            sed, doa = model(x.to(device))
            if sed.shape[-1] % 14:
                raise H.L.SeldHipError(f"predict_test: {sed.shape[-1]} activity outputs are not 14 classes x overlaps")
            if post is not None:
                sed, doa = H.smooth_tracks(sed, doa, **post.kwargs())
            rows, _, offsets = H.decode_events(sed, doa, max_loc_value, 14, sed.shape[-1] // 14)
            rows, offsets = rows.cpu().numpy(), offsets.cpu().tolist()
            out.extend(rows[a:b] for a, b in zip(offsets[:-1], offsets[1:]))
    return out


MEMBER_BUFFER_BYTES = 1 << 30       # predict_recordings: recordings are taken in chunks whose member outputs stay below this


def _active_post(post):
    """`post` (a hip_ops.PostProcess, a dict of its settings or None) as a PostProcess, None when there is nothing to do."""
    if post is None:
        return None
    if isinstance(post, dict):
        post = H.PostProcess(**post)
    if not isinstance(post, H.PostProcess):
        raise TypeError(f"post must be a hip_ops.PostProcess, a dict of its settings or None, got {type(post).__name__}")
    return None if post.is_identity else post


def predict_recordings(model, x, *, seg_len, hop, table=None, window="triangular", align=True, batch=32, frames=None):
    """Whole recordings through the model: x (R, C, F, L) resident on the device -> (sed (R, frames, n), doa (R, frames, 3n))
    on the device.  Windows of seg_len frames every hop frames (hip_ops.window_count of them per recording), each under
    every row of `table` (K of them; None: the window as it is), go through the model `batch` members at a time
    (hip_ops.window_batch cuts and transforms a batch in one launch; the last batch is partial); one
    hip_ops.ensemble_combine per chunk of recordings then maps the DOAs back, aligns the slots of every (frame, class)
    (`align`, for models trained with --pit_loss a must) and averages with the weights `window`.  The pooling factor
    P = seg_len / T_out is read from the first forward: hop must be a multiple of it, frames defaults to L // P.
    n = classes * overlaps is split as 14 classes x n / 14 overlaps, the way predict_test reads it.  Under
    `ema_scope(optimizer)` the recordings are predicted with the moving average of the weights."""
    seg_len, hop, batch = int(seg_len), int(hop), int(batch)
    if x.dim() != 4 or not x.is_cuda:
        raise H.L.SeldHipError(f"predict_recordings: x must be a device tensor (R, C, F, L), got {tuple(x.shape)} on {x.device}")
    if batch < 1 or seg_len < 1 or hop < 1:
        raise H.L.SeldHipError(f"predict_recordings: seg_len, hop and batch must be positive, got {seg_len}, {hop}, {batch}")
    x = x.contiguous()
    R, C, F, length = x.shape
    S = H.window_count(length, seg_len, hop)
    if table is not None:
        table = H.ensemble_table(table, x.device, C)
    K = 1 if table is None else table.shape[0]
    model.eval()
    xb = torch.zeros((batch, C, F, seg_len), device=x.device)

    def forward(r0, rc, first, count):
        H.window_batch(x[r0:r0 + rc], xb, seg_len=seg_len, hop=hop, segments=S, table=table, first=first, count=count)
        return model(xb[:count])

    with torch.no_grad():
        count0 = min(batch, R * S * K)
        sed0, doa0 = forward(0, R, 0, count0)           # the first forward names the geometry
        t_out, n = sed0.shape[1], sed0.shape[2]
        if seg_len % t_out or hop % (seg_len // t_out):
            raise H.L.SeldHipError(f"predict_recordings: the model pools {seg_len} frames to {t_out}; hop {hop} must be a "
                                   f"multiple of {seg_len / t_out:g}")
        if n % 14:
            raise H.L.SeldHipError(f"predict_recordings: {n} activity outputs are not 14 classes x overlaps")
        pool = seg_len // t_out
        frames = length // pool if frames is None else int(frames)
        per_chunk = max(1, min(R, MEMBER_BUFFER_BYTES // (16 * S * K * t_out * n)))     # 4 n floats per member frame
        sed_m = torch.empty((per_chunk * S * K, t_out, n), device=x.device)
        doa_m = torch.empty((per_chunk * S * K, t_out, 3 * n), device=x.device)
        out_sed = torch.empty((R, frames, n), device=x.device)
        out_doa = torch.empty((R, frames, 3 * n), device=x.device)
        for r0 in range(0, R, per_chunk):
            rc = min(per_chunk, R - r0)
            members = rc * S * K
            for first in range(0, members, batch):
                count = min(batch, members - first)
                # members are numbered inside their chunk: the first forward is chunk 0's first batch unless the chunk is
                # smaller than that batch
                sed, doa = (sed0, doa0) if r0 == 0 and first == 0 and count == count0 else forward(r0, rc, first, count)
                sed_m[first:first + count] = sed
                doa_m[first:first + count] = doa
            sed_c, doa_c = H.ensemble_combine(sed_m[:members], doa_m[:members], recordings=rc, segments=S, hop_out=hop // pool,
                                              frames=frames, classes=14, overlaps=n // 14, table=table, window=window,
                                              align=align)
            out_sed[r0:r0 + rc] = sed_c
            out_doa[r0:r0 + rc] = doa_c
    return out_sed, out_doa


def evaluate_recordings(model, device, x_all, y_all, args, *, hop, table, epoch=0, window="triangular", align=True,
                        batch=32, max_loc_value=2., num_frames=600, spatial_threshold=2., post=None):
    """evaluate_test over whole recordings: x_all (R, C, F, L) and the targets y_all (R, frames, 4n) go through
    predict_recordings (seg_len = args.time_dim, `hop`, `table`) and the stitched outputs through
    hip_ops.metrics_accumulate; the same 16-entry result list, printed the same way.  `post`: a hip_ops.PostProcess
    applied to the stitched track (hip_ops.smooth_tracks, one launch for all recordings) before it is scored; None or the
    identity: nothing is launched."""
    post = _active_post(post)
    x_all = x_all.to(device)
    sed, doa = predict_recordings(model, x_all, seg_len=args.time_dim, hop=hop, table=table, window=window, align=align,
                                  batch=batch, frames=y_all.shape[1])
    if post is not None:
        sed, doa = H.smooth_tracks(sed, doa, **post.kwargs())
    report, average = class_report_from_args(args)
    if report or average == "macro":                    # one launch for all recordings: the table keeps them apart
        counted = [H.metrics_accumulate_by(sed, doa, y_all.to(device), num_frames, 14, args.class_overlaps, max_loc_value,
                                           spatial_threshold, args.Dcase21_metrics_DOA_threshold)]
    else:
        counted = H.metrics_new(device)
        for r in range(sed.shape[0]):                   # one recording per launch, as evaluate_test's loader gives them
            H.metrics_accumulate(counted, sed[r:r + 1], doa[r:r + 1], y_all[r:r + 1].to(device), num_frames, 14,
                                 args.class_overlaps, max_loc_value, spatial_threshold, args.Dcase21_metrics_DOA_threshold)
    return _close_test_leg(counted, epoch, args, report, average)
