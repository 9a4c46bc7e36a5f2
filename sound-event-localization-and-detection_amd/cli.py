"""The command line: the reference's flags and this implementation's, and what checks and turns them into objects."""
import argparse
import ast
import os
import sys

from . import hip_ops as H
from .model import SE_MODES, SELD_Model, _at_check, _rnn_check


# ------------------------------------------------------------------------------------------
# configuration (train.py:718-838, utility_functions.py:77-91)
# ------------------------------------------------------------------------------------------
def readFile(path):
    """Tokenise a flag file: split on '=' and newlines, 'True' -> '1', 'False' -> 0, drop '#' tokens."""
    with open(path, 'r') as f:
        toks = f.read().replace('=', '+').replace('\n', '+').split('+')
    out = []
    for t in toks:
        if t == 'True':
            out.append('1')
        elif t == 'False':
            out.append(0)
        elif t != '' and '#' not in t:
            out.append(t)
    return out


_FLAGS = [
    ('results_path', str, 'RESULTS/Task2'), ('checkpoint_dir', str, 'RESULTS/Task2'), ('load_model', str, None),
    ('training_predictors_path', str, '/var/datasets/L3DAS21/processed/task2_predictors_train.pkl'),
    ('training_target_path', str, '/var/datasets/L3DAS21/processed/task2_target_train.pkl'),
    ('validation_predictors_path', str, '/var/datasets/L3DAS21/processed/task2_predictors_validation.pkl'),
    ('validation_target_path', str, '/var/datasets/L3DAS21/processed/task2_target_validation.pkl'),
    ('test_predictors_path', str, '/var/datasets/L3DAS21/processed/task2_predictors_test.pkl'),
    ('test_target_path', str, '/var/datasets/L3DAS21/processed/task2_target_test.pkl'),
    ('gpu_id', int, 0), ('use_cuda', str, 'True'), ('early_stopping', str, 'True'), ('fixed_seed', str, 'True'),
    ('lr', float, 0.0001), ('batch_size', int, 1), ('sr', int, 32000), ('patience', int, 250),
    ('architecture', str, 'DualQSELD-TCN'), ('input_channels', int, 4), ('n_mics', int, 1), ('phase', str, 'False'),
    ('class_overlaps', int, 3), ('time_dim', int, 4800), ('freq_dim', int, 256), ('output_classes', int, 14),
    ('pool_size', str, '[[8,2],[8,2],[2,2],[1,1]]'), ('cnn_filters', str, '[64,64,64]'), ('pool_time', str, 'True'),
    ('dropout_perc', float, 0.3), ('D', str, '[10]'), ('G', int, 128), ('U', int, 128), ('V', str, '[128,128]'),
    ('spatial_dropout_rate', float, 0.5), ('batch_norm', str, 'BN'), ('dilation_mode', str, 'fibonacci'),
    ('model_extra_name', str, ''), ('test_mode', str, 'test_best'), ('use_lr_scheduler', str, 'True'),
    ('lr_scheduler_step_size', int, 150), ('lr_scheduler_gamma', float, 0.5), ('min_lr', float, 0.000005),
    ('dataset_normalization', str, 'True'), ('kernel_size_cnn_blocks', int, 3), ('kernel_size_dilated_conv', int, 3),
    ('use_tcn', str, 'True'), ('use_bias_conv', str, 'True'), ('use_bias_linear', str, 'True'), ('verbose', str, 'False'),
    ('sed_loss_weight', float, 1.), ('doa_loss_weight', float, 5.), ('domain_classifier', str, 'same'),
    ('domain', str, 'DQ'), ('fc_activations', str, 'Linear'), ('fc_dropout', str, 'Last'), ('fc_layers', str, '[128]'),
    ('V_kernel_size', int, 3), ('use_time_distributed', str, 'False'), ('parallel_ConvTC_block', str, 'False'),
    ('max_loc_value', float, 2.), ('num_frames', int, 600), ('spatial_threshold', float, 2.),
    ('checkpoint_step', int, 100), ('test_step', int, 10), ('min_n_epochs', int, 1000),
    ('Dcase21_metrics_DOA_threshold', int, 20), ('parallel_magphase', str, 'False'),
    ('TextArgs', str, 'config/Test.txt'),
]
_EVAL = ('use_cuda', 'early_stopping', 'fixed_seed', 'pool_size', 'cnn_filters', 'verbose', 'D', 'V', 'use_lr_scheduler',
         'phase', 'use_tcn', 'use_bias_conv', 'use_bias_linear', 'fc_layers', 'parallel_magphase',
         'resident_loader', 'graph_step', 'pit_loss', 'class_report', 'decoupled_weight_decay')
# extensions of this implementation (not in the reference): synthetic data so the step can run without L3DAS21;
# resident_loader: minibatches gathered on the device (ResidentLoader) instead of a DataLoader over the resident arrays;
# graph_step (needs resident_loader): full batches run as replays of one recorded step (GraphedTrainStep);
# augment_* (need resident_loader; training loader only; all off by default): augmentation inside the gather launch
# (hip_ops.gather_rows_aug) -- augment_swap: probability of a signed FOA channel permutation with its DOA labels
# (hip_ops.foa_transforms for --n_mics / --phase); augment_freq_masks / augment_time_masks: 0..2 masks per sample of a
# width up to augment_freq_width / augment_time_width bins; augment_seed: the key of the draws;
# feature_layout (magphase by default): the channel layout of the predictors for augment_swap and test_tta -- quaternion, iv
# or logpower_iv for the intensity features of hip_ops.spatial_features, whose components are negated, not turned by pi;
# augment_rotate (needs a feature_layout of quaternion or iv, or magphase with --phase=True; not with augment_swap):
# probability that a sample's sound field is rotated about the vertical axis by a random angle, with random mirrors in y
# and z, and its DOA labels with it (hip_ops.gather_rows_rot, the same single launch).  On magphase predictors with
# phase (hip_ops.gather_rows_polar) magnitude and phase of a bin are one complex number and the STFT is linear: per
# microphone and (f, t) the complex vector (X, Y, Z) = m e^(i phi) becomes R (X, Y, Z), W stays; a standardising
# dataset_normalization is undone and redone around it with the training array's statistics; two spaced microphones
# share one R, the approximation hip_ops.foa_transforms documents for mics=2.  Magnitudes alone are not covariant and stay
# refused; test_tta and augment_swap keep their rules (augment_swap with phase still needs raw phase);
# pit_loss (off by default): the loss takes, per (frame, class), the cheapest pairing of the class_overlaps prediction
# slots with the target slots (hip_ops.seld_loss_pit) instead of comparing slot o with slot o -- training steps (eager,
# data parallel, recorded) and the validation loss alike;
# test_hop / test_tta (both 0 by default: the test leg is evaluate_test over pre-cut samples): the test leg runs whole
# recordings (evaluate_recordings) -- windows of time_dim frames every test_hop frames (0: time_dim, no overlap), each
# under the 8 (z fixed) or 16 signed FOA axis permutations of hip_ops.foa_transforms for --n_mics / --phase when
# test_tta is 8 or 16, stitched back on the device (hip_ops.window_batch, hip_ops.ensemble_combine);
# post_* (all off by default: then nothing is launched): the test leg post-processes the network's or the ensemble's track
# on the device before it is scored (hip_ops.smooth_tracks) -- post_median: odd window of a median filter on the activity;
# post_on / post_off: hysteresis, a stretch above post_off is an event iff it holds a frame above post_on;
# post_max_gap: gaps of at most so many frames between two events are filled; post_min_frames: shorter events are
# dropped; post_doa: frame, mean or weighted -- one DOA per event;
# class_report (off by default): the test leg scores with hip_ops.metrics_accumulate_by, returns and prints the same 16
# results (from row "all" of the table), then prints per class Nref, precision / recall / F1 and ER, F, LE, LR, the class-wise
# macro averages with their leave-one-recording-out standard errors (class_metrics), and writes class_report.json under
# results_path; metrics_average: micro or macro -- which ER, F, LE, LR feed the early stopping metric the report states
# (macro builds the table too; the 16 results stay the micro ones either way);
# grad_clip / weight_decay / decoupled_weight_decay / ema_decay / warmup_steps (all off by default: then the optimiser
# allocates and launches what it always did) -- grad_clip=G: the global gradient norm is clipped to G inside the step
# (hip_ops.grad_norm, one launch, the coefficient stays on the device; eager, data-parallel and recorded steps alike) and
# the epoch line prints the largest norm and the share of clipped steps; weight_decay=W: L2 decay added to the gradient,
# or with decoupled_weight_decay=True torch.optim.AdamW's shrinking of the weights; ema_decay=D: an exponential moving
# average of the weights, updated inside Adam's launch, under which validation and the test leg run and which the
# checkpoints carry as `ema_state_dict` beside the training weights; warmup_steps=N: the learning rate is
# lr * min(1, step / N) on top of StepLR (host side: the factor FlatAdam.lr_scale);
# at_key_size / at_value_size / at_mask / at_band (off by default): at_key_size=K puts a temporal-attention block
# (hip_nn.TemporalAttention, key width K, value width at_value_size or K) in front of every dilation stack of the TCN;
# at_mask: none | causal | band, the band +-at_band frames wide;
# augment_mix=P (off by default; needs resident_loader, feature_layout=magphase and phase=True; not with augment_rotate or
# augment_swap; masks go with it): with probability P another clip of the epoch is mixed into a sample with a gain drawn
# from [augment_mix_gain_lo, augment_mix_gain_hi] (hip_ops.gather_rows_mix, the same single launch): per bin the complex
# sum z_A + g z_B, which is the STFT of the mixed waveforms, and per (frame, class) the active track slots of both targets
# packed into the class_overlaps slots.  A pair of clips that could overflow a class (hip_ops.target_occupancy, computed
# once for the training array) is not mixed, so no label is dropped; a standardising dataset_normalization is undone and
# redone around the sum with the training array's statistics.  Magnitudes alone and intensity vectors are not linear in the
# waveform and stay refused;
# rnn_size / rnn_layers (read only with the reference's --use_tcn=False, which needs --pool_time=CNN): the TCN is replaced by
# rnn_layers bidirectional GRU layers of rnn_size units (hip_nn.GRU, at most 128), the back end of SELDnet / QSELDnet
_EXTRA = [('synthetic', int, 0), ('max_steps', int, 0), ('epochs', int, 0), ('resident_loader', str, 'False'),
          ('graph_step', str, 'False'), ('augment_swap', float, 0.), ('augment_freq_masks', int, 0),
          ('augment_freq_width', int, 0), ('augment_time_masks', int, 0), ('augment_time_width', int, 0),
          ('augment_seed', int, 0), ('feature_layout', str, 'magphase'), ('augment_rotate', float, 0.),
          ('pit_loss', str, 'False'), ('test_hop', int, 0), ('test_tta', int, 0),
          ('post_median', int, 1), ('post_on', float, 0.5), ('post_off', float, 0.5), ('post_min_frames', int, 1),
          ('post_max_gap', int, 0), ('post_doa', str, 'frame'), ('se_reduction', int, 0), ('se_mode', str, 'both'),
          ('class_report', str, 'False'), ('metrics_average', str, 'micro'),
          ('grad_clip', float, 0.), ('weight_decay', float, 0.), ('decoupled_weight_decay', str, 'False'),
          ('ema_decay', float, 0.), ('warmup_steps', int, 0),
          ('at_key_size', int, 0), ('at_value_size', int, 0), ('at_mask', str, 'causal'), ('at_band', int, 0),
          ('augment_mix', float, 0.), ('augment_mix_gain_lo', float, 0.5), ('augment_mix_gain_hi', float, 1.0),
          ('rnn_size', int, 128), ('rnn_layers', int, 2)]


def build_parser():
    p = argparse.ArgumentParser()
    for name, typ, default in _FLAGS + _EXTRA:
        p.add_argument('--' + name, type=typ, default=default)
    return p


def parse_args(argv=None):
    """Two-pass parse like train.py:819-820: argv selects --TextArgs, the file supplies the flags.  Flags the
    reference's parser would reject (e.g. --phm_n in the shipped Q config) are reported, not fatal."""
    parser = build_parser()
    first, _ = parser.parse_known_args(argv)
    tokens = [str(t) for t in readFile(first.TextArgs)] if os.path.isfile(first.TextArgs) else []
    args, unknown = parser.parse_known_args(tokens + list(argv or []))
    if unknown:
        print("ignoring flags unknown to the reference's parser:", unknown, file=sys.stderr)
    for k in _EVAL:
        v = getattr(args, k)
        if isinstance(v, str):
            setattr(args, k, ast.literal_eval(v))
    return args


def pit_overlaps_from_args(args):
    """class_overlaps under --pit_loss, else 0 (the slot-bound loss)."""
    return int(args.class_overlaps) if getattr(args, "pit_loss", False) else 0


def se_from_args(args):
    """dict(se_reduction=, se_mode=) of the --se_reduction / --se_mode flags for SELD_Model (squeeze-and-excitation blocks;
    reduction 0, also for an args object without the flags: none).  Every refusal comes before the device is touched."""
    reduction, mode = getattr(args, "se_reduction", 0), getattr(args, "se_mode", "both")
    if isinstance(reduction, bool) or not isinstance(reduction, int) or reduction < 0:
        raise ValueError(f"--se_reduction must be a non-negative integer (0: no squeeze-and-excitation), got {reduction!r}")
    if mode not in SE_MODES:
        raise ValueError(f"--se_mode must be one of {', '.join(SE_MODES)}, got {mode!r}")
    return dict(se_reduction=reduction, se_mode=mode)


def at_from_args(args):
    """dict(at_key_size=, at_value_size=, at_mask=, at_band=) of the --at_* flags for SELD_Model (temporal-attention
    blocks; key size 0, also for an args object without the flags: none).  Every refusal comes before the device is
    touched."""
    kw = dict(at_key_size=getattr(args, "at_key_size", 0), at_value_size=getattr(args, "at_value_size", 0),
              at_mask=getattr(args, "at_mask", "causal"), at_band=getattr(args, "at_band", 0))
    try:
        _at_check(**kw)
    except ValueError as e:
        raise ValueError("--" + str(e)) from None
    return kw


def rnn_from_args(args):
    """dict(use_tcn=, rnn_size=, rnn_layers=) of the --use_tcn / --rnn_size / --rnn_layers flags for SELD_Model
    (use_tcn=False: bidirectional GRUs in place of the TCN; an args object without the flags: the TCN), checked against
    --pool_time, --se_mode and --at_key_size.  Every refusal comes before the device is touched."""
    kw = dict(use_tcn=getattr(args, "use_tcn", True), rnn_size=getattr(args, "rnn_size", 128),
              rnn_layers=getattr(args, "rnn_layers", 2))
    try:
        _rnn_check(pool_time=getattr(args, "pool_time", "CNN"), se_mode=getattr(args, "se_mode", "both"),
                   at_key_size=getattr(args, "at_key_size", 0), **kw)
    except ValueError as e:
        raise ValueError("--" + str(e)) from None
    return kw


def optimizer_from_args(args):
    """FlatAdam's keyword arguments of the --grad_clip / --weight_decay / --decoupled_weight_decay / --ema_decay flags, after
    checking them and --warmup_steps (an args object without the flags: everything off).  Every refusal comes before the
    device is touched."""
    clip, decay = getattr(args, "grad_clip", 0.), getattr(args, "weight_decay", 0.)
    ema, warmup = getattr(args, "ema_decay", 0.), getattr(args, "warmup_steps", 0)
    decoupled = getattr(args, "decoupled_weight_decay", False)
    if not clip >= 0.:
        raise ValueError(f"--grad_clip must not be negative (0: no clipping), got {clip!r}")
    if not decay >= 0.:
        raise ValueError(f"--weight_decay must not be negative, got {decay!r}")
    if not isinstance(decoupled, (bool, int)):
        raise ValueError(f"--decoupled_weight_decay is True or False, got {decoupled!r}")
    if not 0. <= ema < 1.:
        raise ValueError(f"--ema_decay must lie in [0, 1) (0: no moving average), got {ema!r}")
    if isinstance(warmup, bool) or not isinstance(warmup, int) or warmup < 0:
        raise ValueError(f"--warmup_steps must be a non-negative integer (0: no warm-up), got {warmup!r}")
    return dict(weight_decay=float(decay), decoupled=bool(decoupled) and decay > 0, max_grad_norm=float(clip),
                ema_decay=float(ema))


def model_from_args(args):
    """train.py:448-465, plus the squeeze-and-excitation, temporal-attention and recurrent-back-end flags."""
    return SELD_Model(time_dim=args.time_dim, freq_dim=args.freq_dim, input_channels=args.input_channels,
                      output_classes=args.output_classes, domain=args.domain, domain_classifier=args.domain_classifier,
                      cnn_filters=args.cnn_filters, kernel_size_cnn_blocks=args.kernel_size_cnn_blocks,
                      pool_size=args.pool_size, pool_time=args.pool_time, D=args.D, dilation_mode=args.dilation_mode,
                      G=args.G, U=args.U, kernel_size_dilated_conv=args.kernel_size_dilated_conv,
                      spatial_dropout_rate=args.spatial_dropout_rate, V=args.V, V_kernel_size=args.V_kernel_size,
                      fc_layers=args.fc_layers, fc_activations=args.fc_activations, fc_dropout=args.fc_dropout,
                      dropout_perc=args.dropout_perc, class_overlaps=args.class_overlaps, use_bias_conv=args.use_bias_conv,
                      use_bias_linear=args.use_bias_linear, batch_norm=args.batch_norm,
                      parallel_ConvTC_block=args.parallel_ConvTC_block, parallel_magphase=args.parallel_magphase,
                      extra_name=args.model_extra_name, verbose=args.verbose, **se_from_args(args),
                      **at_from_args(args), **rnn_from_args(args))


_NORM_OFF = {'False', 'false', 'None', 'none'}
_NORM_UNIT = {'DQ_Normalization', 'UnitNormNormalization', 'UnitNorm'}


FEATURE_LAYOUTS = ('magphase', 'quaternion', 'iv', 'logpower_iv')


def feature_layout(args, flag):
    """--feature_layout, checked for the flag that needs it (args without it: magphase).  The intensity layouts hold no
    phase channels and come from 1 or 2 groups of [W, D1, D2, D3]."""
    layout = getattr(args, 'feature_layout', 'magphase')
    if layout not in FEATURE_LAYOUTS:
        raise ValueError(f"--feature_layout is one of {', '.join(FEATURE_LAYOUTS)}, got {layout!r}")
    if layout != 'magphase' and args.phase:
        raise ValueError(f"{flag} with --feature_layout={layout}: that layout has no phase channels, not with --phase")
    return layout


def augment_requested(args):
    return (args.augment_swap > 0 or args.augment_freq_masks > 0 or args.augment_time_masks > 0
            or getattr(args, 'augment_rotate', 0.) > 0 or getattr(args, 'augment_mix', 0.) != 0)


def augment_from_args(args, device):
    """The hip_ops.Augment of the --augment_* flags for the training loader, None when they are all off.  Every refusal
    comes before the device is touched."""
    if not augment_requested(args):
        return None
    if not args.resident_loader:
        raise ValueError("--augment_* flags need --resident_loader (the augmentation is part of the device gather)")
    swap, rotate = args.augment_swap > 0, getattr(args, 'augment_rotate', 0.)
    if not 0. <= rotate <= 1.:
        raise ValueError(f"--augment_rotate is a probability, got {rotate}")
    mix = getattr(args, 'augment_mix', 0.)
    if not 0. <= mix <= 1.:
        raise ValueError(f"--augment_mix is a probability, got {mix}")
    if mix > 0:
        if rotate > 0 or swap:
            raise ValueError("--augment_mix with --augment_rotate or --augment_swap: one transforming gather per sample "
                             "(composing them in one launch is not built)")
        layout = feature_layout(args, "--augment_mix")
        if layout != 'magphase' or not args.phase:
            raise ValueError(f"--augment_mix needs --feature_layout=magphase with --phase=True, got {layout}"
                             + ("" if args.phase else " without phase")
                             + ": magnitude and phase together are linear in the waveform (the mixture's spectrum is the sum "
                               "of the spectra); magnitudes alone and intensity vectors are not linear and cannot be mixed")
        lo, hi = args.augment_mix_gain_lo, args.augment_mix_gain_hi
        if not (0. < lo <= hi < float('inf')):
            raise ValueError(f"--augment_mix_gain_lo / --augment_mix_gain_hi need finite 0 < lo <= hi, got {lo}, {hi}")
        if not 1 <= args.class_overlaps <= H.loader.MIX_MAX_OVERLAPS:
            raise ValueError(f"--augment_mix packs at most {H.loader.MIX_MAX_OVERLAPS} track slots per class, got --class_overlaps "
                             f"{args.class_overlaps}")
        return H.Augment(freq_masks=args.augment_freq_masks, freq_width=args.augment_freq_width, time_masks=args.augment_time_masks,
                         time_width=args.augment_time_width, device=device, p_mix=mix, mix_gain=(lo, hi))
    if rotate > 0 and swap:
        raise ValueError("--augment_rotate with --augment_swap: the rotations with their mirrors contain the signed "
                         "permutations, one channel transform per sample")
    layout = feature_layout(args, "--augment_swap" if swap else "--augment_rotate") if swap or rotate > 0 else 'magphase'
    polar = rotate > 0 and layout == 'magphase' and bool(args.phase)
    if rotate > 0 and not polar and layout not in ('quaternion', 'iv'):
        raise ValueError(f"--augment_rotate needs --feature_layout=quaternion or iv (every directional channel an intensity "
                         f"component) or magphase with --phase=True, got {layout}"
                         + (": magnitudes alone cannot be rotated, magnitude and phase together (--phase=True) can"
                            if layout == 'magphase' else ""))
    if rotate > 0 and args.n_mics not in (1, 2):
        raise ValueError(f"--augment_rotate: the FOA layouts are for 1 or 2 microphones, got --n_mics {args.n_mics}")
    mode = str(args.dataset_normalization)
    if swap and args.phase and mode not in _NORM_OFF and mode not in _NORM_UNIT:
        raise ValueError("--augment_swap with --phase needs raw phase (a sign flip turns the phase by pi): not with a "
                         "standardising --dataset_normalization")
    if swap and args.n_mics not in (1, 2):
        raise ValueError(f"--augment_swap: the FOA transform preset is for 1 or 2 microphones, got --n_mics {args.n_mics}")
    table = H.foa_transforms(mics=args.n_mics, phase=bool(args.phase), layout=layout) if swap else None
    triples = H.foa_triples(mics=args.n_mics, layout=layout) if rotate > 0 and not polar else None
    groups = H.foa_polar(mics=args.n_mics) if polar else None
    return H.Augment(table=table, p_swap=args.augment_swap if swap else 0.0, freq_masks=args.augment_freq_masks,
                     freq_width=args.augment_freq_width, time_masks=args.augment_time_masks,
                     time_width=args.augment_time_width, device=device, p_rot=rotate, rot_triples=triples, rot_polar=groups)


def class_report_from_args(args):
    """(report, average) of the --class_report / --metrics_average flags; an args object without them counts as (False,
    'micro').  Every refusal comes before the device is touched."""
    report, average = getattr(args, "class_report", False), getattr(args, "metrics_average", "micro")
    if not isinstance(report, (bool, int)):
        raise ValueError(f"--class_report is True or False, got {report!r}")
    if average not in ("micro", "macro"):
        raise ValueError(f"--metrics_average is micro or macro, got {average!r}")
    return bool(report), average


def ensemble_requested(args):
    return args.test_hop != 0 or args.test_tta != 0


def ensemble_from_args(args):
    """dict(hop=, table=) of the --test_hop / --test_tta flags for evaluate_recordings (the table on the host, None
    without test-time augmentation), None when both are 0.  Every refusal comes before the device is touched."""
    if not ensemble_requested(args):
        return None
    if args.test_hop < 0:
        raise ValueError(f"--test_hop must not be negative, got {args.test_hop}")
    if args.test_tta not in (0, 8, 16):
        raise ValueError(f"--test_tta is 0, 8 (the z axis fixed) or 16 transforms, got {args.test_tta}")
    table = None
    if args.test_tta:
        layout = feature_layout(args, "--test_tta")
        mode = str(args.dataset_normalization)
        if args.phase and mode not in _NORM_OFF and mode not in _NORM_UNIT:
            raise ValueError("--test_tta with --phase needs raw phase (a sign flip turns the phase by pi): not with a "
                             "standardising --dataset_normalization")
        if args.n_mics not in (1, 2):
            raise ValueError(f"--test_tta: the FOA transform preset is for 1 or 2 microphones, got --n_mics {args.n_mics}")
        table = H.foa_transforms(mics=args.n_mics, phase=bool(args.phase), elevation=args.test_tta == 16, layout=layout)
    return dict(hop=args.test_hop or args.time_dim, table=table)


def postprocess_requested(args):
    return (getattr(args, "post_median", 1) != 1 or getattr(args, "post_on", 0.5) != 0.5
            or getattr(args, "post_off", 0.5) != 0.5 or getattr(args, "post_min_frames", 1) != 1
            or getattr(args, "post_max_gap", 0) != 0 or getattr(args, "post_doa", "frame") != "frame")


def postprocess_from_args(args):
    """The hip_ops.PostProcess of the --post_* flags for the test leg, None when they are all at their defaults (an args
    object without them counts as that).  Every refusal comes before the device is touched."""
    if not postprocess_requested(args):
        return None
    try:
        return H.PostProcess(median=args.post_median, on=args.post_on, off=args.post_off, min_frames=args.post_min_frames,
                             max_gap=args.post_max_gap, doa=args.post_doa)
    except ValueError as err:
        raise ValueError(f"--post_*: {err}") from None
