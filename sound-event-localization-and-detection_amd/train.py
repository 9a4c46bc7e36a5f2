"""Training harness with the CLI of the reference's train.py (`python train.py --TextArgs=config/X.txt`,
same flag names and defaults, train.py:719-818) and its step semantics (train.py:186-204, 498-508, 538-571):

    zero_grad -> forward -> BCELoss(sed) * w_sed + MSELoss(doa) * w_doa -> backward -> Adam(lr 1e-4)

on the gfx950 kernels: the loss is one fused kernel, Adam is ONE launch over a flat parameter buffer,
and under torch.distributed (one process per GPU, RCCL) the gradient exchange is ONE all-reduce of the
flat gradient buffer (the reference is single-device).

The reference's own `main()` cannot run on a current stack (np.Inf, StepLR(verbose=), wandb, ...);
this file restates its behaviour rather than its text.
"""
import functools
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

# The harness lives in the sibling modules ("Training harness layout"); every name that was ever reached as
# train.<name> is imported here by name.  `main` refers to them as this module's globals, so replacing one on this
# module (tests and tools do: FlatAdam, warmup_scale, evaluate_test, evaluate_recordings, model_from_args, evaluate)
# changes what `main` calls, and nothing else.  `evaluate` stays here with `seld_loss`, which it calls: no sibling
# module imports this one.
from .checkpoint import CheckpointRotation, load_model, save_model  # noqa: F401
from .cli import (_EVAL, _EXTRA, _FLAGS, _NORM_OFF, _NORM_UNIT, FEATURE_LAYOUTS, at_from_args, augment_from_args,  # noqa: F401
                  augment_requested, build_parser, class_report_from_args, ensemble_from_args, ensemble_requested,
                  feature_layout, model_from_args, optimizer_from_args, parse_args, pit_overlaps_from_args,
                  postprocess_from_args, postprocess_requested, readFile, rnn_from_args, se_from_args)
from .data import (_DOMAIN_DQ, ResidentLoader, _normalize_dataset, epoch_left_out, epoch_plan, load_pickled,  # noqa: F401
                   normalize_dataset, polar_stats_from, rank_rows, synthetic_batch)
from .evaluate import (MEMBER_BUFFER_BYTES, _active_post, _predict_test, _print_test_results, _results_from_table,  # noqa: F401
                       class_report, ema_scope, evaluate_recordings, evaluate_test, predict_recordings, predict_test,
                       predict_test_post, test_results_from_counters)
from .optim import FlatAdam, StepLR, _torch_adam_defaults, warmup_scale  # noqa: F401
from .step import GraphedTrainStep, seld_loss_fn, train_step, training_restore, training_snapshot  # noqa: F401


class BCELoss(nn.Module):
    """Marker modules so that `seld_loss(x, target, model, criterion_sed, criterion_doa)` keeps the reference's
    signature; the two criteria are evaluated together by one fused kernel."""


class MSELoss(nn.Module):
    pass


def seld_loss(x, target, model, criterion_sed, criterion_doa, args=None):
    """train.py:186-204.  `args` carries output_classes / class_overlaps / loss weights (the reference reads a
    module-level global)."""
    a = args if args is not None else globals().get("args")
    n_sed = int(a.output_classes * a.class_overlaps)
    sed, doa = model(x)
    if isinstance(criterion_sed, BCELoss) and isinstance(criterion_doa, MSELoss):
        return seld_loss_fn(sed, doa, target, n_sed, a.sed_loss_weight, a.doa_loss_weight, pit_overlaps_from_args(a))
    t_sed, t_doa = target[:, :, :n_sed], target[:, :, n_sed:]
    return criterion_sed(torch.flatten(sed, 1), torch.flatten(t_sed, 1)) * a.sed_loss_weight + \
        criterion_doa(torch.flatten(doa, 1), torch.flatten(t_doa, 1)) * a.doa_loss_weight


def evaluate(model, device, criterion_sed, criterion_doa, loader, args):
    """Mean loss over a loader, no grad (train.py:168-183)."""
    model.eval()
    total, n = 0.0, 0
    with torch.no_grad():
        for x, target in loader:
            loss = seld_loss(x.to(device), target.to(device), model, criterion_sed, criterion_doa, args)
            n += 1
            total += (loss.item() - total) / n
    return total


def main(args, history=None):
    """The reference's training loop.  --resident_loader / --graph_step: see cli._EXTRA.  Started under
    `python -m torch.distributed.run --nproc-per-node N` it trains data parallel (needs --resident_loader): --batch_size
    is the global batch, every rank takes its share of each batch; validation, the test leg, checkpoints and printing
    are rank 0's; the training loss it prints is the mean over the ranks.  `history`: a list that receives (epoch, train
    loss, validation loss) per epoch, unrounded (rank 0).
    SELD_DP_BACKEND=gloo with SELD_DP_SINGLE_DEVICE=1 puts every rank on --gpu_id over gloo (RCCL refuses two ranks on one
    device): how a machine with one GPU runs the data-parallel loop, tests/test_gpu_train_loader.py included."""
    from . import dp as DP
    resident, graph_step = bool(args.resident_loader), bool(args.graph_step)
    if graph_step and not resident:
        raise ValueError("--graph_step needs --resident_loader")
    if augment_requested(args) and not resident:
        raise ValueError("--augment_* flags need --resident_loader (the augmentation is part of the device gather)")
    if getattr(args, 'augment_mix', 0.) != 0:
        augment_from_args(args, "cpu")                  # its refusals, before the device is touched
    ensemble = ensemble_from_args(args)
    post = postprocess_from_args(args)
    class_report_from_args(args)
    pit = pit_overlaps_from_args(args)
    se_from_args(args)
    at_from_args(args)
    rnn_from_args(args)
    extras = optimizer_from_args(args)
    warmup_steps = getattr(args, "warmup_steps", 0)
    if pit > 3:
        raise ValueError(f"--pit_loss searches the pairings of at most 3 slots per class, got --class_overlaps {pit}")
    if not args.use_cuda or not torch.cuda.is_available():
        raise RuntimeError("this implementation has no CPU path: a HIP device is required")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:                                   # every refusal before any GPU work
        if not resident or args.synthetic:
            raise ValueError("data-parallel training (WORLD_SIZE > 1) needs --resident_loader and pickled arrays")
        if world > 8:
            raise ValueError(f"at most 8 ranks, got WORLD_SIZE={world}")
        if args.batch_size % world:
            raise ValueError(f"--batch_size {args.batch_size} (the global batch) is not divisible by the {world} ranks")
    rank, local, world = DP.init_from_env(os.environ.get("SELD_DP_BACKEND"))
    if os.environ.get("SELD_DP_SINGLE_DEVICE"):
        local = args.gpu_id
    device = torch.device('cuda:' + str(args.gpu_id))
    if world > 1:
        device = torch.device('cuda', local)
        torch.cuda.set_device(device)
    say = print if rank == 0 else (lambda *a, **k: None)
    if args.fixed_seed:
        np.random.seed(1)
        torch.manual_seed(1)
    model = model_from_args(args).to(device)
    say('Total paramters: ' + str(sum(int(np.prod(p.size())) for p in model.parameters())))
    criterion_sed, criterion_doa = BCELoss(), MSELoss()
    sync = None
    if world > 1:
        DP.seed_rank_streams(rank)
        optimizer = FlatAdam(model.parameters(), lr=args.lr, late=DP.late_parameters(model), **extras)
        DP.broadcast_parameters(optimizer.flat_param)
        optimizer.ema_reset()               # the moving average starts from the weights every rank now holds
        sync = DP.BucketedGradSync(optimizer, model)
    else:
        optimizer = FlatAdam(model.parameters(), lr=args.lr, **extras)
    scheduler = StepLR(optimizer, args.lr_scheduler_step_size, args.lr_scheduler_gamma) if args.use_lr_scheduler else None
    n_out = int(args.output_classes * args.class_overlaps)
    # bound once: the eager and the recorded step take the loss `evaluate` reaches through seld_loss(..., args)
    loss_fn = functools.partial(seld_loss_fn, pit_overlaps=pit) if pit else seld_loss_fn

    if args.synthetic:
        data = [synthetic_batch(args.batch_size, args.input_channels, args.freq_dim, args.time_dim, n_out, 1234 + i, device)
                for i in range(args.synthetic)]
        tr_data, val_data = data, data[:1]
        test_data = None
        if resident:
            raise ValueError("--resident_loader reads pickled arrays: not with --synthetic")
    else:
        def loader(x, y, batch_size, shuffle, rank=0, world=1, augment=None, polar_stats=None):
            if resident:
                return ResidentLoader(x, y, batch_size, shuffle, rank, world, augment=augment, seed=args.augment_seed,
                                      polar_stats=polar_stats, overlaps=args.class_overlaps if augment is not None else None)
            return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, y), batch_size, shuffle=shuffle,
                                               pin_memory=False)
        augment = augment_from_args(args, device)      # the training loader's alone: validation and test see the data as it is
        xs, ys = load_pickled(args.training_predictors_path, args.training_target_path)
        xs = xs.to(device)                              # 288 GB of HBM: the arrays stay resident, loaders index them
        val_data = test_data = None
        norm_stats = []
        if rank == 0:
            xv, yv = load_pickled(args.validation_predictors_path, args.validation_target_path)
            xv = xv.to(device)
            print(normalize_dataset(args, xs, xv, stats=norm_stats))
        else:
            normalize_dataset(args, xs, stats=norm_stats)
        # the rotating gather of magnitude-phase predictors undoes and redoes the standardisation: it takes the training
        # array's own statistics, which every rank computed from the same array
        polar = augment is not None and augment.kind in ("polar", "mix")        # the mix does the same around its sum
        tr_data = loader(xs, ys, args.batch_size, True, rank, world, augment,
                         polar_stats_from(norm_stats[0], device) if polar else None)
        if rank == 0:
            val_data = loader(xv, yv, args.batch_size, False)
            if os.path.isfile(str(args.test_predictors_path)) and os.path.isfile(str(args.test_target_path)):
                xt, yt = load_pickled(args.test_predictors_path, args.test_target_path)
                xt = xt.to(device)
                print(normalize_dataset(args, xt))
                test_data = loader(xt, yt, 1, False)
                test_arrays = (xt, yt)
        if world > 1:
            say(f"data parallel on {world} ranks: {epoch_left_out(xs.shape[0], args.batch_size, world)} of {xs.shape[0]} "
                "samples per epoch left out (the last batch is cut to a multiple of the ranks)")

    model_dir = os.path.join(args.checkpoint_dir, model.model_name)
    os.makedirs(model_dir, exist_ok=True)
    state = {"step": 0, "worse_epochs": 0, "epochs": 0, "best_loss": np.inf, "best_epoch": 0, "best_test_epoch": 0}
    epoch = 0
    if args.load_model is not None and os.path.isfile(args.load_model):
        say("Continuing training full model from checkpoint " + str(args.load_model))
        state = load_model(model, optimizer, args.load_model, args.use_cuda, device, scheduler)
        epoch = state["epochs"]
    rotation = CheckpointRotation(model_dir, model.model_name, args.checkpoint_step, start_epoch=epoch)

    def eager_step(x, target):
        return train_step(model, optimizer, sync, x, target, loss_fn, n_out, args.sed_loss_weight, args.doa_loss_weight)

    runner = None
    if graph_step and any(graphable for _, _, graphable in tr_data.plan):
        # the constructor's warm-up steps TRAIN on the recorded batch: take them on the first rows of the array and put
        # weights, Adam state, BatchNorm buffers and the dropout stream back, so that step 1 of this run (or the step a
        # checkpoint resumes at) starts from the same state as without the recording
        model.train()
        snap = training_snapshot(model, optimizer)
        tr_data.fetch(batch=0)
        runner = GraphedTrainStep(model, optimizer, tr_data.x, tr_data.target, n_out, args.sed_loss_weight,
                                  args.doa_loss_weight, sync=sync, warmup=1, loader=tr_data, pit_overlaps=pit)
        training_restore(model, optimizer, snap)
    while (state["worse_epochs"] < args.patience or epoch < args.min_n_epochs) and not (args.epochs and epoch >= args.epochs):
        epoch += 1
        state["epochs"] += 1
        model.train()
        train_loss = 0.0
        t0 = time.time()
        steps_before = state["step"]
        if resident:
            tr_data.begin_epoch()
            for _, count, graphable in tr_data.plan:
                optimizer.lr_scale = warmup_scale(state["step"] + 1, warmup_steps)     # a replay takes it through _push_lr
                if runner is not None and graphable:
                    runner()                    # gather, step and running mean: one replay (three when data parallel)
                else:
                    # eager; a partial batch always (BatchNorm statistics depend on the true batch size)
                    tr_data.step_end(eager_step(*tr_data.fetch(count)))
                state["step"] += 1
                if args.max_steps and state["step"] >= args.max_steps:
                    break
            if world > 1:                       # every rank's mean is over its own shards: print the global batch's
                torch.distributed.all_reduce(tr_data.mean)
                tr_data.mean /= world
            train_loss = tr_data.mean.item()    # the epoch's one read-back
        else:
            for i, (x, target) in enumerate(tr_data):
                optimizer.lr_scale = warmup_scale(state["step"] + 1, warmup_steps)
                loss = eager_step(x.to(device), target.to(device))
                state["step"] += 1
                train_loss += (loss.detach() - train_loss) / (i + 1)
                if args.max_steps and state["step"] >= args.max_steps:
                    break
        if world > 1:
            DP.average_bn_running_stats(model)      # rank 0's validation and checkpoint speak for all ranks
        # one small read per epoch, next to the loss mean; every rank's statistics are the same (same averaged gradient)
        largest_norm, clipped = optimizer.clip_stats()
        with optimizer.ema_weights():       # --ema_decay: validation sees the moving average (nothing moves without it)
            val_loss = evaluate(model, device, criterion_sed, criterion_doa, val_data, args) if rank == 0 else None
        if scheduler is not None and optimizer.param_groups[0]['lr'] > args.min_lr:
            scheduler.step()
        if rank != 0:
            # validation, the test leg and the checkpoint files are rank 0's: wait for it and take over its verdict
            verdict = torch.zeros(1, device=device, dtype=torch.int64)
            torch.distributed.broadcast(verdict, 0)
            state["worse_epochs"] = int(verdict.item())
            if args.max_steps and state["step"] >= args.max_steps:
                break
            continue
        if history is not None:
            history.append((epoch, float(train_loss), val_loss))
        print(f"epoch {epoch}: train {float(train_loss):.5f} val {val_loss:.5f} lr {optimizer.param_groups[0]['lr']:.2e} "
              f"({time.time() - t0:.1f}s)"
              + (f" grad norm max {largest_norm:.3e} clipped {clipped / max(1, state['step'] - steps_before):.0%}"
                 if optimizer.clip is not None else ""))
        if rotation.end_of_epoch(model, optimizer, scheduler, state, epoch, val_loss, periodic_copy=False):
            print("MODEL IMPROVED ON VALIDATION SET!")
        if test_data is not None and args.test_step > 0 and epoch % args.test_step == 0:      # train.py:623-670
            path, at_epoch = rotation.test_checkpoint(args.test_mode)
            if path is not None:
                live = os.path.join(model_dir, "checkpoint")
                state = load_model(model, optimizer, path, args.use_cuda, device, scheduler)
                at_epoch = state['best_epoch'] if at_epoch is None else at_epoch
            # --ema_decay: the loaded checkpoint (or the live model) is scored under its moving average
            with optimizer.ema_weights():
                if ensemble is None:
                    results = evaluate_test(model, device, test_data, epoch=epoch if path is None else at_epoch,
                                            max_loc_value=args.max_loc_value, num_frames=args.num_frames,
                                            spatial_threshold=args.spatial_threshold, args=args)
                else:
                    results = evaluate_recordings(model, device, *test_arrays, args, epoch=epoch if path is None else at_epoch,
                                                  align=args.class_overlaps <= 3, max_loc_value=args.max_loc_value,
                                                  num_frames=args.num_frames, spatial_threshold=args.spatial_threshold,
                                                  **ensemble, **({} if post is None else dict(post=post)))
            rotation.after_test(model, optimizer, scheduler, state, epoch, results, args.test_mode)
            if path is not None:
                # the reference reloads args.load_model here (train.py:667), which only exists when resuming; the live
                # checkpoint of this epoch is what training must continue from
                best_test_epoch = state.get("best_test_epoch", 0)
                state = load_model(model, optimizer, live, args.use_cuda, device, scheduler)
                state["best_test_epoch"] = best_test_epoch      # set by after_test on the state loaded for the test
        rotation.periodic_copy(state, epoch)                    # after the test leg, as train.py:671-684
        if world > 1:
            torch.distributed.broadcast(torch.tensor([state["worse_epochs"]], device=device, dtype=torch.int64), 0)
        if args.max_steps and state["step"] >= args.max_steps:
            break
    return state


if __name__ == '__main__':
    args = parse_args(sys.argv[1:])
    main(args)
