"""Data: synthetic batches, the pickled arrays, the epoch plan, the device-resident loader, dataset normalisation."""
import pickle

import numpy as np
import torch

from . import hip_ops as H
from .cli import _NORM_OFF, _NORM_UNIT


# ------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------
def synthetic_batch(batch, channels, freq, time, n_out, seed, device):
    """x ~ N(0,1); target = [Bernoulli(0.1) (B, T/8, n_sed) | U(-1,1) (B, T/8, 3 n_sed)]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, channels, freq, time, generator=g)
    sed = (torch.rand(batch, time // 8, n_out, generator=g) < 0.1).float()
    doa = torch.rand(batch, time // 8, 3 * n_out, generator=g) * 2 - 1
    return x.to(device), torch.cat((sed, doa), 2).to(device)


def load_pickled(pred_path, target_path):
    with open(pred_path, 'rb') as f:
        x = np.array(pickle.load(f))
    with open(target_path, 'rb') as f:
        y = np.array(pickle.load(f))
    return torch.tensor(x).float(), torch.tensor(y).float()


def epoch_plan(n, batch_size, world=1):
    """The minibatches of one epoch over n samples as (start, count_per_rank, graphable) triples: the batch covers
    positions [start, start + world * count_per_rank) of the epoch's sample order and rank r takes
    `rank_rows(start, count_per_rank, r)` of them.  `batch_size` is the GLOBAL batch.  Full batches are graphable (they
    have the recorded shape); the last one may be partial, as with the reference's drop_last=False, and is then cut
    down to the largest multiple of `world` (fewer than `world` samples of the epoch are left out; a batch cut to
    nothing is dropped)."""
    n, batch_size, world = int(n), int(batch_size), int(world)
    if n <= 0 or batch_size <= 0 or world <= 0:
        raise ValueError(f"epoch_plan: n, batch_size and world must be positive, got {n}, {batch_size}, {world}")
    if batch_size % world:
        raise ValueError(f"global batch {batch_size} is not divisible by world size {world}")
    per = batch_size // world
    plan = [(start, per, True) for start in range(0, n - batch_size + 1, batch_size)]
    rest = (n % batch_size) // world
    if rest:
        plan.append((n - n % batch_size, rest, False))
    return plan


def rank_rows(start, count_per_rank, rank):
    """(first, last + 1) positions of the epoch's sample order that `rank` takes of the batch `(start, count_per_rank, _)`."""
    return start + rank * count_per_rank, start + (rank + 1) * count_per_rank


def epoch_left_out(n, batch_size, world=1):
    """Samples per epoch that `epoch_plan` leaves out (always fewer than `world`)."""
    return n - sum(world * c for _, c, _ in epoch_plan(n, batch_size, world))


class ResidentLoader:
    """What `DataLoader(TensorDataset(x_all, y_all), batch_size, shuffle)` does for arrays that are resident in HBM, on
    the device: predictors AND targets live there, one permutation per epoch goes up as a single copy of n int64, and a
    batch is ONE launch (hip_ops.gather_rows) into the static buffers `x` / `target`.  Which batch is next is the device
    int32 `cursor`; `step_end(loss)` folds the loss into the device fp32 `mean` (the epoch loop's running mean) and
    advances the cursor, so a recorded step (GraphedTrainStep(loader=...)) walks through the epoch by itself.

    Sample order and RNG consumption are the DataLoader's: every epoch draws the iterator's base seed and, with
    shuffle, the RandomSampler's seed from torch's default generator, so a run with this loader visits the samples in
    the order a run with the DataLoader visits them.  Data parallel: `batch_size` is the global batch, this rank
    gathers its `rank_rows` of every batch; rank 0's order is broadcast, so ranks agree whatever their RNG state.

    `augment` (a hip_ops.Augment; default None: exactly the launches above): every fetch is hip_ops.gather_rows_aug, or
    hip_ops.gather_rows_rot when its p_rot > 0, still one launch.  What a sample draws depends on (`seed`, the device int32 `epoch`, its position in the epoch's order):
    ranks need no agreement, and a recorded fetch draws anew in every epoch.  `epoch` is -1 until the first
    `begin_epoch`, which adds 1 to it.  An `augment` with rot_polar and p_rot > 0 (magnitude-phase predictors) fetches
    with hip_ops.gather_rows_polar; `polar_stats` is then the fp32 device tensor (mean_m, sd_m, mean_p, sd_p) with which
    `x_all` was standardised (`polar_stats_from`), None for raw magnitude and phase.  An `augment` with p_mix > 0 fetches
    with hip_ops.gather_rows_mix: `overlaps` is the number of track slots per class of the targets, `polar_stats` means
    what it means above, and the occupancy table of the targets (hip_ops.target_occupancy) is computed here, once."""

    def __init__(self, x_all, y_all, batch_size, shuffle, rank=0, world=1, augment=None, seed=0, polar_stats=None, overlaps=None):
        self.plan = epoch_plan(x_all.shape[0], batch_size, world)
        if y_all.shape[0] != x_all.shape[0]:
            raise ValueError(f"ResidentLoader: {x_all.shape[0]} predictors but {y_all.shape[0]} targets")
        dev = x_all.device
        self.x_all, self.y_all = x_all.contiguous(), y_all.to(dev).contiguous()
        self.n, self.batch_size, self.shuffle, self.rank, self.world = x_all.shape[0], int(batch_size), bool(shuffle), rank, world
        per = self.batch_size // world
        self.x = torch.zeros((per,) + tuple(x_all.shape[1:]), device=dev, dtype=torch.float32)
        self.target = torch.zeros((per,) + tuple(y_all.shape[1:]), device=dev, dtype=torch.float32)
        self.index = torch.arange(self.n, device=dev, dtype=torch.int64)
        self.cursor = torch.zeros(1, device=dev, dtype=torch.int32)
        self.mean = torch.zeros(1, device=dev, dtype=torch.float32)
        self.epoch = torch.full((1,), -1, device=dev, dtype=torch.int32)
        self.augment, self.seed, self.polar_stats = augment, int(seed), polar_stats
        self.overlaps = self.occupancy = None
        if augment is not None and augment.kind == "mix":
            if overlaps is None:
                raise ValueError("ResidentLoader: an augment that mixes clips needs `overlaps`, the track slots per class of the targets")
            self.overlaps = int(overlaps)
            self.occupancy = H.target_occupancy(self.y_all, self.overlaps)

    def __len__(self):
        return len(self.plan)

    def begin_epoch(self):
        """New sample order (outside any capture), cursor and mean back to zero, the epoch number one up."""
        torch.empty((), dtype=torch.int64).random_()           # the base seed a DataLoader iterator draws first
        if self.shuffle:
            self.index.copy_(H.epoch_permutation(self.n))
            if self.world > 1:
                torch.distributed.broadcast(self.index, 0)
        self.cursor.zero_()
        self.mean.zero_()
        self.epoch += 1

    def fetch(self, count=None, batch=None):
        """Gather this rank's rows of a batch into `x` / `target` and return the views of the rows that were written.
        batch None: the batch the device cursor points at (recordable); else that batch of the plan, whatever the cursor."""
        count = self.x.shape[0] if count is None else count
        if batch is None:
            where = dict(cursor=self.cursor, start=self.rank * count, count=count, stride=self.batch_size)
        else:
            where = dict(start=rank_rows(self.plan[batch][0], count, self.rank)[0], count=count)
        if self.augment is None:
            H.gather_rows(self.x_all, self.y_all, self.index, self.x, self.target, **where)
        else:
            kind = self.augment.kind
            gather = {"swap": H.gather_rows_aug, "rot": H.gather_rows_rot, "polar": H.gather_rows_polar, "mix": H.gather_rows_mix}[kind]
            own = dict(stats=self.polar_stats) if kind == "polar" else {}
            if kind == "mix":
                own = dict(stats=self.polar_stats, overlaps=self.overlaps, occupancy=self.occupancy)
            gather(self.x_all, self.y_all, self.index, self.x, self.target, epoch=self.epoch, seed=self.seed, augment=self.augment,
                   **own, **where)
        return self.x[:count], self.target[:count]

    def step_end(self, loss):
        H.epoch_step_end(loss, self.mean, self.cursor)

    def __iter__(self):
        """One epoch as (x, target) batches, like the DataLoader (evaluation loops).  The batches are views of the static
        buffers: each is valid until the next one is taken."""
        self.begin_epoch()
        for i, (_, count, _) in enumerate(self.plan):
            yield self.fetch(count, batch=i)


_DOMAIN_DQ = ['DQ', 'dq', 'dQ', 'Dual_Quaternion', 'dual_quaternion']


def normalize_dataset(args, *predictors, stats=None):
    """Dataset normalisation of train.py:242-408, in place on device-resident predictor arrays
    (items, channels, F, T) - the reference's training / validation / test predictors, each normalised with its
    OWN statistics as the reference does.  Returns the description the reference appends to `dataset_string`.

      off ('False' / 'None')                        -> untouched
      'UnitNorm' family, 2 mics, DQ domain          -> unit dual quaternion per position (train.py:257-308);
                                                       with --phase the reference raises ValueError (train.py:310)
      'UnitNorm' family otherwise                   -> untouched (the reference has no branch for it)
      anything else ('True')                        -> (g - mean) / std over the magnitude channels
                                                       (first 4 for 1 mic, first 8 for 2 mics) and, with --phase,
                                                       separately over the remaining channels (train.py:341-405)

    `stats`: a list that receives one entry per predictor array, in order: the (mean, std) device tensors of the groups
    `group_standardize_` applied to it (one, or two with --phase), or None where the array was left raw or got another
    normalisation (what ResidentLoader(polar_stats=...) wants to know of the training array).
    """
    desc, entries = _normalize_dataset(args, predictors)
    if stats is not None:
        stats.extend(entries)
    return desc


def _normalize_dataset(args, predictors):
    """(description, [what normalize_dataset reports per array])."""
    untouched = [None] * len(predictors)
    mode = str(args.dataset_normalization)
    if mode in _NORM_OFF:
        return '', untouched
    if mode in _NORM_UNIT:
        if args.n_mics == 2 and args.domain in _DOMAIN_DQ:
            if args.phase:
                raise ValueError('DATASET NORMALIZATION FOR PHASE DUAL QUATERNION NOT YET IMPLEMENTED')
            for x in predictors:
                H.dq_unit_norm_(x)
            return ' Dataset Normalization for 2Mic 8Ch Magnitude Dual Quaternion UnitNorm', untouched
        return '', untouched
    if args.n_mics not in (1, 2):
        return '', untouched
    mag = 4 * args.n_mics
    entries = []
    for x in predictors:
        applied = [H.group_standardize_(x, 0, mag)]
        if args.phase:
            applied.append(H.group_standardize_(x, mag, x.shape[1]))
        entries.append(tuple(applied))
    what = f'{args.n_mics}Mic {mag}Ch Magnitude'
    desc = ' Dataset Normalization for ' + what
    if args.phase:
        desc += f' Dataset Normalization for {args.n_mics}Mic {2 * mag}Ch Magnitude-Phase'
    return desc, entries


def polar_stats_from(entry, device):
    """What ResidentLoader(polar_stats=...) takes, from the entry normalize_dataset(..., stats=[]) reports for the training
    array: the fp32 device tensor (mean_m, sd_m, mean_p, sd_p) of a standardised magnitude-phase array, None for a raw one."""
    if entry is None:
        return None
    if len(entry) != 2:
        raise ValueError("--augment_rotate on magnitude-phase predictors needs the statistics of both halves (--phase=True)")
    return torch.cat([e.reshape(2).to(device=device, dtype=torch.float32) for e in entry]).contiguous()
