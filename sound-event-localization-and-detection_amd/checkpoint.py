"""Checkpoint files in the reference's format and the file rotation of its epoch loop."""
import os
import shutil

import numpy as np
import torch

from . import hip_ops as H


# ------------------------------------------------------------------------------------------
# checkpoints (train.py:26-81): same dictionary keys, `module.` prefixes stripped on load
# ------------------------------------------------------------------------------------------
def save_model(model, optimizer, state, path, scheduler=None):
    """train.py:26-45: same keys, same value layouts (state dicts of the model / Adam / StepLR, the loop state, the
    three RNG states), so either side reads the other's files."""
    sd = model.module.state_dict() if hasattr(model, "module") else model.state_dict()
    if len(os.path.dirname(path)) > 0 and not os.path.exists(os.path.dirname(path)):
        os.makedirs(os.path.dirname(path))
    ck = {'model_state_dict': sd, 'optimizer_state_dict': optimizer.state_dict() if optimizer is not None else None,
          'state': state}
    if scheduler is not None:
        ck['scheduler_state_dict'] = scheduler.state_dict()
    if getattr(optimizer, "ema", None) is not None:
        # --ema_decay: the moving average beside the training weights (model_state_dict stays those: a run resumes
        # exactly), keyed like the model's parameters.  Without the flag the file's keys are what they were
        target = model.module if hasattr(model, "module") else model
        ck['ema_state_dict'] = optimizer.ema_state_dict(target.named_parameters())
    # the reference's three RNG states (train.py:40-43, read back by index at :77-80) + a fourth entry it never looks at:
    # the position of the dropout kernels' counter-based RNG stream, so that a resumed run does not replay masks
    ck['random_states'] = (np.random.get_state(), torch.get_rng_state(),
                           torch.cuda.get_rng_state() if torch.cuda.is_available() else None,
                           {'seld_philox_offset': H.philox.get_offset()})
    torch.save(ck, path)


def load_model(model, optimizer, path, cuda, device, scheduler=None):
    """train.py:47-81: `module.` prefixes stripped, optimizer / scheduler restored when given, checkpoints that only
    hold `step` accepted, the numpy / torch / device RNG states restored.  An optimiser that keeps a moving average of
    the weights gets the file's `ema_state_dict` back, or, from a file without one, an average that starts at the loaded weights."""
    ck = torch.load(path, map_location=device if cuda else 'cpu', weights_only=False)
    sd = {(k[7:] if k.startswith('module.') else k): v for k, v in ck['model_state_dict'].items()}
    target = model.module if hasattr(model, "module") else model
    target.load_state_dict(sd)
    H.hcq_weights.weights_changed()          # the packed weight forms of the fast-product convolutions are stale now
    if optimizer is not None:
        optimizer.load_state_dict(ck['optimizer_state_dict'])
        if getattr(optimizer, "ema", None) is not None:
            # the file's moving average; a file without one (written without --ema_decay): the average starts from its weights
            optimizer.load_ema_state_dict(target.named_parameters(), ck.get('ema_state_dict') or {})
    if scheduler is not None:
        scheduler.load_state_dict(ck['scheduler_state_dict'])
    state = ck['state'] if 'state' in ck else {'step': ck['step']}
    rs = ck.get('random_states')
    if rs is not None:
        np.random.set_state(rs[0])
        torch.set_rng_state(rs[1].cpu())
        if torch.cuda.is_available() and rs[2] is not None:
            torch.cuda.set_rng_state(rs[2].cpu())
    extra = rs[3] if rs is not None and len(rs) > 3 and isinstance(rs[3], dict) else {}
    H.philox.set_offset(int(extra.get('seld_philox_offset', 0)))     # 0 for checkpoints written by the reference
    return state


class CheckpointRotation:
    """The file rotation of the reference's epoch loop (train.py:577-616, 671-684), same file names:

      <model_dir>/checkpoint                              every epoch
      <model_dir>/checkpoint_best_model                   when the validation loss improves
      <model_dir>/checkpoint_best_model_of_checkpoint     the previous best, kept when a new best arrives, or the best
                                                          epoch since that is not the overall best
      <model_dir>checkpoint_epoch_<E>/...                 every `checkpoint_step` epochs: copies of the above
                                                          (the reference concatenates without a separator: kept)

    `end_of_epoch` returns True when the epoch set a new best.  The test-set leg of the rotation
    (`checkpoint_best_model_on_Test`, train.py:623-668) belongs to the metrics row; files that do not
    exist are skipped by the periodic copy where the reference would stop with FileNotFoundError."""

    def __init__(self, model_dir, model_name, checkpoint_step, start_epoch=0):
        self.model_dir, self.model_name, self.checkpoint_step = model_dir, model_name, int(checkpoint_step)
        self.checkpoint_path = os.path.join(model_dir, "checkpoint")
        self.best_path = os.path.join(model_dir, "checkpoint_best_model")
        self.best_of_checkpoint_path = os.path.join(model_dir, "checkpoint_best_model_of_checkpoint")
        self.best_loss_checkpoint = np.inf
        self.best_epoch_checkpoint = start_epoch
        self.new_best = False
        self.best_test_metric = 1

    def end_of_epoch(self, model, optimizer, scheduler, state, epoch, val_loss, extra_files=(), periodic_copy=True):
        """Validation-loss bookkeeping and the per-epoch saves (train.py:588-616).  `periodic_copy=False` leaves the
        checkpoint_epoch_<E>/ copies to an explicit `periodic_copy()` call after the test leg (what `main` does)."""
        improved = not (val_loss >= state["best_loss"])
        if not improved:
            state["worse_epochs"] += 1
        else:
            if self.new_best:
                self.best_loss_checkpoint = state["best_loss"]
                self.best_epoch_checkpoint = state["best_epoch"]
                shutil.copyfile(self.best_path, self.best_of_checkpoint_path)
            state["worse_epochs"] = 0
            state["best_loss"] = val_loss
            state["best_epoch"] = epoch
            state["best_checkpoint"] = self.best_path
            self.new_best = True
            save_model(model, optimizer, state, self.best_path, scheduler)
        if val_loss < self.best_loss_checkpoint and (val_loss != state["best_loss"] or self.best_loss_checkpoint == np.inf):
            self.best_loss_checkpoint = val_loss
            save_model(model, optimizer, state, self.best_of_checkpoint_path, scheduler)
            self.best_epoch_checkpoint = epoch
        save_model(model, optimizer, state, self.checkpoint_path, scheduler)
        if periodic_copy:
            self.periodic_copy(state, epoch, extra_files)
        return improved

    def periodic_copy(self, state, epoch, extra_files=()):
        """train.py:671-684: every `checkpoint_step` epochs copy the rotation's files into checkpoint_epoch_<E>/.  The
        reference does this AFTER the test leg of the same epoch (train.py:623-670), so the copied
        checkpoint_best_model_on_Test and the `best_test_epoch` in its name are this epoch's."""
        if self.checkpoint_step > 0 and epoch % self.checkpoint_step == 0:
            d = self.model_dir + 'checkpoint_epoch_{}/'.format(epoch)
            os.makedirs(d, exist_ok=True)
            copies = [(self.best_path, "checkpoint_best_epoch_{}".format(state["best_epoch"])),
                      (self.checkpoint_path, "checkpoint_epoch_{}".format(epoch)),
                      (self.checkpoint_path + '_best_model_on_Test',
                       "checkpoint_best_model_on_Test_epoch_{}".format(state.get("best_test_epoch", 0))),
                      (self.best_of_checkpoint_path,
                       "checkpoint_best_model_checkpoint_epoch_{}".format(self.best_epoch_checkpoint))]
            copies += [(f, self.model_name + "_" + os.path.basename(f)) for f in extra_files]
            for src, name in copies:
                if os.path.isfile(src):
                    shutil.copyfile(src, d + name)

    def test_checkpoint(self, test_mode):
        """train.py:626-642: which checkpoint the test leg evaluates and the epoch it reports: the best model when this
        epoch set a new best, else the best-of-checkpoint model ('test_best' mode); the live model otherwise (None)."""
        if test_mode != 'test_best':
            return None, None
        if self.new_best:
            return self.best_path, None                 # epoch = state['best_epoch'] after loading
        return self.best_of_checkpoint_path, self.best_epoch_checkpoint

    def after_test(self, model, optimizer, scheduler, state, epoch, test_results, test_mode):
        """train.py:655-670: keep `checkpoint_best_model_on_Test` when the Global SELD score (entry 10 of the results)
        is not worse than the best seen, then clear the 'new best' flag.  Returns True when it saved."""
        saved = False
        if test_results[10] <= self.best_test_metric:
            self.best_test_metric = test_results[10]
            if test_mode == 'test_best':
                state["best_test_epoch"] = state["best_epoch"] if self.new_best else self.best_epoch_checkpoint
            else:
                state["best_test_epoch"] = epoch
            save_model(model, optimizer, state, self.checkpoint_path + '_best_model_on_Test', scheduler)
            saved = True
        self.new_best = False
        return saved
