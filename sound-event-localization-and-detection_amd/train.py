"""Training harness with the CLI of the reference's train.py (`python train.py --TextArgs=config/X.txt`,
same flag names and defaults, train.py:719-818) and its step semantics (train.py:186-204, 498-508, 538-571):

    zero_grad -> forward -> BCELoss(sed) * w_sed + MSELoss(doa) * w_doa -> backward -> Adam(lr 1e-4)

on the gfx950 kernels: the loss is one fused kernel, Adam is ONE launch over a flat parameter buffer,
and under torch.distributed (one process per GPU, RCCL) the gradient exchange is ONE all-reduce of the
flat gradient buffer (the reference is single-device).

The reference's own `main()` cannot run on a current stack (np.Inf, StepLR(verbose=), wandb, ...);
this file restates its behaviour rather than its text.
"""
import argparse
import ast
import contextlib
import functools
import json
import os
import pickle
import shutil
import sys
import time

import numpy as np
import torch
import torch.nn as nn

from . import class_metrics as CM
from . import hip_ops as H
from .model import SE_MODES, SELD_Model, _at_check


# ------------------------------------------------------------------------------------------
# loss / optimiser
# ------------------------------------------------------------------------------------------
def seld_loss_fn(sed, doa, target, n_sed, sed_weight=1.0, doa_weight=5.0, pit_overlaps=0):
    """BCE(sed, target[..., :n_sed]) * sed_weight + MSE(doa, target[..., n_sed:]) * doa_weight, both means.
    pit_overlaps > 0 (--pit_loss): the same with, per (frame, class), the cheapest pairing of the pit_overlaps prediction
    slots with the target slots (hip_ops.seld_loss_pit); one launch either way."""
    assert target.shape[-1] == sed.shape[-1] + doa.shape[-1] and sed.shape[-1] == n_sed
    if pit_overlaps:
        return H.seld_loss_pit(sed, doa, target, pit_overlaps, sed_weight, doa_weight)
    return H.seld_loss(sed, doa, target, sed_weight, doa_weight)


def pit_overlaps_from_args(args):
    """class_overlaps under --pit_loss, else 0 (the slot-bound loss)."""
    return int(args.class_overlaps) if getattr(args, "pit_loss", False) else 0


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


class FlatAdam:
    """torch.optim.Adam semantics (train.py:502) with every parameter, gradient and moment living in one
    flat fp32 buffer each: `step()` is a single kernel launch and a data-parallel gradient exchange is a
    single all-reduce of `flat_grad` (see dp.py).  Parameters that never receive a gradient (SURVEY App. B:
    batch_gate1.*, the last block's conv2_residual) keep a zero gradient, which leaves them unchanged, as
    torch.optim.Adam does by skipping them."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, late=None, decoupled=False,
                 max_grad_norm=0.0, ema_decay=0.0):
        """`late`: parameters whose gradients are the LAST ones a backward pass completes (the front-end convolutions,
        see dp.late_parameters).  They are stored at the front of the flat buffers, so [0, late_numel) and
        [late_numel, total) are the two contiguous buckets of the data-parallel exchange (dp.BucketedGradSync: the big
        bucket is all-reduced while the front end's backward pass is still running).  `self.params`, the state dict
        and the relative order inside each bucket keep `model.parameters()` order.

        The extras, all off by default (then nothing below is allocated and `step()` is the launch it always was):
        `max_grad_norm` > 0: `step()` first launches hip_ops.grad_norm over `flat_grad` -- after the data-parallel
        exchange, so every rank computes the same norm from the same averaged gradient and no collective is added -- and
        the update multiplies the gradient by the coefficient that launch left in device memory (`clip`, 4 floats: norm,
        coefficient, largest norm and clipped steps since `clip_stats()`); nothing is read back, so a recorded step clips
        like an eager one.  `decoupled`: `weight_decay` shrinks the weights as torch.optim.AdamW does instead of joining
        the gradient.  `ema_decay` > 0: the flat buffer `ema` follows the weights inside the update's launch,
        ema <- d ema + (1 - d) p with d = min(ema_decay, (1 + step) / (10 + step)); `ema_weights()` lends it to the model."""
        if not max_grad_norm >= 0.0:
            raise ValueError(f"FlatAdam: max_grad_norm must not be negative (0: no clipping), got {max_grad_norm!r}")
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"FlatAdam: ema_decay must lie in [0, 1) (0: no moving average), got {ema_decay!r}")
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("FlatAdam: no parameters")
        dev = self.params[0].device
        total = sum(p.numel() for p in self.params)
        late_ids = {id(p) for p in (late or ())}
        storage = [p for p in self.params if id(p) in late_ids] + [p for p in self.params if id(p) not in late_ids]
        self.late_numel = sum(p.numel() for p in self.params if id(p) in late_ids)
        self.flat_param = torch.empty(total, device=dev, dtype=torch.float32)
        self.flat_grad = torch.zeros(total, device=dev, dtype=torch.float32)
        self.exp_avg = torch.zeros(total, device=dev, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(total, device=dev, dtype=torch.float32)
        self._offset = {}
        off = 0
        with torch.no_grad():
            for p in storage:
                n = p.numel()
                self._offset[id(p)] = off
                self.flat_param[off:off + n].copy_(p.data.reshape(-1))
                p.data = self.flat_param[off:off + n].view(p.shape)
                p.grad = self.flat_grad[off:off + n].view(p.shape)
                p._seld_direct_grad = True      # HIP backward kernels accumulate straight into this view
                p._seld_owner = self            # ... and may reduce into a slot that is still zero (grad_generation)
                off += n
        self.offsets = [self._offset[id(p)] for p in self.params]      # flat offset of params[i]
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, params=self.params)]
        self.step_count = 0
        self.grad_generation = 0
        self.lr_scale = 1.0         # the learning-rate warm-up's factor (main, --warmup_steps): host side, on top of "lr"
        self.decoupled, self.max_grad_norm, self.ema_decay = bool(decoupled), float(max_grad_norm), float(ema_decay)
        self.clip = torch.zeros(4, device=dev, dtype=torch.float32) if self.max_grad_norm > 0 else None
        self.ema = self.flat_param.clone() if self.ema_decay > 0 else None
        self._extras = self.decoupled or self.clip is not None or self.ema is not None
        self._ema_lent = False

    def zero_grad(self, set_to_none=False, state=None):
        """`state`: the device-resident step state (hip_ops.philox.state): also advance it (graph-recorded steps)."""
        H.deferred_wgrads.discard()                  # jobs of a backward pass nobody finished would add into the fresh buffer
        if self.flat_grad.is_cuda:
            H.step_begin(self.flat_grad, state)      # one launch: zero fill (+ step state)
        else:
            self.flat_grad.zero_()
        self.grad_generation += 1       # every slot is zero again (hip_ops._claim_grad_slots)
        for p, off in zip(self.params, self.offsets):           # re-attach views if something replaced .grad
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * off:
                p.grad = self.flat_grad[off:off + p.numel()].view(p.shape)

    def step(self, grad_scale=1.0, state=None):
        """`state`: take the step number and the learning rate from the device-resident step state instead of the
        host's (graph-recorded steps; GraphedTrainStep keeps the host's count in step and `sync_from_host` pushes host-side
        changes -- eager steps, a restored optimiser -- back into the state before the next replay)."""
        H.deferred_wgrads.flush()       # grouped weight gradients still pending (a backward pass outside the autograd engine)
        H.join_side_stream()            # weight gradients issued on the side stream (hip_ops._on_side_stream)
        H.hcq_weights.weights_changed() # the packed weight forms of the fast-product convolutions are stale now
        g = self.param_groups[0]
        if self._extras:
            return self._step_ex(g, grad_scale, state)
        if state is not None:
            H.adam_flat_step_state(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, state, g["betas"][0],
                                   g["betas"][1], g["eps"], g["weight_decay"], grad_scale)
            return
        self.step_count += 1
        H.adam_flat_step(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.step_count,
                         g["lr"] * self.lr_scale, g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], grad_scale)

    def _step_ex(self, g, grad_scale, state):
        """The step with any of the extras on: the norm launch (clipping only), then the extended update."""
        if self._ema_lent:
            raise RuntimeError("FlatAdam.step() inside ema_weights(): the parameters hold the moving average")
        if self.clip is not None:
            H.grad_norm(self.flat_grad, grad_scale, self.max_grad_norm, self.clip)
        extras = dict(decoupled=self.decoupled, clip=self.clip, ema=self.ema, ema_decay=self.ema_decay)
        if state is not None:
            H.adam_flat_step_state_ex(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, state, g["betas"][0],
                                      g["betas"][1], g["eps"], g["weight_decay"], grad_scale, **extras)
            return
        self.step_count += 1
        H.adam_flat_step_ex(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.step_count,
                            g["lr"] * self.lr_scale, g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], grad_scale,
                            **extras)

    def ema_reset(self):
        """The moving average starts (again) from the weights as they are now: after a broadcast of the parameters, after
        loading a checkpoint that carries no average."""
        if self.ema is not None:
            self.ema.copy_(self.flat_param)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model computes with the moving average: the contents of `flat_param` and `ema` are
        exchanged (the parameters are views of `flat_param`) and exchanged back on the way out, also when the body raised.
        The packed weight forms of the fast-product convolutions are marked stale both times.  BatchNorm buffers are
        not parameters: both sets of weights see the same running statistics.  No average (ema_decay == 0): nothing moves."""
        if self.ema is None:
            yield self
            return
        if self._ema_lent:
            raise RuntimeError("FlatAdam.ema_weights() does not nest")
        self._swap_ema()
        self._ema_lent = True
        try:
            yield self
        finally:
            self._swap_ema()
            self._ema_lent = False

    def _swap_ema(self):
        with torch.no_grad():
            held = self.flat_param.clone()
            self.flat_param.copy_(self.ema)
            self.ema.copy_(held)
        H.hcq_weights.weights_changed()

    def clip_stats(self):
        """(largest gradient norm, clipped steps) since the last call, read from the device and zeroed there: one small
        read, for the epoch line.  (0.0, 0) without clipping."""
        if self.clip is None:
            return 0.0, 0
        largest, clipped = self.clip[2:].tolist()
        self.clip[2:].zero_()
        return float(largest), int(clipped)

    def ema_state_dict(self, named_parameters):
        """{name: the moving average of that parameter} for the checkpoint, keyed like the model's parameters."""
        return {name: self.ema[self._offset[id(p)]:self._offset[id(p)] + p.numel()].view(p.shape).clone()
                for name, p in named_parameters if id(p) in self._offset}

    def load_ema_state_dict(self, named_parameters, sd):
        """Restore `ema_state_dict`'s tensors; a parameter the file does not name starts from its weights."""
        self.ema_reset()
        for name, p in named_parameters:
            if id(p) in self._offset and name in sd:
                if tuple(sd[name].shape) != tuple(p.shape):
                    raise ValueError(f"moving average of {name}: shape {tuple(sd[name].shape)} != {tuple(p.shape)}")
                off = self._offset[id(p)]
                self.ema[off:off + p.numel()].copy_(sd[name].reshape(-1))

    def state_dict(self):
        """torch.optim.Adam's layout (the reference saves `optimizer.state_dict()`, train.py:36): per-parameter
        `step / exp_avg / exp_avg_sq` keyed by the parameter's index in `model.parameters()` order plus one
        param group with torch's hyper-parameter keys, so the reference's `load_model` accepts our checkpoints.
        Every parameter gets an entry once a step was taken (torch omits parameters that never had a gradient;
        an extra entry is ignored by torch for as long as the parameter has no gradient)."""
        state = {}
        if self.step_count > 0:
            for i, (p, off) in enumerate(zip(self.params, self.offsets)):
                n = p.numel()
                state[i] = dict(step=torch.tensor(float(self.step_count)),
                                exp_avg=self.exp_avg[off:off + n].view(p.shape).clone(),
                                exp_avg_sq=self.exp_avg_sq[off:off + n].view(p.shape).clone())
        group = dict(_torch_adam_defaults())
        group.update({k: v for k, v in self.param_groups[0].items() if k != "params"})
        group["params"] = list(range(len(self.params)))
        return dict(state=state, param_groups=[group])

    def load_state_dict(self, sd):
        """Accepts torch.optim.Adam's layout (reference checkpoints) and this class's round-1 flat layout."""
        H.hcq_weights.weights_changed()      # a restore usually comes with new weights: never serve forms from before it
        if "exp_avg" in sd:                                   # flat layout
            self.step_count = int(sd["step"])
            self.exp_avg.copy_(sd["exp_avg"])
            self.exp_avg_sq.copy_(sd["exp_avg_sq"])
            self.param_groups[0].update(sd["param_groups"][0])
            return
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError("loaded state dict has a different number of parameter groups / parameters")
        index_of = {pid: i for i, pid in enumerate(groups[0]["params"])}
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        offsets = self.offsets
        steps = set()
        for pid, st in sd["state"].items():
            i = index_of[pid]
            p, o = self.params[i], offsets[i]
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError(f"optimizer state of parameter {i}: shape {tuple(st['exp_avg'].shape)} != {tuple(p.shape)}")
            self.exp_avg[o:o + p.numel()].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + p.numel()].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): not a checkpoint of one Adam over the model")
        self.step_count = steps.pop() if steps else 0
        for k in ("lr", "betas", "eps", "weight_decay", "initial_lr"):
            if k in groups[0]:
                self.param_groups[0][k] = tuple(groups[0][k]) if k == "betas" else groups[0][k]
        if groups[0].get("amsgrad") or groups[0].get("maximize"):
            raise ValueError("amsgrad / maximize checkpoints are not supported (the reference never sets them)")


class GraphedTrainStep:
    """One training step -- zero_grad -> forward -> BCE + w*MSE -> backward -> [gradient exchange] -> Adam
    (train.py:552-560) -- recorded ONCE as HIP graphs and replayed: ~400 kernel launches on two streams become one
    host call, so the step costs what its kernels cost and nothing of the Python / autograd / ctypes time between them
    (at 16 samples per GPU the eager step is host-bound).  Nothing is traced or compiled: the recorded launches are the
    same C-ABI calls the eager step makes.

    What a replay must not freeze is kept in device memory and read by the kernels: the Philox base of the dropout
    masks, the optimiser's step number and the learning rate (the 4-word step state of seld_step_begin), and, with
    gradient clipping, the clip coefficient (FlatAdam.clip, written by the norm launch and read by Adam's).

    Single process: one graph.  Data parallel (`sync` = dp.BucketedGradSync): three graphs with the two collectives
    issued eagerly between them, so that no collective is ever captured:
        A  zero_grad, forward, loss, backward down to the front-end cut    -> all-reduce of the big bucket (async)
        B  backward of the front-end convolutions (overlaps that all-reduce) -> all-reduce of the late bucket
        C  Adam on the averaged gradients
    The batch is static: `__call__(x, target)` copies into the recorded input buffers (same shapes).

    `loader` (a ResidentLoader; default None: everything above): the recorded input buffers ARE the loader's batch
    buffers, the loader's gather is recorded as the first launch of the step and its `step_end` (running mean of the
    loss, cursor += 1) as the last, so `__call__()` with no arguments trains on the next batch of the epoch: an epoch
    is n replays with no host-to-device traffic.  `x` / `target` are then not copied (pass the loader's buffers).

    `pit_overlaps` (default 0: the slot-bound loss): as in seld_loss_fn; the permutation-invariant loss is one launch
    without a host read, so it is recorded like the plain one."""

    def __init__(self, model, optimizer, x, target, n_sed, sed_weight=1.0, doa_weight=5.0, sync=None, warmup=2, loader=None,
                 pit_overlaps=0):
        self.model, self.opt, self.sync, self.loader = model, optimizer, sync, loader
        self.n_sed, self.w, self.pit_overlaps = n_sed, (float(sed_weight), float(doa_weight)), int(pit_overlaps)
        if loader is None:
            self.x, self.target = x.clone(), target.clone()
        else:
            self.x, self.target = loader.x, loader.target
        self.state = H.philox.state(x.device)
        self.cut = sync.cut if (sync is not None and getattr(sync, "cut", None) is not None and sync.world > 1) else None
        self._lr = None
        dev = x.device
        # eager warm-up on a side stream (allocator pools, kernel modules, host-side caches), as torch recommends
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(max(1, warmup)):
                self._eager()
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        # the step state takes over from the host counters
        self.state[1] = self.opt.step_count
        self.state[0] = H.philox.offset
        self.state[3] = 0
        H.philox.offset = 0
        self._push_lr()
        H.hcq_weights.refresh_table()       # host-to-device copies of the weight-form table: not allowed while capturing
        self.graphs = []
        ga = torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            self.loss = self._phase_a()
            if self.cut is None:
                self._phase_b()
                self._phase_c()
        self.graphs.append(ga)
        if self.cut is not None:
            gb = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gb, pool=ga.pool()):
                self._phase_b()
            gc_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gc_, pool=ga.pool()):
                self._phase_c()
            self.graphs += [gb, gc_]
        # the recording itself ran no kernel: undo its host-side bookkeeping, publish the draws per step
        self.state[3] = H.philox.offset
        H.philox.offset = 0
        self.replays = 0
        self._step_seen = self.opt.step_count
        # the recorded weight-form launch reads the cache's table / block starts / form buffers through raw pointers:
        # hold them, the cache builds NEW tensors when a shape is registered later (hip_ops._HcqWeights.pin_for_graph)
        self._hcq_pinned = H.hcq_weights.pin_for_graph()

    def _push_lr(self):
        lr = float(self.opt.param_groups[0]["lr"]) * float(getattr(self.opt, "lr_scale", 1.0))      # StepLR's, times the warm-up's
        if lr != self._lr:
            self._lr = lr
            self.state[2] = int(np.float32(lr).view(np.uint32))

    def _eager(self):
        self.opt.zero_grad()
        if self.cut is not None:
            self.cut.reset()
        sed, doa = self.model(self.x)
        loss = seld_loss_fn(sed, doa, self.target, self.n_sed, *self.w, self.pit_overlaps)
        H.backward_from_loss(loss)
        if self.cut is not None:
            self.cut.finish()
        H.join_side_stream()
        if self.sync is not None:
            self.sync.reduce_main()
            self.sync.reduce_late()
            self.sync.wait()
        self.opt.step(grad_scale=self.sync.average_scale() if self.sync is not None else 1.0)
        return loss

    def _phase_a(self):
        if self.loader is not None:
            self.loader.fetch()
        self.opt.zero_grad(state=self.state)
        if self.cut is not None:
            self.cut.reset()
        sed, doa = self.model(self.x)
        loss = seld_loss_fn(sed, doa, self.target, self.n_sed, *self.w, self.pit_overlaps)
        H.backward_from_loss(loss)
        H.join_side_stream()
        return loss.detach()

    def _phase_b(self):
        if self.cut is not None:
            self.cut.finish()
            H.join_side_stream()

    def _phase_c(self):
        self.opt.step(grad_scale=self.sync.average_scale() if self.sync is not None else 1.0, state=self.state)
        if self.loader is not None:
            self.loader.step_end(self.loss)

    def __call__(self, x=None, target=None):
        if x is not None:
            self.x.copy_(x, non_blocking=True)
        if target is not None:
            self.target.copy_(target, non_blocking=True)
        self._push_lr()
        self.sync_from_host()
        self.graphs[0].replay()
        if self.cut is not None:
            self.sync.reduce_main()
            self.graphs[1].replay()
            self.sync.reduce_late()
            self.sync.wait()
            self.graphs[2].replay()
        self.replays += 1
        self.opt.step_count += 1
        self._step_seen = self.opt.step_count
        # the replayed Adam step rewrote the weights behind the host cache's back: an eager forward after this (validation,
        # an instrumented step) must re-pack the fast-product weight forms
        H.hcq_weights.weights_changed()
        return self.loss

    def sync_from_host(self):
        """Bring the device-resident step state up to date with what happened on the host between replays: eager steps
        or `optimizer.load_state_dict` moved the step count; eager dropout draws moved the host Philox offset (a replay's
        own draws are recorded with offsets from 0 on top of the device base, which the step itself advances)."""
        if self.opt.step_count != self._step_seen:
            self.state[1] = self.opt.step_count
            self._step_seen = self.opt.step_count
        if H.philox.offset:
            self.state[0] += int(H.philox.offset)
            H.philox.offset = 0


_ADAM_DEFAULTS = None


def _torch_adam_defaults():
    """Hyper-parameter keys of this torch version's Adam param group (amsgrad, foreach, capturable, ...)."""
    global _ADAM_DEFAULTS
    if _ADAM_DEFAULTS is None:
        g = torch.optim.Adam([torch.zeros(1, requires_grad=True)]).param_groups[0]
        _ADAM_DEFAULTS = {k: v for k, v in g.items() if k != "params"}
    return _ADAM_DEFAULTS


class StepLR:
    """torch.optim.lr_scheduler.StepLR(step_size, gamma) for FlatAdam (train.py:505-508, 570-571)."""

    def __init__(self, optimizer, step_size, gamma=0.1):
        self.opt, self.step_size, self.gamma = optimizer, step_size, gamma
        self.base_lr = optimizer.param_groups[0].setdefault("initial_lr", optimizer.param_groups[0]["lr"])   # as torch does
        self.last_epoch = 0

    def step(self):
        self.last_epoch += 1
        self.opt.param_groups[0]["lr"] = self.base_lr * self.gamma ** (self.last_epoch // self.step_size)

    def state_dict(self):
        """torch.optim.lr_scheduler.StepLR's keys (train.py:37 saves `scheduler.state_dict()`)."""
        return dict(step_size=self.step_size, gamma=self.gamma, base_lrs=[self.base_lr], last_epoch=self.last_epoch,
                    _step_count=self.last_epoch + 1, _get_lr_called_within_step=False,
                    _last_lr=[self.opt.param_groups[0]["lr"]])

    def load_state_dict(self, sd):
        self.step_size, self.gamma, self.last_epoch = sd["step_size"], sd["gamma"], sd["last_epoch"]
        self.base_lr = sd["base_lrs"][0] if "base_lrs" in sd else sd["base_lr"]


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
# waveform and stay refused
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
          ('augment_mix', float, 0.), ('augment_mix_gain_lo', float, 0.5), ('augment_mix_gain_hi', float, 1.0)]


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


def warmup_scale(step, warmup_steps):
    """The learning-rate warm-up's factor for the 1-based `step`: min(1, step / warmup_steps); 1 without warm-up."""
    return min(1.0, step / warmup_steps) if warmup_steps > 0 else 1.0


def model_from_args(args):
    """train.py:448-465, plus the squeeze-and-excitation and temporal-attention flags."""
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
                      **at_from_args(args))


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
        if not hasattr(self, "best_test_metric"):
            self.best_test_metric = 1
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


def training_snapshot(model, optimizer):
    """Everything a training step changes: weights, Adam moments and step count, every module buffer (BatchNorm running
    statistics, num_batches_tracked), the position of the dropout RNG stream and, where the optimiser keeps them, the
    moving average of the weights and the clip statistics."""
    snap = dict(param=optimizer.flat_param.clone(), exp_avg=optimizer.exp_avg.clone(), exp_avg_sq=optimizer.exp_avg_sq.clone(),
                step=optimizer.step_count, buffers=[b.clone() for b in model.buffers()], philox=H.philox.get_offset())
    for key in ("ema", "clip"):         # the moving average and the clip statistics, where the optimiser keeps them
        if getattr(optimizer, key, None) is not None:
            snap[key] = getattr(optimizer, key).clone()
    return snap


def training_restore(model, optimizer, snap):
    """Put back a `training_snapshot`, in place (recorded launches keep pointing at the same memory).  After
    GraphedTrainStep's constructor, whose warm-up steps train: the run then starts from where it stood before."""
    with torch.no_grad():
        optimizer.flat_param.copy_(snap["param"])
        optimizer.exp_avg.copy_(snap["exp_avg"])
        optimizer.exp_avg_sq.copy_(snap["exp_avg_sq"])
        for b, saved in zip(model.buffers(), snap["buffers"]):
            b.copy_(saved)
        for key in ("ema", "clip"):
            if key in snap:
                getattr(optimizer, key).copy_(snap[key])
    optimizer.step_count = snap["step"]         # GraphedTrainStep.sync_from_host pushes it into the step state
    H.philox.set_offset(snap["philox"])
    H.hcq_weights.weights_changed()


_NORM_OFF = {'False', 'false', 'None', 'none'}
_NORM_UNIT = {'DQ_Normalization', 'UnitNormNormalization', 'UnitNorm'}
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


def polar_stats_from(entry, device):
    """What ResidentLoader(polar_stats=...) takes, from the entry normalize_dataset(..., stats=[]) reports for the training
    array: the fp32 device tensor (mean_m, sd_m, mean_p, sd_p) of a standardised magnitude-phase array, None for a raw one."""
    if entry is None:
        return None
    if len(entry) != 2:
        raise ValueError("--augment_rotate on magnitude-phase predictors needs the statistics of both halves (--phase=True)")
    return torch.cat([e.reshape(2).to(device=device, dtype=torch.float32) for e in entry]).contiguous()


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


def class_report_from_args(args):
    """(report, average) of the --class_report / --metrics_average flags; an args object without them counts as (False,
    'micro').  Every refusal comes before the device is touched."""
    report, average = getattr(args, "class_report", False), getattr(args, "metrics_average", "micro")
    if not isinstance(report, (bool, int)):
        raise ValueError(f"--class_report is True or False, got {report!r}")
    if average not in ("micro", "macro"):
        raise ValueError(f"--metrics_average is micro or macro, got {average!r}")
    return bool(report), average


def _results_from_table(counters, total_de, epoch):
    """The 16 results from row "all" of a breakdown table (numpy, all recordings)."""
    all_c, all_de = CM.totals(counters, total_de)
    counts = dict(zip(H.METRIC_COUNTERS, all_c[-1].tolist()))
    return test_results_from_counters(counts, float(all_de[-1]), epoch)


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
    output_classes = args.output_classes if args is not None else 14
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
            if by:
                tables.append(H.metrics_accumulate_by(sed, doa, target.to(device), num_frames, 14, class_overlaps, max_loc_value,
                                                      spatial_threshold, doa_threshold))
            else:
                H.metrics_accumulate(acc, sed, doa, target.to(device), num_frames, 14, class_overlaps, max_loc_value,
                                     spatial_threshold, doa_threshold)
    if by:
        return _report_results(tables, epoch, args, report, average)
    counts = dict(zip(H.METRIC_COUNTERS, acc[0].cpu().tolist()))
    results = test_results_from_counters(counts, float(acc[1].item()), epoch)
    _print_test_results(results)
    return results


def _report_results(tables, epoch, args, report, average):
    """The close of a test leg that scored with metrics_accumulate_by: one read-back of the tables, the 16 results, the report."""
    counters = torch.cat([t[0] for t in tables]).cpu().numpy()
    total_de = torch.cat([t[1] for t in tables]).cpu().numpy()
    results = _results_from_table(counters, total_de, epoch)
    _print_test_results(results)
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
        table = H.metrics_accumulate_by(sed, doa, y_all.to(device), num_frames, 14, args.class_overlaps, max_loc_value,
                                        spatial_threshold, args.Dcase21_metrics_DOA_threshold)
        return _report_results([table], epoch, args, report, average)
    acc = H.metrics_new(device)
    for r in range(sed.shape[0]):                       # one recording per launch, as evaluate_test's loader gives them
        H.metrics_accumulate(acc, sed[r:r + 1], doa[r:r + 1], y_all[r:r + 1].to(device), num_frames, 14, args.class_overlaps,
                             max_loc_value, spatial_threshold, args.Dcase21_metrics_DOA_threshold)
    counts = dict(zip(H.METRIC_COUNTERS, acc[0].cpu().tolist()))
    results = test_results_from_counters(counts, float(acc[1].item()), epoch)
    _print_test_results(results)
    return results


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
    """The reference's training loop.  --resident_loader / --graph_step: see _EXTRA.  Started under
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
    # bound once: the data-parallel step and the recorded step take the loss the eager step and `evaluate` reach through
    # seld_loss(..., args)
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
        if sync is not None:
            return DP.dp_train_step(model, optimizer, sync, x, target, n_out, loss_fn, args.sed_loss_weight,
                                    args.doa_loss_weight)
        optimizer.zero_grad()
        loss = seld_loss(x, target, model, criterion_sed, criterion_doa, args)
        loss.backward()
        optimizer.step()
        return loss.detach()

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
                optimizer.zero_grad()
                loss = seld_loss(x.to(device), target.to(device), model, criterion_sed, criterion_doa, args)
                loss.backward()
                optimizer.step()
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
