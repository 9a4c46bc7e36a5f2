"""The training step: the loss, the one step sequence (three phases, an eager driver) and its recorded form."""
import numpy as np
import torch

from . import hip_ops as H


def seld_loss_fn(sed, doa, target, n_sed, sed_weight=1.0, doa_weight=5.0, pit_overlaps=0):
    """BCE(sed, target[..., :n_sed]) * sed_weight + MSE(doa, target[..., n_sed:]) * doa_weight, both means.
    pit_overlaps > 0 (--pit_loss): the same with, per (frame, class), the cheapest pairing of the pit_overlaps prediction
    slots with the target slots (hip_ops.seld_loss_pit); one launch either way."""
    assert target.shape[-1] == sed.shape[-1] + doa.shape[-1] and sed.shape[-1] == n_sed
    if pit_overlaps:
        return H.seld_loss_pit(sed, doa, target, pit_overlaps, sed_weight, doa_weight)
    return H.seld_loss(sed, doa, target, sed_weight, doa_weight)


# ---- the step sequence: three phases with the gradient exchange between them.  `train_step` runs them eagerly,
# GraphedTrainStep records them; nobody else spells a training step out.
#   a  [fetch] -> zero_grad -> forward -> loss -> backward, down to the front-end cut where there is one: afterwards the
#      main bucket's gradients are complete
#   b  the backward pass of the front end, which overlaps the main bucket's exchange; nothing without a cut
#   c  Adam on the (averaged) gradients [-> the loader's running mean and cursor]
# `cut`: the sync's dp.BackwardCut or None; `state`: the device-resident step state of a recording, None in an eager step;
# `loader`: a ResidentLoader whose gather and `step_end` are part of the step (recorded steps), or None
def phase_a(model, optimizer, cut, x, target, loss_fn, loss_args, state=None, loader=None):
    if loader is not None:
        loader.fetch()
    optimizer.zero_grad(state=state)
    if cut is not None:
        cut.reset()
    sed, doa = model(x)
    loss = loss_fn(sed, doa, target, *loss_args)
    H.backward_from_loss(loss)
    H.join_side_stream()
    return loss


def phase_b(cut):
    if cut is not None:
        cut.finish()
        H.join_side_stream()


def phase_c(optimizer, sync, state=None, loader=None, loss=None):
    optimizer.step(grad_scale=sync.average_scale() if sync is not None else 1.0, state=state)
    if loader is not None:
        loader.step_end(loss)


def train_step(model, optimizer, sync, x, target, loss_fn, *loss_args):
    """One eager training step, the canonical order: a -> all-reduce of the main bucket (asynchronous) -> b -> all-reduce
    of the late bucket, wait -> c.  `sync`: None (single process), a dp.BucketedGradSync, or a dp.FlatGradSync (no cut:
    one `all_reduce()` after the whole backward pass).  Returns `loss_fn(sed, doa, target, *loss_args)`, not detached."""
    cut = getattr(sync, "cut", None)
    loss = phase_a(model, optimizer, cut, x, target, loss_fn, loss_args)
    if hasattr(sync, "reduce_main"):
        sync.reduce_main()
        phase_b(cut)
        sync.reduce_late()
        sync.wait()
    elif sync is not None:
        sync.all_reduce()
    phase_c(optimizer, sync)
    return loss


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
    (phase_a / phase_b / phase_c above; `train_step` warms up).  More than one rank without a cut is refused: one graph.
    The batch is static: `__call__(x, target)` copies into the recorded input buffers (same shapes).

    `loader` (a ResidentLoader; default None: everything above): the recorded input buffers ARE the loader's batch
    buffers, the loader's gather is recorded as the first launch of the step and its `step_end` (running mean of the
    loss, cursor += 1) as the last, so `__call__()` with no arguments trains on the next batch of the epoch: an epoch
    is n replays with no host-to-device traffic.  `x` / `target` are then not copied (pass the loader's buffers).

    `pit_overlaps` (default 0: the slot-bound loss): as in seld_loss_fn; the permutation-invariant loss is one launch
    without a host read, so it is recorded like the plain one."""

    def __init__(self, model, optimizer, x, target, n_sed, sed_weight=1.0, doa_weight=5.0, sync=None, warmup=2, loader=None,
                 pit_overlaps=0):
        self.cut = getattr(sync, "cut", None)
        # the ranks `sync` averages over, from what it states itself: `world`, else 1 / average_scale() (dp.FlatGradSync
        # has no `world`); a sync that states neither is an AttributeError, never "one rank"
        ranks = 1 if sync is None else sync.world if hasattr(sync, "world") else round(1.0 / sync.average_scale())
        if ranks > 1 and self.cut is None:
            # one graph, replayed with no collective at all: the ranks would drift apart silently
            raise ValueError("GraphedTrainStep: a gradient exchange over more than one rank needs the front-end cut, the "
                             "place between two graphs where the collectives are issued: build the optimiser as "
                             "FlatAdam(..., late=dp.late_parameters(model)) and the exchange as BucketedGradSync(optimizer, model)")
        # model and loader are held for their memory: the graphs write BatchNorm buffers, cursor and mean through raw pointers
        self.model, self.opt, self.sync, self.loader = model, optimizer, sync, loader
        loss_args = (n_sed, float(sed_weight), float(doa_weight), int(pit_overlaps))
        if loader is None:
            self.x, self.target = x.clone(), target.clone()
        else:
            self.x, self.target = loader.x, loader.target
        self.state = H.philox.state(x.device)
        self._lr = None
        dev = x.device
        # eager warm-up on a side stream (allocator pools, kernel modules, host-side caches), as torch recommends
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(max(1, warmup)):
                train_step(model, optimizer, sync, self.x, self.target, seld_loss_fn, *loss_args)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        # the step state takes over from the host counters
        self.state[1] = self.opt.step_count
        self.state[0] = H.philox.offset
        self.state[3] = 0
        H.philox.offset = 0
        self._push_lr()
        H.hcq_weights.refresh_table()       # host-to-device copies of the weight-form table: not allowed while capturing
        ga = torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            self.loss = phase_a(model, optimizer, self.cut, self.x, self.target, seld_loss_fn, loss_args, self.state,
                                loader).detach()
            if self.cut is None:            # phase b is nothing then
                phase_c(optimizer, sync, self.state, loader, self.loss)
        self.graphs = [ga]
        if self.cut is not None:
            gb = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gb, pool=ga.pool()):
                phase_b(self.cut)
            gc_ = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gc_, pool=ga.pool()):
                phase_c(optimizer, sync, self.state, loader, self.loss)
            self.graphs += [gb, gc_]
        # the recording itself ran no kernel: undo its host-side bookkeeping, publish the draws per step
        self.state[3] = H.philox.offset
        H.philox.offset = 0
        self.replays, self._step_seen = 0, self.opt.step_count
        # the recorded weight-form launch reads the cache's table / block starts / form buffers through raw pointers:
        # hold them, the cache builds NEW tensors when a shape is registered later (hip_ops._HcqWeights.pin_for_graph)
        self._hcq_pinned = H.hcq_weights.pin_for_graph()

    def _push_lr(self):
        lr = float(self.opt.param_groups[0]["lr"]) * float(getattr(self.opt, "lr_scale", 1.0))      # StepLR's, times the warm-up's
        if lr != self._lr:
            self._lr = lr
            self.state[2] = int(np.float32(lr).view(np.uint32))

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
