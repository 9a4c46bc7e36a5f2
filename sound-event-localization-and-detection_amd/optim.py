"""FlatAdam (torch.optim.Adam over one flat buffer: one launch per step), StepLR and the learning-rate warm-up."""
import contextlib
import functools

import torch

from . import hip_ops as H


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
        steps = set()
        for pid, st in sd["state"].items():
            i = index_of[pid]
            p, o = self.params[i], self.offsets[i]
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


@functools.lru_cache(maxsize=None)
def _torch_adam_defaults():
    """Hyper-parameter keys of this torch version's Adam param group (amsgrad, foreach, capturable, ...)."""
    g = torch.optim.Adam([torch.zeros(1, requires_grad=True)]).param_groups[0]
    return {k: v for k, v in g.items() if k != "params"}


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


def warmup_scale(step, warmup_steps):
    """The learning-rate warm-up's factor for the 1-based `step`: min(1, step / warmup_steps); 1 without warm-up."""
    return min(1.0, step / warmup_steps) if warmup_steps > 0 else 1.0
