"""The second HIP streams, created and forked onto here only: `side_queue` carries the weight gradients and the weight
re-layouts issued ahead of the data gradient, `branch_queue` the second of two branches (run_branches)."""
import contextlib
import os

import torch

from .. import _lib as L
from ._core import _req, deterministic
from .weight_forms import hcq_weights


class SideQueue:
    """One lazily created HIP stream beside the caller's."""

    def __init__(self):
        self._stream = None

    def stream(self):
        if self._stream is None:
            self._stream = torch.cuda.Stream()
        return self._stream

    @contextlib.contextmanager
    def fork(self, *reads):
        """Launches inside the block go to the queue, ordered after everything already on the current stream.  `reads`
        (None entries skipped) are read there: the caching allocator must not recycle them before the queue is done."""
        st = self.stream()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        st.wait_event(ev)
        with torch.cuda.stream(st):
            yield
        for t in reads:
            if t is not None:
                t.record_stream(st)

    def event(self):
        """An event behind everything issued on the queue so far."""
        ev = torch.cuda.Event()
        ev.record(self.stream())
        return ev


# ---- weight gradients on a second HIP stream -------------------------------------------------------------
# A layer's weight gradient and its data gradient both start from dy and are independent; the accumulating weight-
# gradient kernels write only FlatAdam's gradient slots.  Issued on a side stream they overlap the data gradient and
# the element-wise kernels that follow it on the main stream: a 70 us kernel on this GPU spends ~13 us ramping up and
# draining, which another queue fills (measured: two independent 1x3 convolutions 142 -> 121 us).  The main stream
# joins the side stream when the backward pass ends (autograd engine callback) and in FlatAdam.step().
class _WgradQueue(SideQueue):
    def __init__(self):
        super().__init__()
        self.dirty = False      # something was issued since the last join
        self.keep = []          # tensors the queue reads, referenced until the join (see _on_side_stream)

    def join(self):
        """Make the current stream wait for everything issued on the side stream."""
        if self.dirty:
            torch.cuda.current_stream().wait_event(self.event())
            self.dirty = False
        self.keep.clear()


side_queue = _WgradQueue()
branch_queue = SideQueue()
join_side_stream = side_queue.join


def _side_enabled():
    return os.environ.get("SELD_WGRAD_SIDE_STREAM", "1") != "0" and not deterministic()


def _on_side_stream(fn, *tensors):
    """Run `fn` (kernel launches only) on the side stream, ordered after everything already on the current stream.
    `tensors` are read there: the caching allocator must not recycle them before the side stream is done, and
    nothing on the main stream may overwrite them before the join.  The second point is about autograd: a backward
    that hands `dy` on as the gradient of an addend (HyperConvAddFn / HyperConvPairFn) gives the engine a tensor it
    accumulates into IN PLACE when it holds the only reference -- while the side stream may still be reading it.
    Holding a reference here until the join makes the engine accumulate out of place instead."""
    with side_queue.fork(*tensors):
        fn()
    side_queue.keep.extend(t for t in tensors if t is not None)
    if not side_queue.dirty:
        side_queue.dirty = True
        try:
            torch.autograd.Variable._execution_engine.queue_callback(join_side_stream)
        except RuntimeError:            # not inside a backward pass: join at once
            join_side_stream()


# ---- the two branches of the two-stream model on two queues --------------------------------------------------------
def two_queue_branches():
    """SELD_BRANCH_STREAMS=0 turns the second queue off (both branches then run one after the other on the caller's)."""
    return os.environ.get("SELD_BRANCH_STREAMS", "1") != "0"


def run_branches(fa, xa, fb, xb):
    """(fa(xa), fb(xb)) with fb on a second HIP stream.  Used for the two ConvTC blocks of the two-stream model
    (model.py:463-471: independent until their outputs are concatenated, and at 16 samples per GPU neither fills the
    device by itself) and for the SED / DOA classifier heads (model.py:473-480: two chains of small-grid kernels).
    Autograd replays each branch's backward on the stream its forward ran on and orders the streams at the fork and
    the join; the weight forms are packed BEFORE the fork (they are packed once per step, by whoever asks first)."""
    if not (xa.is_cuda and two_queue_branches()):
        return fa(xa), fb(xb)
    hcq_weights.ensure_packed()
    main = torch.cuda.current_stream()
    sb = branch_queue.stream()
    sb.wait_stream(main)             # not fork(): B is ordered behind what precedes the branches, not behind A
    xb.record_stream(sb)
    ya = fa(xa)                      # host order A, B as on one queue: the dropout counters are drawn in the same order
    with torch.cuda.stream(sb):
        yb = fb(xb)
    main.wait_stream(sb)
    yb.record_stream(main)
    return ya, yb


class FanOut2Fn(torch.autograd.Function):
    """x -> (x, x) for a tensor with two consumers (the SED and DOA heads, model.py:473-480): the sum of the two
    gradients is this library's add kernel on the consumer's stream instead of the autograd engine's ATen add."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None or gb is None:
            return ga if gb is None else gb
        ga, gb = _req(ga, "ga"), _req(gb, "gb")
        out = torch.empty_like(ga)
        L.check(L.lib().seld_add(L.ptr(ga), L.ptr(gb), ga.numel(), L.ptr(out), L.current_stream()), "seld_add")
        return out


def fan_out2(x):
    if not (x.is_cuda and x.requires_grad and torch.is_grad_enabled()):
        return x, x
    return FanOut2Fn.apply(x)
