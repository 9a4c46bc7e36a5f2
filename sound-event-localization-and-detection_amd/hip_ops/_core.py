"""What every kernel family's host glue shares: the launch timer, the scratch pools, the memo of library answers, the
kernel-label query and the argument checks.  Private to the package; `hip_ops` re-exports the public names."""
import collections
import ctypes
import functools
import os

import torch

from .. import _lib as L


class KernelTimer:
    """HIP-event timing of individual conv launches on the stream they are enqueued on (bench.py's roofline
    leg).  Inactive by default: then the wrappers below add nothing to the launch path."""

    def __init__(self):
        self.active = False
        self.only = None       # None: every conv launch; else the set of kernel labels to time (the others run bare)
        self.records = []      # (label, start_event, end_event, flops, bytes)

    def reset(self):
        self.records = []

    def summary(self):
        """label -> dict(calls, ms, flops, bytes); call after torch.cuda.synchronize()."""
        out = {}
        for label, e0, e1, fl, by in self.records:
            d = out.setdefault(label, dict(calls=0, ms=0.0, flops=0.0, bytes=0.0))
            d["calls"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += by
        return out


kernel_timer = KernelTimer()


class timed:
    """KernelTimer record of the launch(es) inside the `with` block.  label: the kernel label, or a callable that asks the
    library for it; work: callable returning (flops, bytes) of one call; mult: how many such calls the launch does.  With
    the timer inactive neither callable runs and no event is created: the launch path makes no library call for it.
    With `kernel_timer.only` set, a launch whose label is not in the set runs bare."""

    def __init__(self, label, work, mult=1):
        self.on = kernel_timer.active
        if self.on:
            self.label = label() if callable(label) else label
            self.on = kernel_timer.only is None or self.label in kernel_timer.only
        if self.on:
            self.work, self.mult = work, mult
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        if self.on:
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.e1.record()
            fl, by = self.work()
            kernel_timer.records.append((self.label, self.e0, self.e1, fl * self.mult, by * self.mult))
        return False


def kernel_label(fn, *args, size=64):
    """The label the library's query `fn(*args, buffer, size)` writes."""
    buf = ctypes.create_string_buffer(size)
    L.check(fn(*args, buf, size), fn.__name__)
    return buf.value.decode()


_memo_stores = []


def memo(fn):
    """Memoise a pure function of a descriptor (plus small hashable positional arguments) that the library answers.  The
    answers depend on the library's SELD_* switches: _lib.reload_env() drops every store registered here."""
    store = {}
    _memo_stores.append(store)

    @functools.wraps(fn)
    def cached(desc, *args):
        key = (bytes(desc), args)
        v = store.get(key)
        if v is None:
            v = store[key] = fn(desc, *args)
        return v
    return cached


def _drop_kernel_choice_caches():
    for store in _memo_stores:
        store.clear()


L._reload_hooks.append(_drop_kernel_choice_caches)


_scratch_pools = collections.defaultdict(dict)       # pool name -> {(device, stream): buffer}


def scratch(pool, nbytes, device):
    """At least `nbytes` of scratch (uint8, contents undefined: the kernels rewrite it fully per call) from the named
    pool's buffer of (device, current stream), grown by reallocation."""
    if torch.cuda.is_current_stream_capturing():
        # a recorded step: the scratch comes from (and stays in) the graph's own memory pool
        return torch.empty(nbytes, device=device, dtype=torch.uint8)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    t = _scratch_pools[pool].get(key)
    if t is None or t.numel() * t.element_size() < nbytes:
        t = torch.empty(nbytes, device=device, dtype=torch.uint8)
        _scratch_pools[pool][key] = t
    return t


def deterministic():
    """SELD_DETERMINISTIC=1: run-to-run reproducible training (include/seld_hip.h).  The library reads the switch itself
    (reductions in one ordered chain); here: BatchNorm statistics by seld_channel_stats instead of the convolution
    epilogues' atomics, weight gradients by the grouped kernels (no atomics) or seld_hc_conv_bwd_weight_det, no side
    stream.  Set it before the first library call (or call _lib.reload_env())."""
    return os.environ.get("SELD_DETERMINISTIC", "0") not in ("", "0")


def _req(t, name):
    if t is None:
        return None
    if not t.is_cuda:
        raise L.SeldHipError(f"{name}: expected a HIP device tensor (this package has no CPU path)")
    if t.dtype != torch.float32:
        raise L.SeldHipError(f"{name}: expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _pair(v):
    if isinstance(v, (tuple, list)):
        return (int(v[0]), int(v[1])) if len(v) == 2 else (1, int(v[0]))
    return (int(v), int(v))
