"""2-D / 1-D hypercomplex convolution (csrc/hc_conv*.hip, csrc/hcq_*.hip): descriptors, the three entry points, the packed
weight forms of the fast-product kernels, grouped / deferred / side-stream weight gradients, and the autograd functions."""
import ctypes
import os

import torch

from .. import _lib as L
from ._core import _pair, _req, deterministic, kernel_label, memo, scratch, timed
from .conv3d import HyperConv3dFn
from .norm_act import _direct_targets, _ncs, channel_stats


def conv_work(desc, which):
    """Algorithmic flops / bytes of one conv call: x and y once, COMPONENT weights once, structured
    flops (48 of 64 blocks for the dual quaternion, all 16 for the quaternion).  which: 0 fwd, 1 dgrad, 2 wgrad."""
    A = desc.algebra
    o = conv_out_shape(desc)
    s_in = desc.in_[0] * desc.in_[1]
    s_out = o[0] * o[1]
    K = desc.k[0] * desc.k[1]
    nb = {1: 1, 4: 16, 8: 48}[A]
    blk = (desc.Cout // A) * (desc.Cin // A)
    flops = 2.0 * desc.N * s_out * K * nb * blk
    by = 4.0 * (desc.N * desc.Cin * s_in + desc.N * desc.Cout * s_out + A * blk * K)
    return flops, by


@memo
def _label(desc, which):
    return kernel_label(L.lib().seld_hc_conv_kernel_label, ctypes.byref(desc), which)


def _timed(desc, which, mult=1, variant=False, label=None):
    """KernelTimer record (_core.timed) of one launch of conv_work(desc, which), `mult` of them in one for the pair forms.
    variant: the launch runs the kernel's other instantiation (pair data gradient, fused first-stage weight gradient): its
    symbol ends in ', 1>' instead of ', 0>'.  label: the kernel symbol, or a callable for it, when the caller knows it
    (the fast-product kernels)."""
    def conv_label():
        lab = _label(desc, which)
        if (variant or (mult == 2 and which == 1)) and lab.endswith(", 0>"):
            lab = lab[:-4] + ", 1>"
        return lab
    return timed(label if label is not None else conv_label, lambda: conv_work(desc, which), mult)


def make_conv_desc(x_shape, cout, algebra, kernel, stride, padding, dilation, groups=1):
    """x_shape: (N, C, T) or (N, C, H, W).  kernel/stride/padding/dilation: int or tuple."""
    d = L.ConvDesc()
    nd = len(x_shape) - 2
    if nd not in (1, 2):
        raise Exception("The convolutional input is either 3, 4 or 5 dimensions. input.dim = " + str(len(x_shape)))
    d.algebra, d.ndim, d.N, d.Cin, d.Cout, d.groups = algebra, nd, x_shape[0], x_shape[1], cout, groups

    def two(v):
        if nd == 1:
            v = v[0] if isinstance(v, (tuple, list)) else v
            return (1, int(v))
        return _pair(v)
    if nd == 1:
        d.in_[0], d.in_[1] = 1, x_shape[2]
        k = two(kernel); s = two(stride); p = (0, two(padding)[1]); dl = two(dilation)
    else:
        d.in_[0], d.in_[1] = x_shape[2], x_shape[3]
        k = two(kernel); s = two(stride); p = two(padding); dl = two(dilation)
    for i in range(2):
        d.k[i], d.stride[i], d.pad[i], d.dil[i] = k[i], s[i], p[i], dl[i]
    return d


def conv_out_shape(desc):
    out = (ctypes.c_int32 * 2)()
    L.check(L.lib().seld_hc_conv_out_shape(ctypes.byref(desc), out), "seld_hc_conv_out_shape")
    return out[0], out[1]


def _y_shape(desc, o):
    return (desc.N, desc.Cout, o[1]) if desc.ndim == 1 else (desc.N, desc.Cout, o[0], o[1])


def conv_fwd(desc, x, ws, bias=None, out=None, epilogue=0, addend=None, stats=None):
    x = _req(x, "x")
    ws = [_req(w, "w") for w in ws]
    bias = _req(bias, "bias")
    o = conv_out_shape(desc)
    y = out if out is not None else torch.empty(_y_shape(desc, o), device=x.device, dtype=torch.float32)
    if stats is not None and deterministic():
        # statistics by one ordered reduction per channel instead of the epilogue's float atomics
        y = conv_fwd(desc, x, ws, bias, out=y, epilogue=epilogue & ~L.SELD_EPI_STATS, addend=addend, stats=None)
        channel_stats(y, out=stats)
        return y
    wp = hcq_weights.get(desc, 0, ws) if desc.algebra > 1 else None
    if wp is not None:                      # 8-multiplication Hamilton product (csrc/hcq_conv.hip)
        with _timed(desc, 0, label=lambda: hcq_label(desc, 0, 1)):
            hcq_conv(desc, 0, x, wp, (y,), (bias,), (epilogue,), (_req(addend, "addend"),), (stats,))
        return y
    with _timed(desc, 0):
        L.check(L.lib().seld_hc_conv_fwd_ex(ctypes.byref(desc), L.ptr(x), L.ptr_array8(ws), L.ptr(bias), L.ptr(y),
                                            epilogue, L.ptr(_req(addend, "addend")), L.ptr(stats),
                                            L.current_stream()), "seld_hc_conv_fwd")
    return y


def conv_bwd_data(desc, dy, ws, x_shape, ahead=None):
    """`ahead`: (workspace, event) from _transpose_ahead -- the weights are already re-laid out."""
    dy = _req(dy, "dy")
    dx = torch.empty(x_shape, device=dy.device, dtype=torch.float32)
    lib = L.lib()
    wp = hcq_weights.get(desc, 1, ws) if desc.algebra > 1 else None
    if wp is not None:
        with _timed(desc, 1, label=lambda: hcq_label(desc, 1, 1)):
            hcq_conv(desc, 1, dy, wp, (dx,))
        return dx
    if ahead is not None:
        wt, ev = ahead
        torch.cuda.current_stream().wait_event(ev)
        with _timed(desc, 1):
            L.check(lib.seld_hc_conv_bwd_data_wt(ctypes.byref(desc), L.ptr(dy), L.ptr(wt), L.ptr(dx), L.current_stream()),
                    "seld_hc_conv_bwd_data_wt")
        return dx
    ws = [_req(w, "w") for w in ws]
    nbytes = lib.seld_hc_conv_bwd_data_workspace(ctypes.byref(desc))
    wsb = torch.empty((nbytes + 3) // 4, device=dy.device, dtype=torch.float32)
    with _timed(desc, 1):
        L.check(lib.seld_hc_conv_bwd_data_ex(ctypes.byref(desc), L.ptr(dy), L.ptr_array8(ws), L.ptr(dx), L.ptr(wsb),
                                             nbytes, L.current_stream()), "seld_hc_conv_bwd_data")
    return dx


def _hcq_wgrad_ok(desc, npair=1):
    if deterministic():
        return False
    return _hcq_wgrad_taken(desc, npair)


@memo
def _hcq_wgrad_taken(desc, npair):
    return desc.algebra > 1 and (_hcq_wgrad_row_bytes(desc, npair) > 0 or
                                 bool(L.lib().seld_hcq_wgrad_supported(ctypes.byref(desc), int(npair))))


@memo
def _hcq_wgrad_label(desc, npair=1):
    return kernel_label(L.lib().seld_hcq_wgrad_label, ctypes.byref(desc), int(npair), size=96)


@memo
def _hcq_wgrad_row_bytes(desc, npair=1):
    """Scratch bytes of the 24-product dual-quaternion weight gradient (csrc/hcq_wgrad_row.hip), 0 = shape not taken."""
    return int(L.lib().seld_hcq_wgrad_row_workspace(ctypes.byref(desc), int(npair))) if desc.algebra == 8 else 0


@memo
def _hcq_wgrad_row_label(desc, npair=1):
    return kernel_label(L.lib().seld_hcq_wgrad_row_label, ctypes.byref(desc), int(npair), size=96)


def hcq_wgrad_acc(desc, x, dyA, dwA, dyB=None, dwB=None):
    """dwA[c] += wgrad(x, dyA) [, dwB[c] += wgrad(x, dyB)] on the fast-product kernels: the row-chunk GEMM on forms for
    the dual quaternion (seld_hcq_wgrad_row_acc), else seld_hcq_wgrad_acc."""
    npair = 2 if dyB is not None else 1
    nbytes = _hcq_wgrad_row_bytes(desc, npair)
    if nbytes:
        ws = scratch("wgrad_row", nbytes, x.device, zeroed=True)       # every call hands it back zeroed
        with _timed(desc, 2, npair, label=lambda: _hcq_wgrad_row_label(desc, npair)):
            L.check(L.lib().seld_hcq_wgrad_row_acc(ctypes.byref(desc), npair, L.ptr(x), L.ptr(dyA), L.ptr(dyB),
                                                   L.ptr_array8(dwA), L.ptr_array8(dwB) if dwB is not None else None,
                                                   L.ptr(ws), ws.numel() * 4, L.current_stream()),
                    "seld_hcq_wgrad_row_acc")
        return
    with _timed(desc, 2, npair, label=lambda: _hcq_wgrad_label(desc, npair)):
        L.check(L.lib().seld_hcq_wgrad_acc(ctypes.byref(desc), npair, L.ptr(x), L.ptr(dyA), L.ptr(dyB), L.ptr_array8(dwA),
                                           L.ptr_array8(dwB) if dwB is not None else None, L.current_stream()),
                "seld_hcq_wgrad_acc")


# ---- grouped weight gradients (csrc/hcq_wgrad_grp.hip) -----------------------------------------------------------------
def wgrad_group_jobs(jobs):
    """ctypes array of seld_wgrad_job from [(desc, x, dy, [8 gradient tensors]), ...]."""
    arr = (L.WgradJob * len(jobs))()
    for a, (desc, x, dy, dws) in zip(arr, jobs):
        ctypes.memmove(ctypes.byref(a.desc), ctypes.byref(desc), ctypes.sizeof(L.ConvDesc))
        a.x, a.dy = x.data_ptr(), dy.data_ptr()
        for i in range(8):
            a.dw[i] = dws[i].data_ptr()
    return arr


def wgrad_group_bytes(jobs_arr):
    """Scratch bytes of a grouped call, 0 when one of the jobs is not a shape the grouped kernels take."""
    return int(L.lib().seld_hcq_wgrad_group_workspace(jobs_arr, len(jobs_arr)))


def wgrad_group(jobs):
    """dw[c] += weight gradient for every (desc, x, dy, dws) of `jobs` -- dual-quaternion convolutions of the shape
    families of seld_hcq_wgrad_group -- in one persistent launch per family.  Returns False (nothing launched) when a job
    is not taken.  Deterministic: no atomics, fixed summation order."""
    arr = wgrad_group_jobs(jobs)
    nbytes = wgrad_group_bytes(arr)
    if nbytes == 0:
        return False
    dev = jobs[0][1].device
    ws = scratch("wgrad_group", nbytes, dev)
    L.check(L.lib().seld_hcq_wgrad_group(arr, len(arr), L.ptr(ws), ws.numel(), L.current_stream()),
            "seld_hcq_wgrad_group")
    return True


@memo
def wgrad_group_family(desc):
    """Shape family (0..3) of `desc` in the grouped kernels, -1 = not taken (cached)."""
    return int(L.lib().seld_hcq_wgrad_group_family(ctypes.byref(desc)))


class _DeferredWgrads:
    """Weight gradients the backward pass does NOT launch where autograd reaches them: the dual-quaternion layers of the
    TCN and of the 3x3 stages are collected -- (desc, x, dy, gradient slots), the tensors kept alive -- and issued as ONE
    grouped call (seld_hcq_wgrad_group: one persistent launch per shape family) when the backward pass ends, i.e. before
    anything reads the gradient buffer (data-parallel exchange, Adam).  Why: a workgroup that keeps a layer's whole output
    tile in registers needs hundreds of positions to amortise it, and one layer spread over 256 CUs has 64
    (csrc/hcq_wgrad_grp.hip).  SELD_WGRAD_GROUP=0 restores the per-layer launches on the side stream.

    Families deferred: 0 (192 -> 384 1x3), 1 (384 -> 192 1x1), 2 (192 -> 192 3x3); family 3 (384 -> 384 1x3, tcn.conv2) is
    three steps per workgroup at its size and stays on the per-layer kernels."""
    FAMILIES = (0, 1, 2)

    def __init__(self):
        self.jobs = []
        self.armed = False

    @staticmethod
    def enabled():
        return os.environ.get("SELD_WGRAD_GROUP", "1") != "0"

    def takes(self, desc):
        if desc.algebra != 8 or not self.enabled():
            return False
        fam = wgrad_group_family(desc)
        return fam in self.FAMILIES or (fam == 3 and deterministic())        # the grouped kernels have no atomics

    def add(self, desc, x, dy, dws):
        # the stream this backward node runs on produced dy (branch B of the two-stream model runs on its own queue)
        self.jobs.append((desc, x, dy, list(dws), torch.cuda.current_stream(x.device)))
        if not self.armed:
            self.armed = True
            try:
                torch.autograd.Variable._execution_engine.queue_callback(self.flush)
            except RuntimeError:            # not inside a backward pass: issue at once
                self.flush()

    def flush(self):
        self.armed = False
        jobs, self.jobs = self.jobs, []
        if not jobs:
            return
        here = torch.cuda.current_stream(jobs[0][1].device)
        for st in {j[4] for j in jobs}:
            if st != here:
                here.wait_stream(st)
                for _, x, dy, _, st_ in jobs:
                    if st_ == st:
                        x.record_stream(here)
                        dy.record_stream(here)
        jobs = [j[:4] for j in jobs]
        def work():
            fl = by = 0.0
            for desc, _, _, _ in jobs:
                f_, b_ = conv_work(desc, 2)
                fl, by = fl + f_, by + b_
            return fl, by
        with timed("hcq_wgrad_grp_kernel", work) as grouped:
            if not wgrad_group(jobs):        # cannot happen for jobs `takes` accepted; never lose a gradient to it
                grouped.on = False           # the per-layer launches record themselves
                for desc, x, dy, dws in jobs:
                    conv_bwd_weight(desc, x, dy, tuple(dws[0].shape), False, into=dws)

    def discard(self):
        self.jobs, self.armed = [], False


deferred_wgrads = _DeferredWgrads()


def conv_bwd_weight(desc, x, dy, w_shape, want_bias, into=None, bias_into=None):
    """Component weight gradients.  `into` (list of A tensors, e.g. views of FlatAdam.flat_grad) selects the
    accumulating entry point: the kernel adds straight into them and nothing is returned for autograd."""
    x = _req(x, "x")
    dy = _req(dy, "dy")
    if deterministic():
        lib = L.lib()
        nbytes = int(lib.seld_hc_conv_bwd_weight_det_workspace(ctypes.byref(desc)))
        wsb = torch.empty(max(nbytes, 16), device=x.device, dtype=torch.uint8)
        dws = into if into is not None else [torch.zeros(w_shape, device=x.device, dtype=torch.float32) for _ in range(desc.algebra)]
        dbias = bias_into if bias_into is not None else (torch.zeros(desc.Cout, device=x.device, dtype=torch.float32) if want_bias else None)
        with _timed(desc, 2):
            L.check(lib.seld_hc_conv_bwd_weight_det(ctypes.byref(desc), L.ptr(x), L.ptr(dy), L.ptr_array8(dws),
                                                    L.ptr(dbias), L.ptr(wsb), wsb.numel(), L.current_stream()),
                    "seld_hc_conv_bwd_weight_det")
        return (None, None) if into is not None else (dws, dbias)
    if not want_bias and bias_into is None and _hcq_wgrad_ok(desc):
        if into is not None:
            hcq_wgrad_acc(desc, x, dy, into)
            return None, None
        dws = [torch.zeros(w_shape, device=x.device, dtype=torch.float32) for _ in range(desc.algebra)]
        hcq_wgrad_acc(desc, x, dy, dws)
        return dws, None
    if into is not None:
        with _timed(desc, 2):
            L.check(L.lib().seld_hc_conv_bwd_weight_acc(ctypes.byref(desc), L.ptr(x), L.ptr(dy), L.ptr_array8(into),
                                                        L.ptr(bias_into), L.current_stream()),
                    "seld_hc_conv_bwd_weight_acc")
        return None, None
    dws = [torch.empty(w_shape, device=x.device, dtype=torch.float32) for _ in range(desc.algebra)]
    dbias = torch.empty(desc.Cout, device=x.device, dtype=torch.float32) if want_bias else None
    with _timed(desc, 2):
        L.check(L.lib().seld_hc_conv_bwd_weight(ctypes.byref(desc), L.ptr(x), L.ptr(dy), L.ptr_array8(dws),
                                                L.ptr(dbias), None, 0, L.current_stream()),
                "seld_hc_conv_bwd_weight")
    return dws, dbias


@memo
def _hcq_ok(desc, mode, npair=1):
    """Does the fast-product kernel take this (shape, direction)?  (cached; no weights needed)"""
    return desc.algebra > 1 and hcq_pack_floats(desc, mode, npair) > 0


def stacked_conv_weight(params):
    """ONE convolution weight (sum of the Cout's, Cin, k...) over parameters that lie back to back in memory -- FlatAdam
    re-homes a model's parameters into one flat buffer in registration order, so the attention's values / keys / queries
    (model.py:18-20) are three consecutive row blocks of it -- or None.  With gradients enabled the gradient slots must be
    adjacent in the same order too: the stacked weight is a fresh leaf over the same storage whose gradient the backward
    kernels write straight into those slots (`_direct_targets`), so autograd never sees the member parameters."""
    p0 = params[0]
    need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    at = p0.data_ptr()
    for p in params:
        if p.data_ptr() != at or not p.is_contiguous() or p.shape[1:] != p0.shape[1:] or p.dtype != torch.float32:
            return None
        at += 4 * p.numel()
    shape = (sum(int(p.shape[0]) for p in params),) + tuple(p0.shape[1:])
    same_buffer = lambda ts: all(t.untyped_storage().data_ptr() == ts[0].untyped_storage().data_ptr() for t in ts)
    if not same_buffer(params):                     # neighbours by accident of the allocator: not one tensor's memory
        return None
    gview = None
    if need_grad:
        if not all(getattr(p, "_seld_direct_grad", False) and p.grad is not None and p.requires_grad for p in params):
            return None
        if not same_buffer([p.grad for p in params]):
            return None
        gat = p0.grad.data_ptr()
        for p in params:
            if p.grad.data_ptr() != gat or not p.grad.is_contiguous():
                return None
            gat += 4 * p.numel()
        gview = p0.grad.as_strided(shape, p0.grad.stride())
    w = p0.detach().as_strided(shape, p0.stride())
    if need_grad:
        w.requires_grad_(True)
        w._seld_base_param = p0
        w._seld_grad = gview
    return w


def as_conv_weight(param, shape):
    """A contiguous reshape of a parameter used as a convolution weight (the attention's Linear applied as a 1x1
    convolution, model.py:46): the view remembers its parameter, so the backward kernels write that parameter's gradient
    slot directly instead of returning a tensor for autograd to add to it."""
    w = param.view(shape)
    w._seld_base_param = param
    return w


# ---- weight gradients on a second HIP stream -------------------------------------------------------------
# A layer's weight gradient and its data gradient both start from dy and are independent; the accumulating weight-
# gradient kernels write only FlatAdam's gradient slots.  Issued on a side stream they overlap the data gradient and
# the element-wise kernels that follow it on the main stream: a 70 us kernel on this GPU spends ~13 us ramping up and
# draining, which another queue fills (measured: two independent 1x3 convolutions 142 -> 121 us).  The main stream
# joins the side stream when the backward pass ends (autograd engine callback) and in FlatAdam.step().
_side = {"stream": None, "dirty": False, "keep": []}


def _side_enabled():
    return os.environ.get("SELD_WGRAD_SIDE_STREAM", "1") != "0" and not deterministic()


def join_side_stream():
    """Make the current stream wait for everything issued on the side stream."""
    if _side["dirty"]:
        ev = torch.cuda.Event()
        ev.record(_side["stream"])
        torch.cuda.current_stream().wait_event(ev)
        _side["dirty"] = False
    _side["keep"].clear()


def _on_side_stream(fn, *tensors):
    """Run `fn` (kernel launches only) on the side stream, ordered after everything already on the current stream.
    `tensors` are read there: the caching allocator must not recycle them before the side stream is done, and
    nothing on the main stream may overwrite them before the join.  The second point is about autograd: a backward
    that hands `dy` on as the gradient of an addend (HyperConvAddFn / HyperConvPairFn) gives the engine a tensor it
    accumulates into IN PLACE when it holds the only reference -- while the side stream may still be reading it.
    Holding a reference here until the join makes the engine accumulate out of place instead."""
    if _side["stream"] is None:
        _side["stream"] = torch.cuda.Stream()
    st = _side["stream"]
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    st.wait_event(ev)
    with torch.cuda.stream(st):
        fn()
    for t in tensors:
        if t is not None:
            t.record_stream(st)
            _side["keep"].append(t)
    if not _side["dirty"]:
        _side["dirty"] = True
        try:
            torch.autograd.Variable._execution_engine.queue_callback(join_side_stream)
        except RuntimeError:            # not inside a backward pass: join at once
            join_side_stream()


def _transpose_ahead(desc, ws):
    """The data gradient's weight re-layout (seld_hc_conv_transpose_weights), issued NOW on the side stream -- i.e. during
    the forward pass, where it overlaps the convolution -- instead of in front of the data-gradient kernel on the critical
    path of the backward pass (47 launches of ~5 us per step).  Returns (workspace tensor, event) or None."""
    if not _side_enabled() or not torch.is_grad_enabled() or _hcq_ok(desc, 1):
        return None
    lib = L.lib()
    nbytes = lib.seld_hc_conv_bwd_data_workspace(ctypes.byref(desc))
    wt = torch.empty((nbytes + 3) // 4, device=ws[0].device, dtype=torch.float32)
    if _side["stream"] is None:
        _side["stream"] = torch.cuda.Stream()
    st = _side["stream"]
    ev0 = torch.cuda.Event()
    ev0.record(torch.cuda.current_stream())
    st.wait_event(ev0)                                   # the weights may still be in flight (Adam of the last step)
    with torch.cuda.stream(st):
        L.check(lib.seld_hc_conv_transpose_weights(ctypes.byref(desc), L.ptr_array8([_req(w, "w") for w in ws]),
                                                   L.ptr(wt), nbytes, L.current_stream()),
                "seld_hc_conv_transpose_weights")
        ev = torch.cuda.Event()
        ev.record(st)
    wt.record_stream(st)
    return wt, ev


def _conv_backward(ctx, dy, first_w):
    x = ctx.saved_tensors[0]
    ws = ctx.w_params
    dy = _req(dy, "dy")
    dws, dbias = [None] * len(ws), None
    need_w = any(ctx.needs_input_grad[first_w:]) or (ctx.has_bias and ctx.needs_input_grad[1])
    direct = _direct_targets(ws, ctx.bias_param) if need_w else None
    if direct is not None and direct[1] is None and deferred_wgrads.takes(ctx.desc):
        deferred_wgrads.add(ctx.desc, x, dy, direct[0])          # issued with the other layers' when the backward pass ends
        need_w = False
    elif direct is not None and _side_enabled() and ctx.needs_input_grad[0]:
        _on_side_stream(lambda: conv_bwd_weight(ctx.desc, x, dy, tuple(ws[0].shape), ctx.has_bias, into=direct[0],
                                                bias_into=direct[1]), x, dy)
        need_w = False
    dx = conv_bwd_data(ctx.desc, dy, ws, tuple(x.shape), getattr(ctx, "wt_ahead", None)) if ctx.needs_input_grad[0] else None
    if need_w:
        if direct is not None:
            conv_bwd_weight(ctx.desc, x, dy, tuple(ws[0].shape), ctx.has_bias, into=direct[0], bias_into=direct[1])
        else:
            dws, dbias = conv_bwd_weight(ctx.desc, x, dy, tuple(ws[0].shape), ctx.has_bias)
    return dx, dbias, dws


class HyperConvFn(torch.autograd.Function):
    """y = W (x) x  for algebra 1/4/8; replaces quaternion_conv / dual_quaternion_conv / F.convNd."""

    @staticmethod
    def forward(ctx, x, bias, stride, padding, dilation, *ws):
        algebra = len(ws)
        k = tuple(ws[0].shape[2:])
        desc = make_conv_desc(tuple(x.shape), ws[0].shape[0] * algebra, algebra, k, stride, padding, dilation)
        x = _req(x, "x")
        y = conv_fwd(desc, x, ws, bias)
        ctx.desc = desc
        ctx.has_bias = bias is not None
        ctx.w_params, ctx.bias_param = ws, bias
        ctx.wt_ahead = _transpose_ahead(desc, ws) if ctx.needs_input_grad[0] else None
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dbias, dws = _conv_backward(ctx, dy, 5)
        return (dx, dbias, None, None, None, *dws)


def hyper_conv(x, ws, bias, stride, padding, dilation):
    if x.dim() == 5:
        return HyperConv3dFn.apply(x, bias, stride, padding, dilation, *ws)
    return HyperConvFn.apply(x, bias, stride, padding, dilation, *ws)


# ======================================================================================
# 8-multiplication Hamilton product kernels (csrc/hcq_conv.hip)
# ======================================================================================
def hcq_pack_floats(desc, mode, nsets=1):
    """Floats of the packed weight-form buffer, 0 if the fast-product kernel does not take this shape."""
    return int(L.lib().seld_hcq_pack_floats(ctypes.byref(desc), int(mode), int(nsets)))


class _HcqWeights:
    """Packed weight forms of every (layer, direction) that runs on the fast-product kernels.

    The forms depend on the weights only, so they are rebuilt when the weights change, not per call:
      * `weights_changed()` (FlatAdam.step, anything that rewrites parameters behind torch's back) starts a new epoch;
        the first request of an epoch re-packs EVERY registered entry in one launch (seld_hcq_pack_table);
      * an in-place edit torch knows about (load_state_dict, an eager optimiser) shows in the tensors' version counters
        and re-packs just the entry that is asked for;
      * parameters that moved (Module.to, FlatAdam re-homing them into its flat buffer) are noticed by their pointers.
    Entries hold weak references: a deleted model drops out at the next full re-pack."""

    def __init__(self):
        self.entries = {}
        self.epoch = 0
        self.packed_epoch = -1
        self.table = None
        self.table_dirty = True
        self.max_floats = 0
        self._esize = None

    def weights_changed(self):
        self.epoch += 1

    def reset(self):
        self.entries.clear()
        self.table, self.table_dirty, self.packed_epoch = None, True, -1

    class _Entry:
        __slots__ = ("desc", "mode", "refs", "npair", "nA", "buf", "ptrs", "vers", "epoch", "host")

    @staticmethod
    def _alive(e):
        ws = [r() for r in e.refs]
        return None if any(w is None for w in ws) else ws

    def _fill(self, e, ws):
        """(Re)build the table entry of `e` from the weights' current addresses."""
        lib = L.lib()
        if self._esize is None:
            self._esize = int(lib.seld_hcq_pack_entry_bytes())
        host = ctypes.create_string_buffer(self._esize)
        wsA, wsB = ws[:e.nA], (ws[e.nA:] if e.npair == 2 else None)
        L.check(lib.seld_hcq_pack_entry(ctypes.byref(e.desc), e.mode, e.npair, L.ptr_array8(wsA),
                                        L.ptr_array8(wsB) if wsB is not None else None, L.ptr(e.buf), host),
                "seld_hcq_pack_entry")
        e.host = host.raw
        e.ptrs = tuple(w.data_ptr() for w in ws)
        e.vers = None
        e.epoch = -1
        self.table_dirty = True

    def refresh_table(self):
        """Bring the device-side table up to date with the registered entries WITHOUT packing (host work + two small
        host-to-device copies).  train.GraphedTrainStep calls it right before recording: entries registered during the
        warm-up step left the table dirty, and the copies are not allowed inside a stream capture."""
        return self._collect()[0]

    def _collect(self):
        dead = []
        versions = {}
        for key, e in self.entries.items():
            if e is None:
                continue
            ws = self._alive(e)
            if ws is None or any(not w.is_cuda for w in ws):
                dead.append(key)
                continue
            if tuple(w.data_ptr() for w in ws) != e.ptrs:
                self._fill(e, ws)
            versions[id(e)] = tuple(w._version for w in ws)
        for key in dead:
            del self.entries[key]
            self.table_dirty = True
        live = [e for e in self.entries.values() if e is not None]
        if live and self.table_dirty:
            import numpy as np
            raw = b"".join(e.host for e in live)
            self.table = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(live[0].buf.device)
            starts = np.zeros(len(live) + 1, dtype=np.int32)
            starts[1:] = np.cumsum([(e.buf.numel() + 255) // 256 for e in live])
            self.starts = torch.from_numpy(starts).to(live[0].buf.device)
            self.total_blocks = int(starts[-1])
            self.table_dirty = False
        return live, versions

    def _pack_all(self):
        live, versions = self._collect()
        if not live:
            self.packed_epoch = self.epoch
            return
        L.check(L.lib().seld_hcq_pack_flat(L.ptr(self.table), L.ptr(self.starts), len(live), self.total_blocks,
                                           L.current_stream()), "seld_hcq_pack_flat")
        # the version counters the forms were built from: an in-place edit torch knows about (load_state_dict) between now
        # and the entry's next request shows as a mismatch there and re-packs that entry (with None recorded
        # here, an entry that was bulk-packed and then edited was served stale)
        for e in live:
            e.epoch, e.vers = self.epoch, versions[id(e)]
        self.packed_epoch = self.epoch

    def pin_for_graph(self):
        """Everything a RECORDED seld_hcq_pack_flat launch points at: the table, the block starts and the entries' form
        buffers as they are now.  `_pack_all` never edits a table in place -- it builds new tensors when an entry is added
        -- so a recorded step that holds these references keeps replaying against valid memory whatever shapes are
        registered later (validation at another batch size, an eval-only pooling entry)."""
        live = [e for e in self.entries.values() if e is not None]
        return (self.table, getattr(self, "starts", None), [e.buf for e in live])

    def get(self, desc, mode, wsA, wsB=None):
        """Packed forms for (desc, mode) of the given component tensors, or None if the shape runs on the 16/48-product
        kernels.  Fresh with respect to the weights as they are when the returned launch order is reached."""
        import weakref
        ws = list(wsA) + (list(wsB) if wsB is not None else [])
        key = (bytes(desc), mode, tuple(id(w) for w in ws))
        e = self.entries.get(key, 0)
        if e is None:
            return None
        if e == 0 or self._alive(e) is None:
            npair = 2 if wsB is not None else 1
            n = hcq_pack_floats(desc, mode, npair) if all(w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
                                                          for w in ws) else 0
            if n == 0:
                self.entries[key] = None
                return None
            e = self._Entry()
            e.desc = L.ConvDesc.from_buffer_copy(bytes(desc))
            e.mode, e.npair, e.nA = int(mode), npair, len(wsA)
            e.refs = [weakref.ref(w) for w in ws]
            e.buf = torch.empty(n, device=ws[0].device, dtype=torch.float32)
            self._fill(e, ws)
            self.entries[key] = e
        ptrs = tuple(w.data_ptr() for w in ws)
        if ptrs != e.ptrs:
            self._fill(e, ws)
        if self.packed_epoch != self.epoch:
            self._pack_all()
        vers = tuple(w._version for w in ws)
        if e.epoch != self.epoch or (e.vers is not None and e.vers != vers):
            wsA_, wsB_ = ws[:e.nA], (ws[e.nA:] if e.npair == 2 else None)
            hcq_pack(desc, mode, wsA_, wsB_, out=e.buf)
            e.epoch = self.epoch
        e.vers = vers
        return e.buf


hcq_weights = _HcqWeights()


# ---- the two branches of the two-stream model on two queues --------------------------------------------------------
_branch = {"stream": None}


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
    if hcq_weights.packed_epoch != hcq_weights.epoch:
        hcq_weights._pack_all()
    main = torch.cuda.current_stream()
    if _branch["stream"] is None:
        _branch["stream"] = torch.cuda.Stream()
    sb = _branch["stream"]
    sb.wait_stream(main)
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


L._reload_hooks.append(hcq_weights.reset)       # the forms are packed for the kernels the switches selected


@memo
def hcq_label(desc, mode, npair=1):
    return kernel_label(L.lib().seld_hcq_kernel_label, ctypes.byref(desc), int(mode), int(npair), size=96)


def hcq_pack(desc, mode, wsA, wsB=None, out=None):
    """Weight forms F_m(W) in MFMA fragment order (seld_hcq_pack): mode 0 forward, 1 data gradient."""
    nsets = 2 if wsB is not None else 1
    n = hcq_pack_floats(desc, mode, nsets)
    if n == 0:
        return None
    if out is None:
        out = torch.empty(n, device=wsA[0].device, dtype=torch.float32)
    L.check(L.lib().seld_hcq_pack(ctypes.byref(desc), int(mode), nsets, L.ptr_array8([_req(w, "w") for w in wsA]),
                                  L.ptr_array8([_req(w, "w") for w in wsB]) if wsB is not None else None, L.ptr(out),
                                  L.current_stream()), "seld_hcq_pack")
    return out


def _ptr2(a, b=None):
    arr = (ctypes.c_void_p * 2)()
    arr[0] = a.data_ptr() if a is not None else 0
    arr[1] = b.data_ptr() if b is not None else 0
    return arr


def hcq_conv(desc, mode, x, wpack, outs, biases=(None, None), epilogues=(0, 0), addends=(None, None), stats=(None, None),
             x2=None):
    """Convolution (mode 0; one or two weight sets -> outs) or data gradient (mode 1; with x2: the sum of the data
    gradients of two convolutions of the same input) from packed weight forms."""
    npair = len(outs) if mode == 0 else (2 if x2 is not None else 1)
    epi = (ctypes.c_int32 * 2)(int(epilogues[0]), int(epilogues[1]) if len(outs) > 1 else 0)
    pad = lambda v: (tuple(v) + (None, None))[:2]
    L.check(L.lib().seld_hcq_conv(ctypes.byref(desc), int(mode), npair, L.ptr(_req(x, "x")), L.ptr(_req(x2, "x2")),
                                  L.ptr(wpack), _ptr2(*pad(outs)), _ptr2(*pad(biases)), epi, _ptr2(*pad(addends)),
                                  _ptr2(*pad(stats)), L.current_stream()), "seld_hcq_conv")
    return outs


# ======================================================================================
# conv with fused epilogue (bias / residual add) as an autograd op
# ======================================================================================
class HyperConvAddFn(torch.autograd.Function):
    """y = W (x) x + addend  -- the `x + conv2_residual(y)` of model.py:132 and the running
    skip-connection sum of model.py:210-212 ride in the conv epilogue (SELD_EPI_ADD)."""

    @staticmethod
    def forward(ctx, x, bias, addend, stride, padding, dilation, *ws):
        algebra = len(ws)
        k = tuple(ws[0].shape[2:])
        desc = make_conv_desc(tuple(x.shape), ws[0].shape[0] * algebra, algebra, k, stride, padding, dilation)
        x = _req(x, "x")
        y = conv_fwd(desc, x, ws, bias, epilogue=L.SELD_EPI_ADD, addend=addend)
        ctx.desc = desc
        ctx.has_bias = bias is not None
        ctx.w_params, ctx.bias_param = ws, bias
        ctx.wt_ahead = _transpose_ahead(desc, ws) if ctx.needs_input_grad[0] else None
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, dbias, dws = _conv_backward(ctx, dy, 6)
        return (dx, dbias, dy if ctx.needs_input_grad[2] else None, None, None, None, *dws)


def hyper_conv_add(x, ws, bias, addend, stride, padding, dilation):
    return HyperConvAddFn.apply(x, bias, addend, stride, padding, dilation, *ws)


# ======================================================================================
# two convolutions of one geometry on the same input in one launch
# ======================================================================================
@memo
def _pair_ok(desc, which):
    return bool(L.lib().seld_hc_conv_pair_supported(ctypes.byref(desc), which))


class HyperConvPairFn(torch.autograd.Function):
    """(yA, yB) = (WA (x) x [+ addA], WB (x) x [+ addB]): conv1_filter | conv1_gate (model.py:121-122) and
    conv2_skip | conv2_residual (model.py:130-132, 210-212) of a residual block, one launch each way
    (seld_hc_conv_pair_*).  Falls back to the single entry points per direction when a shape does not qualify."""

    @staticmethod
    def forward(ctx, x, biasA, biasB, addA, addB, stride, padding, dilation, algebra, statsA, statsB, *ws):
        wsA, wsB = ws[:algebra], ws[algebra:]
        k = tuple(wsA[0].shape[2:])
        desc = make_conv_desc(tuple(x.shape), wsA[0].shape[0] * algebra, algebra, k, stride, padding, dilation)
        x = _req(x, "x")
        o = conv_out_shape(desc)
        yA = torch.empty(_y_shape(desc, o), device=x.device, dtype=torch.float32)
        yB = torch.empty_like(yA)
        det_stats = deterministic() and (statsA is not None or statsB is not None)
        kstA, kstB = (None, None) if det_stats else (statsA, statsB)         # statistics the kernels gather themselves
        epiA = (L.SELD_EPI_ADD if addA is not None else 0) | (L.SELD_EPI_STATS if kstA is not None else 0)
        epiB = (L.SELD_EPI_ADD if addB is not None else 0) | (L.SELD_EPI_STATS if kstB is not None else 0)
        one_launch = all(v == 1 for v in k)          # 1x1 pairs run the pair instantiation of the kernel
        # (issuing the second of two launches on the side stream was measured: 14.69 vs 14.58 ms per step, not kept)
        wp = hcq_weights.get(desc, 0, wsA, wsB) if algebra > 1 else None
        if wp is not None:                           # both convolutions in one launch of the fast-product kernel
            with _timed(desc, 0, 2, label=lambda: hcq_label(desc, 0, 2)):
                hcq_conv(desc, 0, x, wp, (yA, yB), (_req(biasA, "bias"), _req(biasB, "bias")), (epiA, epiB),
                         (_req(addA, "addend"), _req(addB, "addend")), (kstA, kstB))
        else:
            with _timed(desc, 0, 2, one_launch):
                rc = L.lib().seld_hc_conv_pair_fwd(
                    ctypes.byref(desc), L.ptr(x), L.ptr_array8([_req(w, "w") for w in wsA]),
                    L.ptr_array8([_req(w, "w") for w in wsB]), L.ptr(_req(biasA, "bias")), L.ptr(_req(biasB, "bias")),
                    L.ptr(yA), L.ptr(yB), epiA, epiB, L.ptr(_req(addA, "addend")), L.ptr(_req(addB, "addend")),
                    L.ptr(kstA), L.ptr(kstB), L.current_stream())
            if rc == -4:       # SELD_EUNSUPPORTED: e.g. the two weight sets lie more than 4 GB apart
                conv_fwd(desc, x, wsA, biasA, out=yA, epilogue=epiA, addend=addA, stats=kstA)
                conv_fwd(desc, x, wsB, biasB, out=yB, epilogue=epiB, addend=addB, stats=kstB)
            else:
                L.check(rc, "seld_hc_conv_pair_fwd")
        if det_stats:
            if statsA is not None:
                channel_stats(yA, out=statsA)
            if statsB is not None:
                channel_stats(yB, out=statsB)
        ctx.desc, ctx.algebra = desc, algebra
        ctx.params = (wsA, wsB, biasA, biasB)
        ctx.wt_ahead = None
        if ctx.needs_input_grad[0] and _pair_ok(desc, 1) and not _hcq_ok(desc, 1, 2):
            a_, b_ = _transpose_ahead(desc, wsA), _transpose_ahead(desc, wsB)
            ctx.wt_ahead = (a_, b_) if a_ is not None and b_ is not None else None
        ctx.save_for_backward(x)
        return yA, yB

    @staticmethod
    def backward(ctx, dyA, dyB):
        (x,) = ctx.saved_tensors
        desc, A = ctx.desc, ctx.algebra
        wsA, wsB, biasA, biasB = ctx.params
        dyA, dyB = _req(dyA, "dy"), _req(dyB, "dy")
        lib = L.lib()
        dx = None
        if ctx.needs_input_grad[0]:
            wp = hcq_weights.get(desc, 1, wsA, wsB) if A > 1 else None
            if wp is not None:                       # sum of both data gradients in one launch
                dx = torch.empty(tuple(x.shape), device=x.device, dtype=torch.float32)
                with _timed(desc, 1, 2, label=lambda: hcq_label(desc, 1, 2)):
                    hcq_conv(desc, 1, dyA, wp, (dx,), x2=dyB)
            elif _pair_ok(desc, 1) and ctx.wt_ahead is not None:
                (wtA, evA), (wtB, evB) = ctx.wt_ahead
                dx = torch.empty(tuple(x.shape), device=x.device, dtype=torch.float32)
                torch.cuda.current_stream().wait_event(evA)
                torch.cuda.current_stream().wait_event(evB)
                with _timed(desc, 1, 2):
                    L.check(lib.seld_hc_conv_pair_bwd_data_wt(ctypes.byref(desc), L.ptr(dyA), L.ptr(dyB), L.ptr(wtA),
                                                              L.ptr(wtB), L.ptr(dx), L.current_stream()),
                            "seld_hc_conv_pair_bwd_data_wt")
            elif _pair_ok(desc, 1):
                dx = torch.empty(tuple(x.shape), device=x.device, dtype=torch.float32)
                nbytes = 2 * lib.seld_hc_conv_bwd_data_workspace(ctypes.byref(desc))
                wsb = torch.empty((nbytes + 3) // 4, device=x.device, dtype=torch.float32)
                with _timed(desc, 1, 2):
                    L.check(lib.seld_hc_conv_pair_bwd_data(ctypes.byref(desc), L.ptr(dyA), L.ptr(dyB),
                                                           L.ptr_array8(list(wsA)), L.ptr_array8(list(wsB)), L.ptr(dx),
                                                           L.ptr(wsb), nbytes, L.current_stream()),
                            "seld_hc_conv_pair_bwd_data")
            else:
                dx = conv_bwd_data(desc, dyA, wsA, tuple(x.shape))
                dx += conv_bwd_data(desc, dyB, wsB, tuple(x.shape))
        need_w = any(ctx.needs_input_grad[11:]) or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dwsA, dwsB, dbA, dbB = [None] * A, [None] * A, None, None
        if need_w:
            dirA, dirB = _direct_targets(wsA, biasA), _direct_targets(wsB, biasB)
            if dirA is not None and dirB is not None and dirA[1] is None and dirB[1] is None and deferred_wgrads.takes(desc):
                deferred_wgrads.add(desc, x, dyA, dirA[0])
                deferred_wgrads.add(desc, x, dyB, dirB[0])
            elif dirA is not None and dirB is not None and dirA[1] is None and dirB[1] is None and _hcq_wgrad_ok(desc, 2):
                def pair_wgrad_fast():
                    hcq_wgrad_acc(desc, x, dyA, dirA[0], dyB, dirB[0])
                if _side_enabled():
                    _on_side_stream(pair_wgrad_fast, x, dyA, dyB)
                else:
                    pair_wgrad_fast()
            elif dirA is not None and dirB is not None and _pair_ok(desc, 2) and not deterministic():
                def pair_wgrad():
                    with _timed(desc, 2, 2):
                        L.check(lib.seld_hc_conv_pair_bwd_weight_acc(ctypes.byref(desc), L.ptr(x), L.ptr(dyA), L.ptr(dyB),
                                                                     L.ptr_array8(dirA[0]), L.ptr_array8(dirB[0]),
                                                                     L.ptr(dirA[1]), L.ptr(dirB[1]), L.current_stream()),
                                "seld_hc_conv_pair_bwd_weight_acc")
                if _side_enabled():
                    _on_side_stream(pair_wgrad, x, dyA, dyB)
                else:
                    pair_wgrad()
            else:
                for ws_, b_, dy_, tgt in ((wsA, biasA, dyA, "A"), (wsB, biasB, dyB, "B")):
                    d_ = _direct_targets(ws_, b_)
                    if d_ is not None:
                        conv_bwd_weight(desc, x, dy_, tuple(ws_[0].shape), b_ is not None, into=d_[0], bias_into=d_[1])
                    else:
                        g, gb = conv_bwd_weight(desc, x, dy_, tuple(ws_[0].shape), b_ is not None)
                        if tgt == "A":
                            dwsA, dbA = g, gb
                        else:
                            dwsB, dbB = g, gb
        return (dx, dbA, dbB, dyA if ctx.needs_input_grad[3] else None, dyB if ctx.needs_input_grad[4] else None,
                None, None, None, None, None, None, *dwsA, *dwsB)


def hyper_conv_pair(x, wsA, biasA, wsB, biasB, stride, padding, dilation, addA=None, addB=None, statsA=None, statsB=None):
    """Two convolutions of the same input.  One call when both have the same shape (and one launch per direction
    where the kernels support the pair form); otherwise exactly the two single calls.  statsA / statsB: zeroed
    statistics buffers (`new_stats`) to receive the BatchNorm batch statistics of the two results."""
    same = (len(wsA) == len(wsB) and tuple(wsA[0].shape) == tuple(wsB[0].shape) and
            (biasA is None) == (biasB is None) and x.is_cuda)
    if same:
        k = tuple(wsA[0].shape[2:])
        desc = make_conv_desc(tuple(x.shape), wsA[0].shape[0] * len(wsA), len(wsA), k, stride, padding, dilation)
        if _pair_ok(desc, 0):
            return HyperConvPairFn.apply(x, biasA, biasB, addA, addB, stride, padding, dilation, len(wsA), statsA, statsB,
                                         *wsA, *wsB)

    def one(ws, bias, add, stats):
        y = hyper_conv(x, ws, bias, stride, padding, dilation) if add is None else \
            hyper_conv_add(x, ws, bias, add, stride, padding, dilation)
        if stats is not None:
            N, C, S = _ncs(y)
            L.check(L.lib().seld_channel_stats(L.ptr(y), N, C, S, L.ptr(stats), L.current_stream()), "seld_channel_stats")
        return y
    return one(wsA, biasA, addA, statsA), one(wsB, biasB, addB, statsB)
