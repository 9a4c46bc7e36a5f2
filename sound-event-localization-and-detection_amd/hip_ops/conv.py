"""2-D / 1-D hypercomplex convolution (csrc/hc_conv*.hip, csrc/hcq_*.hip): descriptors, the three entry points, the
grouped / deferred weight gradients, the router that decides where a layer's weight gradient goes, and the autograd
functions.  The packed weight forms live in weight_forms.py, the side stream in streams.py."""
import ctypes
import os

import torch

from .. import _lib as L
from ._core import _pair, _req, deterministic, kernel_label, memo, scratch, timed
from .conv3d import HyperConv3dFn
from .norm_act import _direct_targets, channel_stats
from .streams import _on_side_stream, _side_enabled, side_queue
from .weight_forms import _hcq_ok, hcq_weights


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


def conv_pair_bwd_data(desc, dyA, dyB, wsA, wsB, x_shape, ahead=None):
    """Sum of the data gradients of two convolutions of one input: one launch where a pair form takes the shape, else the
    two single calls.  `ahead`: the two sets' (workspace, event) from _transpose_ahead."""
    lib = L.lib()
    wp = hcq_weights.get(desc, 1, wsA, wsB) if desc.algebra > 1 else None
    if wp is None and not _pair_ok(desc, 1):
        dx = conv_bwd_data(desc, dyA, wsA, x_shape)
        dx += conv_bwd_data(desc, dyB, wsB, x_shape)
        return dx
    dx = torch.empty(x_shape, device=dyA.device, dtype=torch.float32)
    if wp is not None:
        with _timed(desc, 1, 2, label=lambda: hcq_label(desc, 1, 2)):
            hcq_conv(desc, 1, dyA, wp, (dx,), x2=dyB)
    elif ahead is not None:
        (wtA, evA), (wtB, evB) = ahead
        torch.cuda.current_stream().wait_event(evA)
        torch.cuda.current_stream().wait_event(evB)
        with _timed(desc, 1, 2):
            L.check(lib.seld_hc_conv_pair_bwd_data_wt(ctypes.byref(desc), L.ptr(dyA), L.ptr(dyB), L.ptr(wtA), L.ptr(wtB),
                                                      L.ptr(dx), L.current_stream()), "seld_hc_conv_pair_bwd_data_wt")
    else:
        nbytes = 2 * lib.seld_hc_conv_bwd_data_workspace(ctypes.byref(desc))
        wsb = torch.empty((nbytes + 3) // 4, device=dyA.device, dtype=torch.float32)
        with _timed(desc, 1, 2):
            L.check(lib.seld_hc_conv_pair_bwd_data(ctypes.byref(desc), L.ptr(dyA), L.ptr(dyB), L.ptr_array8(list(wsA)),
                                                   L.ptr_array8(list(wsB)), L.ptr(dx), L.ptr(wsb), nbytes,
                                                   L.current_stream()), "seld_hc_conv_pair_bwd_data")
    return dx


def _hcq_wgrad_ok(desc, npair=1):
    if deterministic():
        return False
    return _hcq_wgrad_taken(desc, npair)


@memo
def _hcq_wgrad_taken(desc, npair):
    return bool(L.lib().seld_hcq_wgrad_supported(ctypes.byref(desc), int(npair)))


@memo
def _hcq_wgrad_label(desc, npair=1):
    return kernel_label(L.lib().seld_hcq_wgrad_label, ctypes.byref(desc), int(npair), size=96)


def hcq_wgrad_acc(desc, x, dyA, dwA, dyB=None, dwB=None):
    """dwA[c] += wgrad(x, dyA) [, dwB[c] += wgrad(x, dyB)] on the fast-product kernel of the quaternion layers
    (seld_hcq_wgrad_acc)."""
    npair = 2 if dyB is not None else 1
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


def _transpose_ahead(desc, ws):
    """The data gradient's weight re-layout (seld_hc_conv_transpose_weights), issued NOW on the side stream -- i.e. during
    the forward pass, where it overlaps the convolution -- instead of in front of the data-gradient kernel on the critical
    path of the backward pass (47 launches of ~5 us per step).  Returns (workspace tensor, event) or None."""
    if not _side_enabled() or not torch.is_grad_enabled() or _hcq_ok(desc, 1):
        return None
    lib = L.lib()
    nbytes = lib.seld_hc_conv_bwd_data_workspace(ctypes.byref(desc))
    wt = torch.empty((nbytes + 3) // 4, device=ws[0].device, dtype=torch.float32)
    with side_queue.fork(wt):                            # the weights may still be in flight (Adam of the last step)
        L.check(lib.seld_hc_conv_transpose_weights(ctypes.byref(desc), L.ptr_array8([_req(w, "w") for w in ws]),
                                                   L.ptr(wt), nbytes, L.current_stream()),
                "seld_hc_conv_transpose_weights")
        ev = side_queue.event()
    return wt, ev


@memo
def _pair_ok(desc, which):
    return bool(L.lib().seld_hc_conv_pair_supported(ctypes.byref(desc), which))


def _route_wgrads(desc, x, sets, need_dx):
    """Where the weight gradients of one convolution of `x`, or of two of the same geometry, go.  sets: [(dy, ws, bias)]
    per weight set; need_dx: x takes a gradient too.  The first that applies:
      1. the deferred group (issued with the other layers' when the backward pass ends): every set has gradient slots
         (`_direct_targets`), none a bias slot, and `deferred_wgrads` takes the shape;
      2. two sets, one launch of the fast-product kernels: slots, no bias slot, `_hcq_wgrad_ok(desc, 2)`;
      3. two sets, one launch of the pair kernel: slots, `_pair_ok(desc, 2)`, not deterministic();
         (2 and 3 on the side stream when it is enabled, else on the current one)
      4. one set, the per-layer accumulating kernels on the side stream: slots, side stream enabled, need_dx;
      5. per set, on the current stream: accumulated into the set's slots where it has them, else fresh tensors.
    1 - 4 are issued here.  Returns a callable that issues 5, if it is left, and returns per set the (dws, dbias) autograd
    still has to receive.  A single convolution calls it behind its data gradient; the pair routes behind its own."""
    direct = [_direct_targets(ws, bias) for _, ws, bias in sets]
    slots = all(d is not None for d in direct)
    no_bias = slots and all(d[1] is None for d in direct)
    dys = [dy for dy, _, _ in sets]
    pair = len(sets) == 2
    none = ([None] * desc.algebra, None)

    def per_set():
        out = []
        for (dy, ws, bias), d in zip(sets, direct):
            into, bias_into = d or (None, None)
            g = conv_bwd_weight(desc, x, dy, tuple(ws[0].shape), bias is not None, into=into, bias_into=bias_into)
            out.append(g if d is None else none)
        return out

    def pair_kernel():
        (dwA, dbA), (dwB, dbB) = direct
        with _timed(desc, 2, 2):
            L.check(L.lib().seld_hc_conv_pair_bwd_weight_acc(ctypes.byref(desc), L.ptr(x), L.ptr(dys[0]), L.ptr(dys[1]),
                                                             L.ptr_array8(dwA), L.ptr_array8(dwB), L.ptr(dbA), L.ptr(dbB),
                                                             L.current_stream()), "seld_hc_conv_pair_bwd_weight_acc")

    if no_bias and deferred_wgrads.takes(desc):
        for dy, d in zip(dys, direct):
            deferred_wgrads.add(desc, x, dy, d[0])
    elif pair and no_bias and _hcq_wgrad_ok(desc, 2):
        launch = lambda: hcq_wgrad_acc(desc, x, dys[0], direct[0][0], dys[1], direct[1][0])
        _on_side_stream(launch, x, *dys) if _side_enabled() else launch()
    elif pair and slots and _pair_ok(desc, 2) and not deterministic():
        _on_side_stream(pair_kernel, x, *dys) if _side_enabled() else pair_kernel()
    elif not pair and slots and _side_enabled() and need_dx:
        _on_side_stream(per_set, x, *dys)
    else:
        return per_set
    return lambda: [none] * len(sets)


def _conv_forward(ctx, x, bias, ws, stride, padding, dilation, epilogue=0, addend=None, stats=None):
    """forward() of the autograd functions of ONE convolution: y, and in ctx what _conv_backward needs."""
    algebra = len(ws)
    k = tuple(ws[0].shape[2:])
    desc = make_conv_desc(tuple(x.shape), ws[0].shape[0] * algebra, algebra, k, stride, padding, dilation)
    x = _req(x, "x")
    y = conv_fwd(desc, x, ws, bias, epilogue=epilogue, addend=addend, stats=stats)
    ctx.desc = desc
    ctx.has_bias = bias is not None
    ctx.w_params, ctx.bias_param = ws, bias
    ctx.wt_ahead = _transpose_ahead(desc, ws) if ctx.needs_input_grad[0] else None
    ctx.save_for_backward(x)
    return y


def _conv_backward(ctx, dy, first_w):
    x, ws = ctx.saved_tensors[0], ctx.w_params
    dy = _req(dy, "dy")
    dws, dbias = [None] * len(ws), None
    need_w = any(ctx.needs_input_grad[first_w:]) or (ctx.has_bias and ctx.needs_input_grad[1])
    rest = _route_wgrads(ctx.desc, x, [(dy, ws, ctx.bias_param)], ctx.needs_input_grad[0]) if need_w else None
    dx = conv_bwd_data(ctx.desc, dy, ws, tuple(x.shape), ctx.wt_ahead) if ctx.needs_input_grad[0] else None
    if rest is not None:
        (dws, dbias), = rest()
    return dx, dbias, dws


class HyperConvFn(torch.autograd.Function):
    """y = W (x) x  for algebra 1/4/8; replaces quaternion_conv / dual_quaternion_conv / F.convNd."""

    @staticmethod
    def forward(ctx, x, bias, stride, padding, dilation, *ws):
        return _conv_forward(ctx, x, bias, ws, stride, padding, dilation)

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
@memo
def hcq_label(desc, mode, npair=1):
    return kernel_label(L.lib().seld_hcq_kernel_label, ctypes.byref(desc), int(mode), int(npair), size=96)


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
        return _conv_forward(ctx, x, bias, ws, stride, padding, dilation, epilogue=L.SELD_EPI_ADD, addend=addend)

    @staticmethod
    def backward(ctx, dy):
        dx, dbias, dws = _conv_backward(ctx, dy, 6)
        return (dx, dbias, dy if ctx.needs_input_grad[2] else None, None, None, None, *dws)


def hyper_conv_add(x, ws, bias, addend, stride, padding, dilation):
    return HyperConvAddFn.apply(x, bias, addend, stride, padding, dilation, *ws)


# ======================================================================================
# two convolutions of one geometry on the same input in one launch
# ======================================================================================
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
        for y, stats in ((yA, statsA), (yB, statsB)) if det_stats else ():
            if stats is not None:
                channel_stats(y, out=stats)
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
        (x,), desc = ctx.saved_tensors, ctx.desc
        wsA, wsB, biasA, biasB = ctx.params
        dyA, dyB = _req(dyA, "dy"), _req(dyB, "dy")
        dx = conv_pair_bwd_data(desc, dyA, dyB, wsA, wsB, tuple(x.shape), ctx.wt_ahead) if ctx.needs_input_grad[0] else None
        grads = [([None] * ctx.algebra, None)] * 2
        if any(ctx.needs_input_grad[11:]) or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            grads = _route_wgrads(desc, x, [(dyA, wsA, biasA), (dyB, wsB, biasB)], ctx.needs_input_grad[0])()
        (dwsA, dbA), (dwsB, dbB) = grads
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
            channel_stats(y, out=stats)
        return y
    return one(wsA, biasA, addA, statsA), one(wsB, biasB, addB, statsB)
