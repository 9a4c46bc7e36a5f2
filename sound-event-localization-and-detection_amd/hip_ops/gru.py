"""GRU layers (csrc/gru.hip): the input and weight-gradient products on the linear kernels, the recurrence in one launch per
layer and pass for every direction."""
import torch

from .. import _lib as L
from ._core import _req, kernel_label
from .norm_act import _claim_grad_slots
from .norm_act import dropout as _dropout
from .weight_forms import gru_weights

__all__ = ["gru", "gru_kernel_label", "GruLayerFn", "GRU_MAX_HIDDEN", "GRU_FWD", "GRU_BWD"]

GRU_MAX_HIDDEN = 128        # SELD_GRU_MAX_HIDDEN
GRU_FWD, GRU_BWD = 0, 1     # seld_gru_kernel_label(op, ...)


def gru_kernel_label(op, hidden):
    """Name of the kernel instance seld_gru_fwd / seld_gru_bwd launches for this hidden size."""
    return kernel_label(L.lib().seld_gru_kernel_label, int(op), int(hidden))


def _linear_bwd(rows, in_f, out_f, x, dy, w, dx, dw, db):
    lib = L.lib()
    nbytes = lib.seld_hc_linear_bwd_workspace(L.SELD_LIN_REAL, in_f, out_f)
    wsb = torch.empty((nbytes + 3) // 4, device=dy.device, dtype=torch.float32)
    L.check(lib.seld_hc_linear_bwd(L.SELD_LIN_REAL, rows, in_f, out_f, L.ptr(x), L.ptr(dy), L.ptr_array8([w]), L.ptr(dx),
                                   L.ptr_array8([dw]) if dw is not None else None, L.ptr(db), L.ptr(wsb), nbytes,
                                   L.current_stream()), "seld_hc_linear_bwd")


class GruLayerFn(torch.autograd.Function):
    """One layer: x (B, T, I), h0 (dirs, B, H) or None -> y (B, T, dirs*H), h_n (dirs, B, H).  `params` is, per direction,
    weight_ih (3H, I), weight_hh (3H, H), bias_ih, bias_hh (both None in a layer without bias)."""

    @staticmethod
    def forward(ctx, x, h0, hidden, dirs, has_bias, *params):
        x = _req(x, "x")
        if x.dim() != 3:
            raise L.SeldHipError(f"gru: expected x (B, T, I), got {tuple(x.shape)}")
        B, T, I = x.shape
        per = 4 if has_bias else 2
        if len(params) != dirs * per:
            raise L.SeldHipError(f"gru: {dirs} direction(s) take {dirs * per} parameters, got {len(params)}")
        groups = [params[d * per:(d + 1) * per] for d in range(dirs)]
        for w_ih, w_hh, *bs in groups:
            if tuple(w_ih.shape) != (3 * hidden, I) or tuple(w_hh.shape) != (3 * hidden, hidden) or \
                    any(tuple(b.shape) != (3 * hidden,) for b in bs):
                raise L.SeldHipError(f"gru: parameter shapes do not fit hidden {hidden}, input {I}")
        h0 = _req(h0, "h0")
        if h0 is not None and tuple(h0.shape) != (dirs, B, hidden):
            raise L.SeldHipError(f"gru: expected h0 {(dirs, B, hidden)}, got {tuple(h0.shape)}")
        lib, st, dev = L.lib(), L.current_stream(), x.device
        G = 3 * hidden
        gx = torch.empty((dirs, B, T, G), device=dev, dtype=torch.float32)
        for d, (w_ih, _, *bs) in enumerate(groups):
            L.check(lib.seld_hc_linear_fwd(L.SELD_LIN_REAL, B * T, I, G, L.ptr(x), L.ptr_array8([_req(w_ih, "weight_ih")]),
                                           L.ptr(_req(bs[0], "bias_ih") if bs else None), L.ptr(gx[d]), st),
                    "seld_hc_linear_fwd")
        wpack = gru_weights.get(hidden, [g[1] for g in groups], [g[3] if has_bias else None for g in groups])
        need = any(ctx.needs_input_grad)
        nsaved = int(lib.seld_gru_saved_floats(dirs, B, T, hidden)) if need else 0
        saved = torch.empty(nsaved, device=dev, dtype=torch.float32) if need else None
        y = torch.empty((B, T, dirs * hidden), device=dev, dtype=torch.float32)
        h_n = torch.empty((dirs, B, hidden), device=dev, dtype=torch.float32)
        L.check(lib.seld_gru_fwd(dirs, B, T, hidden, L.ptr(gx), L.ptr(wpack), L.ptr(h0), L.ptr(y), L.ptr(h_n), L.ptr(saved),
                                 nsaved, st), "seld_gru_fwd")
        ctx.geom = (dirs, B, T, I, hidden, has_bias, h0 is not None)
        ctx.params = params
        ctx.set_materialize_grads(False)
        if need:
            ctx.save_for_backward(x, saved, wpack)
        return y, h_n

    @staticmethod
    def backward(ctx, dy, dh_n):
        dirs, B, T, I, hidden, has_bias, has_h0 = ctx.geom
        x, saved, wpack = ctx.saved_tensors
        lib, st, dev = L.lib(), L.current_stream(), x.device
        G, per = 3 * hidden, 4 if has_bias else 2
        if dy is None:
            dy = torch.zeros((B, T, dirs * hidden), device=dev, dtype=torch.float32)
        dy, dh_n = _req(dy, "dy"), _req(dh_n, "dh_n")
        dgx = torch.empty((dirs, B, T, G), device=dev, dtype=torch.float32)
        dgh = torch.empty_like(dgx)
        dh0 = torch.empty((dirs, B, hidden), device=dev, dtype=torch.float32) if has_h0 and ctx.needs_input_grad[1] else None
        L.check(lib.seld_gru_bwd(dirs, B, T, hidden, L.ptr(dy), L.ptr(dh_n), L.ptr(wpack), L.ptr(saved), saved.numel(),
                                 L.ptr(dgx), L.ptr(dgh), L.ptr(dh0), st), "seld_gru_bwd")
        params = ctx.params
        need_p = any(ctx.needs_input_grad[5:])
        # as in HyperLinearFn: the folds WRITE the parameter gradients, straight into flat-gradient slots that are still
        # zero since zero_grad; otherwise autograd accumulates what is returned
        direct = False
        if need_p and all(ctx.needs_input_grad[5:]) and all(p.is_contiguous() for p in params):
            slot, clean = _claim_grad_slots(list(params), adjacent=False)
            direct = slot is not None and clean
        grads = [None] * len(params)
        if need_p:
            grads = [p.grad if direct else torch.empty_like(p) for p in params]
        h_prev = saved.view(5, dirs, B * T, hidden)[4]
        dxs = []
        for d in range(dirs):
            w_ih, w_hh = params[d * per], params[d * per + 1]
            g = grads[d * per:(d + 1) * per]
            dxd = torch.empty((B * T, I), device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
            if dxd is not None or need_p:
                _linear_bwd(B * T, I, G, x, dgx[d], w_ih, dxd, g[0], g[2] if has_bias else None)
            if need_p:
                _linear_bwd(B * T, hidden, G, h_prev[d], dgh[d], w_hh, None, g[1], g[3] if has_bias else None)
            dxs.append(dxd)
        dx = dxs[0]
        if dx is not None and dirs == 2:
            dx = torch.empty_like(dxs[0])
            L.check(lib.seld_add(L.ptr(dxs[0]), L.ptr(dxs[1]), dx.numel(), L.ptr(dx), st), "seld_add")
        if dx is not None:
            dx = dx.view(B, T, I)
        if direct or not need_p:
            grads = [None] * len(params)
        return (dx, dh0, None, None, None, *grads)


def gru(x, params, hidden, layers, dirs, h0=None, dropout=0., training=False):
    """torch.nn.GRU's forward on a batch-first x (B, T, I): `params[layer][direction]` = (weight_ih, weight_hh, bias_ih,
    bias_hh), the biases None in a stack without them; h0 (layers*dirs, B, hidden) or None.  Returns y (B, T, dirs*hidden)
    of the last layer and h_n (layers*dirs, B, hidden).  Between layers (not after the last) the project's dropout: the
    same distribution as torch's, another random stream."""
    if hidden > GRU_MAX_HIDDEN or hidden < 1:
        raise L.SeldHipError(f"gru: hidden size {hidden} outside 1..{GRU_MAX_HIDDEN}")
    if dirs not in (1, 2) or layers < 1 or len(params) != layers or any(len(p) != dirs for p in params):
        raise L.SeldHipError(f"gru: expected parameters of {layers} layer(s) x {dirs} direction(s)")
    if h0 is not None and (h0.dim() != 3 or h0.shape[0] != layers * dirs):
        raise L.SeldHipError(f"gru: expected h0 ({layers * dirs}, B, {hidden}), got {tuple(h0.shape)}")
    has_bias = params[0][0][2] is not None
    h_ns = []
    for layer, groups in enumerate(params):
        flat = [p for g in groups for p in (g if has_bias else g[:2])]
        h0_l = h0[layer * dirs:(layer + 1) * dirs] if h0 is not None else None
        x, h_n = GruLayerFn.apply(x, h0_l, hidden, dirs, has_bias, *flat)
        h_ns.append(h_n)
        if layer + 1 < layers:
            x = _dropout(x, dropout, training)
    return x, (h_ns[0] if layers == 1 else torch.cat(h_ns, 0))
