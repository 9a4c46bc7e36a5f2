"""fp64 GRU written from the formulas of include/seld_hip.h (gate order r | z | n), forward and backward, without
torch.nn.GRU and without autograd; the shared case list; seeded inputs.

    r  = sigmoid(gx_r + W_hr h + b_hr)        z = sigmoid(gx_z + W_hz h + b_hz)
    n  = tanh(gx_n + r * (W_hn h + b_hn))     h' = (1 - z) * n + z * h           gx = x @ W_ih^T + b_ih
"""
import math

import torch

# (B, T, I, H, dirs, h0, bias, scale)
CASES = {
    "single_step": (1, 1, 8, 16, 1, False, True, 1.0),
    "odd_T_masked_columns": (3, 37, 24, 32, 2, True, True, 1.0),
    "saturated_gates": (3, 37, 24, 32, 2, False, True, 4.0),
    "second_tile_no_bias": (17, 33, 40, 48, 2, True, False, 2.0),
    "H_padded": (2, 9, 8, 20, 2, True, True, 1.0),
    "largest_resident": (2, 64, 128, 128, 2, False, True, 1.0),
    "whole_clip": (2, 600, 16, 16, 1, False, True, 1.0),
}


def make_case(name):
    """Inputs of a case, float64 tensors holding float32 values (so the fp32 code under test reads the same numbers):
    x (B, T, I); per direction w_ih, w_hh, b_ih, b_hh (None without bias), U(-1/sqrt(H), 1/sqrt(H)) * scale; h0
    (dirs, B, H) or None; the output gradients dy (B, T, dirs*H) and dh_n (dirs, B, H); and gx32 (dirs, B, T, 3H), gx
    rounded to float32: the recurrence alone is tested from it."""
    B, T, I, H, dirs, has_h0, bias, scale = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    f32 = lambda t: t.float().double()
    rnd = lambda *s: f32(torch.randn(*s, generator=g, dtype=torch.float64))
    k = scale / math.sqrt(H)
    uni = lambda *s: f32((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k)
    params = []
    for _ in range(dirs):
        w_ih, w_hh = uni(3 * H, I), uni(3 * H, H)
        params.append((w_ih, w_hh, uni(3 * H) if bias else None, uni(3 * H) if bias else None))
    c = dict(name=name, B=B, T=T, I=I, H=H, dirs=dirs, x=rnd(B, T, I), params=params,
             h0=0.5 * rnd(dirs, B, H) if has_h0 else None, dy=rnd(B, T, dirs * H), dh_n=rnd(dirs, B, H))
    c["h0"] = f32(c["h0"]) if has_h0 else None
    c["gx32"] = f32(input_gates(c["x"], params))
    return c


def input_gates(x, params):
    """gx (dirs, B, T, 3H)."""
    return torch.stack([x @ w_ih.T + (b_ih if b_ih is not None else 0) for w_ih, _, b_ih, _ in params])


def recurrence_forward(gx, params, h0):
    """y (B, T, dirs*H), h_n (dirs, B, H) and what the backward needs, from gx (dirs, B, T, 3H)."""
    dirs, B, T, G = gx.shape
    H = G // 3
    y = gx.new_zeros(B, T, dirs * H)
    h_n = gx.new_zeros(dirs, B, H)
    saved = {k: gx.new_zeros(dirs, B, T, H) for k in ("r", "z", "n", "q", "h_prev")}
    for d in range(dirs):
        _, w_hh, _, b_hh = params[d]
        h = h0[d].clone() if h0 is not None else gx.new_zeros(B, H)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            gh = h @ w_hh.T + (b_hh if b_hh is not None else 0)
            r = torch.sigmoid(gx[d, :, t, :H] + gh[:, :H])
            z = torch.sigmoid(gx[d, :, t, H:2 * H] + gh[:, H:2 * H])
            q = gh[:, 2 * H:]
            n = torch.tanh(gx[d, :, t, 2 * H:] + r * q)
            for k, v in (("r", r), ("z", z), ("n", n), ("q", q), ("h_prev", h)):
                saved[k][d, :, t] = v
            h = (1 - z) * n + z * h
            y[:, t, d * H:(d + 1) * H] = h
        h_n[d] = h
    return y, h_n, saved


def recurrence_backward(dy, dh_n, params, saved):
    """dgx, dgh (dirs, B, T, 3H) and dh0 (dirs, B, H)."""
    dirs, B, T, H = saved["r"].shape
    dgx = dy.new_zeros(dirs, B, T, 3 * H)
    dgh = dy.new_zeros(dirs, B, T, 3 * H)
    dh0 = dy.new_zeros(dirs, B, H)
    for d in range(dirs):
        w_hh = params[d][1]
        dh = dh_n[d].clone() if dh_n is not None else dy.new_zeros(B, H)
        for t in (range(T - 1, -1, -1) if d == 0 else range(T)):
            r, z, n, q, hp = (saved[k][d, :, t] for k in ("r", "z", "n", "q", "h_prev"))
            dh = dh + dy[:, t, d * H:(d + 1) * H]
            dn = dh * (1 - z) * (1 - n * n)
            dr = dn * q * r * (1 - r)
            dz = dh * (hp - n) * z * (1 - z)
            dgx[d, :, t] = torch.cat((dr, dz, dn), 1)
            dgh[d, :, t] = torch.cat((dr, dz, dn * r), 1)
            dh = dh * z + dgh[d, :, t] @ w_hh
        dh0[d] = dh
    return dgx, dgh, dh0


def layer(c):
    """Everything one layer computes for the case `c`, forward and backward of sum(y * dy) + sum(h_n * dh_n): a dict of
    y, h_n, dgx, dh0, dx and, per direction, dW_ih, dW_hh, db_ih, db_hh."""
    x, params = c["x"], c["params"]
    gx = input_gates(x, params)
    y, h_n, saved = recurrence_forward(gx, params, c["h0"])
    dgx, dgh, dh0 = recurrence_backward(c["dy"], c["dh_n"], params, saved)
    B, T, I = x.shape
    H = c["H"]
    out = dict(y=y, h_n=h_n, dgx=dgx, dh0=dh0, dx=sum(dgx[d] @ params[d][0] for d in range(c["dirs"])))
    for d in range(c["dirs"]):
        gxd, ghd = dgx[d].reshape(B * T, 3 * H), dgh[d].reshape(B * T, 3 * H)
        out[f"dW_ih{d}"] = gxd.T @ x.reshape(B * T, I)
        out[f"dW_hh{d}"] = ghd.T @ saved["h_prev"][d].reshape(B * T, H)
        out[f"db_ih{d}"] = gxd.sum(0)
        out[f"db_hh{d}"] = ghd.sum(0)
    return out


def recurrence(c):
    """The recurrence alone, from gx32: y, h_n, dgx, dgh, dh0."""
    y, h_n, saved = recurrence_forward(c["gx32"], c["params"], c["h0"])
    dgx, dgh, dh0 = recurrence_backward(c["dy"], c["dh_n"], c["params"], saved)
    return dict(y=y, h_n=h_n, dgx=dgx, dgh=dgh, dh0=dh0)


def torch_gru(c, dtype, identity_input=False):
    """torch.nn.GRU (CPU, `dtype`) on the case: the same dict as `layer`.  identity_input: the layer is fed gx32 through
    an identity W_ih and no b_ih, so that its input gradient is dgx (the products with 1 and 0 are exact): the dict of
    `recurrence` without dgh."""
    B, T, I, H, dirs = c["B"], c["T"], c["I"], c["H"], c["dirs"]
    bias = c["params"][0][2] is not None
    G = 3 * H
    m = torch.nn.GRU(dirs * G if identity_input else I, H, 1, bias=bias, batch_first=True, bidirectional=dirs == 2).to(dtype)
    with torch.no_grad():
        for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(c["params"]):
            sfx = "_l0" + ("_reverse" if d else "")
            if identity_input:
                w_ih = torch.zeros(G, dirs * G, dtype=torch.float64)
                w_ih[:, d * G:(d + 1) * G] = torch.eye(G, dtype=torch.float64)
                b_ih = torch.zeros(G, dtype=torch.float64) if bias else None
            getattr(m, "weight_ih" + sfx).copy_(w_ih)
            getattr(m, "weight_hh" + sfx).copy_(w_hh)
            if bias:
                getattr(m, "bias_ih" + sfx).copy_(b_ih)
                getattr(m, "bias_hh" + sfx).copy_(b_hh)
    if identity_input:
        x = c["gx32"].permute(1, 2, 0, 3).reshape(B, T, dirs * G).to(dtype).clone().requires_grad_(True)
    else:
        x = c["x"].to(dtype).clone().requires_grad_(True)
    h0 = (c["h0"] if c["h0"] is not None else torch.zeros(dirs, B, H)).to(dtype).clone().requires_grad_(True)    # zeros: still dh0
    y, h_n = m(x, h0)
    ((y * c["dy"].to(dtype)).sum() + (h_n * c["dh_n"].to(dtype)).sum()).backward()
    out = dict(y=y.detach(), h_n=h_n.detach())
    out["dh0"] = h0.grad
    if identity_input:
        out["dgx"] = x.grad.reshape(B, T, dirs, G).permute(2, 0, 1, 3).contiguous()
        return out
    out["dx"] = x.grad
    for d in range(dirs):
        sfx = "_l0" + ("_reverse" if d else "")
        out[f"dW_ih{d}"], out[f"dW_hh{d}"] = getattr(m, "weight_ih" + sfx).grad, getattr(m, "weight_hh" + sfx).grad
        if bias:
            out[f"db_ih{d}"], out[f"db_hh{d}"] = getattr(m, "bias_ih" + sfx).grad, getattr(m, "bias_hh" + sfx).grad
    return out


def rel_err(got, want):
    """Largest difference relative to the reference tensor's largest entry."""
    want = want.double()
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()
