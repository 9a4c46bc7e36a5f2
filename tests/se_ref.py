"""Squeeze-and-excitation in fp64 on the CPU, written as the formulas of include/seld_hip.h (no autograd): the yardstick
of tests/test_se_host.py (which checks it against torch.autograd) and tests/test_gpu_squeeze_excite.py.

x (N, C, *spatial), A components, Cg = C / A, channel c = k Cg + g; w1 (Hd, Cg), b1 (Hd), w2 (Cg, Hd), b2 (Cg)."""
import torch

# the case table of the issue: (N, C, spatial, A, Hd), each the smallest shape that reaches one hazard
CASES = (
    (3, 8, (1,), 1, 1),            # S = 1, Hd = 1
    (2, 16, (51,), 4, 2),          # S % 4 != 0, below one wave's worth
    (3, 8, (52,), 8, 1),           # Cg = 1, 13 live lanes
    (1, 24, (1000,), 1, 3),        # N = 1, odd Hd, several trips per row
    (2, 8, (4099,), 4, 2),         # multi-trip row with a misaligned base and a 3-element tail
    (2, 320, (20,), 1, 40),        # more channels than threads in the excite workgroup, many short rows per workgroup
    (2, 16, (5, 13), 8, 2),        # 4-D input
    (5, 12, (260,), 4, 3),         # row count not a multiple of the four rows of a row-form workgroup
    (1, 4, (1023,), 1, 1),         # the last row length of the row form (SE_BLOCK_MIN_S - 1) ...
    (1, 4, (1024,), 4, 1),         # ... and the first of the block form
)
case_id = lambda c: "x".join(map(str, (c[0], c[1]) + tuple(c[2]))) + f"-A{c[3]}-H{c[4]}"


def make_case(case, seed=0, dtype=torch.float64):
    """Seeded inputs of a case: x and dy normal plus a per-channel offset (the sums do not hover around zero); b1 centres
    each hidden unit's pre-activation on +0.5 (even units) or -0.5 (odd units), so both sides of the ReLU occur wherever
    Hd >= 2; w2 and b2 spread s over about 0.02 .. 0.98 across the table."""
    N, C, spatial, A, Hd = case
    Cg = C // A
    g = torch.Generator().manual_seed(1000 + seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    off = rnd(1, C, *([1] * len(spatial)))
    x = rnd(N, C, *spatial) + 1.5 * off
    dy = 0.5 * rnd(N, C, *spatial) + 0.3 * rnd(1, C, *([1] * len(spatial)))
    w1 = rnd(Hd, Cg) * (1.5 / Cg ** 0.5)
    pre = (x.reshape(N, A, Cg, -1).mean(dim=(1, 3)) @ w1.T).mean(0)
    b1 = 0.1 * rnd(Hd) - pre + 0.5 * (1 - 2 * (torch.arange(Hd) % 2)).double()
    w2 = rnd(Cg, Hd) * (2.5 / Hd ** 0.5)
    b2 = 1.5 * rnd(Cg)
    return tuple(t.to(dtype) for t in (x, dy, w1, b1, w2, b2))


def _fold(t, N, A, Cg):
    """(N, C, S) -> (N, Cg): the sum over the A component blocks and over S."""
    return t.reshape(N, A, Cg, -1).sum(dim=(1, 3))


def se_forward(x, w1, b1, w2, b2, A):
    """dict(z, h, s, y) in the dtype of the inputs."""
    N, C = x.shape[:2]
    Cg = C // A
    S = x[0, 0].numel()
    z = _fold(x, N, A, Cg) / (A * S)
    h = torch.clamp(z @ w1.T + b1, min=0)
    s = 1.0 / (1.0 + torch.exp(-(h @ w2.T + b2)))
    gate = s.repeat(1, A).reshape(N, C, *([1] * (x.dim() - 2)))        # channel k Cg + g takes s[:, g]
    return dict(z=z, h=h, s=s, y=x * gate)


def se_backward(x, dy, w1, w2, z, h, s, A):
    """dict(q, dp2, dh, dz, dw1, db1, dw2, db2, dx) from the forward's z, h, s (so a caller can feed the fp32 values a
    kernel produced)."""
    N, C = x.shape[:2]
    Cg = C // A
    S = x[0, 0].numel()
    q = _fold(dy * x, N, A, Cg)
    dp2 = q * s * (1.0 - s)
    dh = (dp2 @ w2) * (h > 0).to(x.dtype)
    dz = dh @ w1
    shape = (N, C, *([1] * (x.dim() - 2)))
    dx = dy * s.repeat(1, A).reshape(shape) + (dz / (A * S)).repeat(1, A).reshape(shape)
    return dict(q=q, dp2=dp2, dh=dh, dz=dz, dw1=dh.T @ z, db1=dh.sum(0), dw2=dp2.T @ h, db2=dp2.sum(0), dx=dx)


def se_module_apply(sd, prefix, x, A):
    """hip_nn.SqueezeExcite with the parameters `prefix`.fc{1,2}.{weight,bias} of a state dict, differentiable."""
    N, C = x.shape[:2]
    z = x.reshape(N, A, C // A, -1).mean(dim=(1, 3))
    h = torch.relu(z @ sd[prefix + ".fc1.weight"].T + sd[prefix + ".fc1.bias"])
    s = torch.sigmoid(h @ sd[prefix + ".fc2.weight"].T + sd[prefix + ".fc2.bias"])
    return x * s.repeat(1, A).reshape(N, C, *([1] * (x.dim() - 2)))


def seld_forward_se(sd, cfg, x, train, mode="explicit"):
    """oracle.seld_forward for a single-stream model without dropout, with the squeeze-and-excitation modules the state
    dict holds: `...cnn.{i}.5` on each CNN stage's output, `...ResBlocks.{i}.se` on the gated y.  The layers are the
    oracle's own (its conv, BatchNorm, attention and heads); only the walk over them is restated here, since the oracle
    has no hook at these two points."""
    import torch.nn.functional as F
    from oracle import seld_oracle as O
    assert not cfg.two_stream
    A, p = cfg.algebra, "seld_block"
    cnn_bn = cfg.batch_norm in {"BN", "BN_on_CNN", "BNonCNN"}
    tcn_bn = cfg.batch_norm in {"BN", "BN_on_TCN", "BNonTCN"}
    for i, pool in enumerate(cfg.pool_size[:len(cfg.cnn_filters)]):
        x = O._conv_layer(sd, f"{p}.cnn.{i}.0", A, x, 1, 1, 1, mode)
        if cnn_bn:
            x = O._bn(sd, f"{p}.cnn.{i}.1", x, train, None)
        x = F.max_pool2d(torch.relu(x), [pool[0], pool[1]] if cfg.pool_time == "CNN" else [pool[0], 1])
        if f"{p}.cnn.{i}.5.fc1.weight" in sd:
            x = se_module_apply(sd, f"{p}.cnn.{i}.5", x, A)
    B = x.shape[0]
    x = x.permute(0, 3, 1, 2).reshape(B, x.shape[3], -1).permute(0, 2, 1)
    t = p + ".tcn"
    k = cfg.kernel_size_dilated_conv
    skip_sum = None
    for bi, d in enumerate(O.dilations(cfg)):
        b = f"{t}.ResBlocks.{bi}"
        pad = int(((k - 1) * d) / 2)
        if tcn_bn:
            x = torch.tanh(O._bn(sd, b + ".batch_filter1", x, train, None))
        yf = O._conv_layer(sd, b + ".conv1_filter", A, x, 1, pad, d, mode)
        yg = O._conv_layer(sd, b + ".conv1_gate", A, x, 1, pad, d, mode)
        if tcn_bn:
            yf, yg = O._bn(sd, b + ".batch_filter2", yf, train, None), O._bn(sd, b + ".batch_gate2", yg, train, None)
        y = torch.tanh(yf) * torch.sigmoid(yg)
        if b + ".se.fc1.weight" in sd:
            y = se_module_apply(sd, b + ".se", y, A)
        skip = O._conv_layer(sd, b + ".conv2_skip", A, y, 1, 0, 1, mode)
        x = x + O._conv_layer(sd, b + ".conv2_residual", A, y, 1, 0, 1, mode)
        skip_sum = skip if skip_sum is None else skip_sum + skip
    out = torch.relu(skip_sum)
    tcn_pool = cfg.pool_time == "TCN"
    if tcn_pool:
        out = F.max_pool1d(out, cfg.pool_size[0][1])
    out = O._conv_layer(sd, t + ".conv1", A, out, 1, 1, 1, mode)
    a = t + ".attention"
    out = O.multi_head_attention(out.permute(0, 2, 1), sd[a + ".queries.weight"], sd[a + ".keys.weight"],
                                 sd[a + ".values.weight"], sd[a + ".fc_out.weight"], sd[a + ".fc_out.bias"],
                                 num_heads=8).permute(0, 2, 1)
    out = torch.relu(out)
    if tcn_pool:
        out = F.max_pool1d(out, cfg.pool_size[1][1])
    out = torch.tanh(O._conv_layer(sd, t + ".conv2", A, out, 1, 1, 1, mode))
    if tcn_pool:
        out = F.max_pool1d(out, cfg.pool_size[2][1])
    feat = out.permute(0, 2, 1)
    return torch.sigmoid(O._head(sd, "sed", cfg, feat, mode)), torch.tanh(O._head(sd, "doa", cfg, feat, mode))
