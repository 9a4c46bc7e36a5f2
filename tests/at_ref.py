"""Temporal attention in fp64 on the CPU, written as the formulas of include/seld_hip.h (dense, no autograd): the yardstick
of tests/test_at_host.py (which checks it against torch.autograd) and tests/test_gpu_temporal_attention.py.

qkv (N, 2K + V, T) = [q (K) | k (K) | v (V)]; score[n,t,s] = q[n,:,t] . k[n,:,s] / sqrt(K); allowed(n,t,s) = kind(t, s) and
s < len[n]; excluded keys weigh exactly 0; a row with no allowed key reads 0, has lse = +inf and no gradient."""
import math

import torch

# the case table of the issue: (N, K, V, T, mask, W, lengths), each the smallest shape that reaches one hazard
CASES = (
    (1, 1, 1, 1, "none", 0, None),                  # 1  T = 1
    (2, 3, 5, 37, "causal", 0, None),               # 2  odd widths on VALU, T not a multiple of any tile
    (2, 16, 16, 64, "causal", 0, None),             # 3  MFMA, K == V
    (1, 16, 48, 80, "band", 1, None),               # 4  narrowest band
    (2, 32, 16, 144, "band", 16, None),             # 5  band edge on a 16-row boundary
    (1, 64, 64, 96, "band", 17, None),              # 6  band edge one past a 16-row boundary
    (2, 16, 32, 130, "none", 0, None),              # 7  MFMA widths but T % 16 != 0, so VALU
    (3, 16, 64, 128, "causal", 0, (128, 5, 77)),    # 8  per-sample lengths
    (2, 8, 12, 40, "band", 3, (40, 5)),             # 9  rows t >= 8 of sample 1 (t - 3 > 4) have no allowed key
    (1, 48, 16, 272, "band", 64, None),             # 10 whole key tiles skipped on both sides
    (1, 16, 16, 512, "causal", 0, None),            # 11 the model's own length
    (1, 16, 16, 1040, "band", 200, None),           # 12 multi-tile band
)
MFMA_CASES = (3, 4, 5, 6, 8, 10, 11, 12)            # 1-based numbers of the cases the fp32-MFMA kernels serve


def case_id(case):
    N, K, V, T, mask, W, lengths = case
    return f"{N}x{K}x{V}x{T}-{mask}" + (f"{W}" if mask == "band" else "") + ("-len" if lengths else "")


def make_case(case, seed=0, dtype=torch.float64):
    """Seeded (qkv, dread) of a case.  As in tests/test_gpu_mha_mask.py one key column is scaled by 6 in a later tile, so
    the online-softmax rescale is exercised."""
    N, K, V, T, _, _, _ = case
    g = torch.Generator().manual_seed(2000 + seed)
    qkv = torch.randn(N, 2 * K + V, T, generator=g, dtype=torch.float64)
    qkv[:, K:2 * K, min(T - 1, T // 2 + 7)] *= 6.0
    dread = torch.randn(N, V, T, generator=g, dtype=torch.float64)
    return qkv.to(dtype), dread.to(dtype)


def allowed(N, T, mask, W=0, lengths=None):
    """(N, T, T) bool: [n, t, s] is True where query t of sample n may attend key s."""
    t = torch.arange(T).view(T, 1)
    s = torch.arange(T).view(1, T)
    if mask == "none":
        kind = torch.ones(T, T, dtype=torch.bool)
    elif mask == "causal":
        kind = s <= t
    elif mask == "band":
        kind = (t - s).abs() <= W
    else:
        raise ValueError(mask)
    length = torch.full((N,), T) if lengths is None else torch.as_tensor(lengths).clamp(1, T)
    return kind.unsqueeze(0) & (s.unsqueeze(0) < length.view(N, 1, 1))


def at_forward(qkv, K, V, mask, W=0, lengths=None):
    """dict(p (N, T, T), read (N, V, T), lse (N, T)) in the dtype of qkv."""
    N, _, T = qkv.shape
    q, k, v = qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:]
    ok = allowed(N, T, mask, W, lengths)
    score = torch.einsum("ndt,nds->nts", q, k) / math.sqrt(K)
    score = torch.where(ok, score, torch.full_like(score, -math.inf))
    m = score.max(dim=2, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)            # a row with no allowed key: every e is exp(-inf) = 0
    e = torch.exp(score - m)
    l = e.sum(dim=2, keepdim=True)
    dead = l == 0
    p = torch.where(dead, torch.zeros_like(e), e / torch.where(dead, torch.ones_like(l), l))
    lse = torch.where(dead, torch.full_like(l, math.inf), m + torch.log(torch.where(dead, torch.ones_like(l), l))).squeeze(2)
    return dict(p=p, read=torch.einsum("nts,nds->ndt", p, v), lse=lse)


def at_backward(qkv, dread, K, V, p, read):
    """dqkv (N, 2K + V, T) from the forward's p and read: delta = sum_d dread read, ds = p (dp - delta) / sqrt(K)."""
    q, k, v = qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:]
    delta = (dread * read).sum(dim=1)                                  # (N, T)
    dp = torch.einsum("ndt,nds->nts", dread, v)
    ds = p * (dp - delta.unsqueeze(2)) / math.sqrt(K)
    dq = torch.einsum("nts,nds->ndt", ds, k)
    dk = torch.einsum("nts,ndt->nds", ds, q)
    dv = torch.einsum("nts,ndt->nds", p, dread)
    return torch.cat((dq, dk, dv), dim=1)


def at_dense_autograd(qkv, K, V, mask, W=0, lengths=None):
    """read by torch ops that autograd follows (masked_fill + softmax; rows with no allowed key zeroed)."""
    N, _, T = qkv.shape
    q, k, v = qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:]
    ok = allowed(N, T, mask, W, lengths)
    score = (q.transpose(1, 2) @ k) / math.sqrt(K)
    live = ok.any(dim=2, keepdim=True)
    score = score.masked_fill(~ok & live, -math.inf)                   # dead rows keep finite scores and are zeroed below
    p = torch.softmax(score, dim=2) * (ok & live).to(qkv.dtype)
    return (p @ v.transpose(1, 2)).transpose(1, 2)


def at_module_apply(sd, prefix, x, mask="causal", W=0, lengths=None):
    """hip_nn.TemporalAttention with the parameters `prefix`.{qkv,out}.{weight,bias} of a state dict, differentiable:
    y = x + out(read(qkv(x))).  The widths come from the weights' shapes."""
    wq, bq = sd[prefix + ".qkv.weight"], sd[prefix + ".qkv.bias"]
    wo, bo = sd[prefix + ".out.weight"], sd[prefix + ".out.bias"]
    V = wo.shape[1]
    K = (wq.shape[0] - V) // 2
    qkv = torch.einsum("oc,nct->not", wq[:, :, 0], x) + bq.view(1, -1, 1)
    read = at_dense_autograd(qkv, K, V, mask, W, lengths)
    return x + torch.einsum("oc,nct->not", wo[:, :, 0], read) + bo.view(1, -1, 1)


def stack_starts(D):
    """Index of the first residual block of every dilation stack (an entry of D; an explicit list is one stack)."""
    out, first = [], 0
    for stack in D:
        n = len(stack) if isinstance(stack, list) else int(stack)
        if n > 0:
            out.append(first)
        first += n
    return out


def seld_forward_at(sd, cfg, x, train, mask="causal", W=0, mode="explicit"):
    """oracle.seld_forward for a single-stream model without dropout, with the temporal-attention blocks the state dict
    holds: `...tcn.at.{j}` on the residual stream in front of the first residual block of dilation stack j.  The layers
    are the oracle's own (its conv, BatchNorm, attention and heads); only the walk over them is restated here, since the
    oracle has no hook at this point (tests/se_ref.py::seld_forward_se is the same walk with its own hooks)."""
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
    B = x.shape[0]
    x = x.permute(0, 3, 1, 2).reshape(B, x.shape[3], -1).permute(0, 2, 1)
    t = p + ".tcn"
    k = cfg.kernel_size_dilated_conv
    at_before = {first: j for j, first in enumerate(stack_starts(cfg.D))} if f"{t}.at.0.qkv.weight" in sd else {}
    skip_sum = None
    for bi, d in enumerate(O.dilations(cfg)):
        if bi in at_before:
            x = at_module_apply(sd, f"{t}.at.{at_before[bi]}", x, mask, W)
        b = f"{t}.ResBlocks.{bi}"
        pad = int(((k - 1) * d) / 2)
        x_hat = torch.tanh(O._bn(sd, b + ".batch_filter1", x, train, None)) if tcn_bn else x
        yf = O._conv_layer(sd, b + ".conv1_filter", A, x_hat, 1, pad, d, mode)
        yg = O._conv_layer(sd, b + ".conv1_gate", A, x_hat, 1, pad, d, mode)
        if tcn_bn:
            yf, yg = O._bn(sd, b + ".batch_filter2", yf, train, None), O._bn(sd, b + ".batch_gate2", yg, train, None)
        y = torch.tanh(yf) * torch.sigmoid(yg)
        skip = O._conv_layer(sd, b + ".conv2_skip", A, y, 1, 0, 1, mode)
        x = x_hat + O._conv_layer(sd, b + ".conv2_residual", A, y, 1, 0, 1, mode)
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
