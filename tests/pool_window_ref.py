"""The pooling decision of the first stage on the host (no GPU): which row of a MaxPool2d(pool, 1) window the pooling
convolution keeps.  relu(gamma invstd (y - mean) + beta) is largest where sign(gamma) * y is, so the kernel looks at the
convolution output alone: the FIRST row at which sign(gamma) * y is largest, and row 0 for gamma == 0 (everything ties).
Shared by tests/test_gpu_hcq_first_pool_exact.py and tests/first_stage_exact.py."""
import torch


def bn_inputs(C, gen):
    """gamma in {-2 .. 2} with a positive, a negative and a zero channel in every group of 8 (their places move with the
    group); mean, beta integers in [-2, 2]; invstd in {0.5, 1, 2}."""
    gamma = torch.randint(-2, 3, (C,), generator=gen).float().view(C // 8, 8)
    for g in range(C // 8):
        gamma[g, g % 8], gamma[g, (g + 3) % 8], gamma[g, (g + 5) % 8] = 1 + g % 2, -1 - (g // 2) % 2, 0
    mean, beta = (torch.randint(-2, 3, (C,), generator=gen).float() for _ in range(2))
    invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=gen)]
    return {"gamma": gamma.view(C), "mean": mean, "beta": beta, "invstd": invstd}


def window_rows(o, gamma, pool):
    """o: float64 (N, C, H, W) convolution output, gamma: (C,).  Returns (raw, idx, ties): the window value and its row,
    both (N, C, H // pool, W) -- idx as int64 --, and the number of windows with more than one maximal row."""
    N, C, H, Wd = o.shape
    win = o.view(N, C, H // pool, pool, Wd)
    key = torch.sign(gamma).double().view(1, C, 1, 1, 1) * win
    best = key.max(dim=3, keepdim=True).values
    idx = ((key == best).cumsum(3) == 0).sum(3)                          # rows before the first maximum
    raw = win.gather(3, idx.unsqueeze(3)).squeeze(3)
    return raw, idx, int(((key == best).sum(3) > 1).sum())


def bn_relu(raw, gamma, beta, mean, invstd):
    """relu(a raw + b) in float64 with a = gamma invstd, b = beta - mean a (per channel, dim 1)."""
    C = raw.shape[1]
    a = (gamma * invstd).double()
    b = beta.double() - mean.double() * a
    return torch.relu(a.view(1, C, 1, 1) * raw + b.view(1, C, 1, 1))
