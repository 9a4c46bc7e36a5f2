"""fp64 brute-force reference of the permutation-invariant SELD loss (include/seld_hip.h: seld_loss_pit_fwd_bwd) and
the input generator its tests share.  A helper, not a test: imported by tests/test_pit_loss_host.py (CPU) and
tests/test_gpu_pit_loss.py.

Everything is computed in fp64 from the fp32 inputs: the O x O pair costs of every (row, class) cell, all O! permutation
costs in lexicographic order summed in slot order, the first minimum, and from it loss, parts, gradients and perm.

A cell is AMBIGUOUS when some permutation that gives a different permuted target costs less than
AMBIGUOUS_REL * sum |P[o][j]| more than the best one: an fp32 evaluation may then legitimately choose the other target.
Permutations that only swap identical target slots are the same choice and never make a cell ambiguous.  1e-4 is about
100 times the fp32 error of a pair cost; it decides which cells the gradient and perm checks leave out and is not a
tolerance of the kernel."""
import itertools

import torch

AMBIGUOUS_REL = 1e-4


def permutations(overlaps):
    """Prediction slot -> target slot, in the index order of the C ABI (lexicographic)."""
    return list(itertools.permutations(range(overlaps)))


def split(sed, doa, target, classes, overlaps):
    """fp64 views (rows, C, O), (rows, C, O, 3), (rows, C, O), (rows, C, O, 3) of the project's layouts."""
    rows, n_sed = sed.shape[0], classes * overlaps
    assert sed.shape == (rows, n_sed) and doa.shape == (rows, 3 * n_sed) and target.shape == (rows, 4 * n_sed)
    return (sed.double().view(rows, classes, overlaps), doa.double().view(rows, classes, overlaps, 3),
            target[:, :n_sed].double().view(rows, classes, overlaps),
            target[:, n_sed:].double().view(rows, classes, overlaps, 3))


def pit_reference(sed, doa, target, classes, overlaps, w_sed=1.0, w_doa=5.0):
    """dict of loss (float), parts (2 floats), dsed (rows, n_sed), ddoa (rows, n_doa), perm (rows, C) int64, costs
    (rows, C, O!), and the boolean (rows, C) maps ambiguous / choice (some permutation changes the target) /
    distinct (target slots pairwise different) / moved (the chosen permuted target is not the target as given)."""
    s, d, ts, td = split(sed, doa, target, classes, overlaps)
    rows, C, O = s.shape
    a, b = w_sed / (rows * C * O), w_doa / (rows * 3 * C * O)
    l1, l0 = torch.log(s).clamp(min=-100.0), torch.log(1.0 - s).clamp(min=-100.0)
    # [r, c, o, j]
    bce = -(ts[:, :, None, :] * l1[..., None] + (1.0 - ts[:, :, None, :]) * l0[..., None])
    sq = ((d[:, :, :, None, :] - td[:, :, None, :, :]) ** 2).sum(-1)
    P = a * bce + b * sq
    perms = permutations(O)
    costs = []
    for pi in perms:
        c = P[:, :, 0, pi[0]]
        for o in range(1, O):
            c = c + P[:, :, o, pi[o]]
        costs.append(c)
    costs = torch.stack(costs, -1)
    best, perm = costs[..., 0].clone(), torch.zeros(rows, C, dtype=torch.int64)
    for k in range(1, len(perms)):
        better = costs[..., k] < best
        best = torch.where(better, costs[..., k], best)
        perm = torch.where(better, torch.full_like(perm, k), perm)
    full = torch.cat((ts[..., None], td), -1)                           # (rows, C, O, 4): a slot's whole target
    permuted = torch.stack([full[:, :, list(pi), :] for pi in perms], 2)  # (rows, C, O!, O, 4)
    chosen = torch.gather(permuted, 2, perm[:, :, None, None, None].expand(rows, C, 1, O, 4))[:, :, 0]
    other = (permuted != chosen[:, :, None]).flatten(3).any(-1)          # (rows, C, O!): a different permuted target
    near = costs - best[..., None] < AMBIGUOUS_REL * P.abs().sum((-1, -2))[..., None]
    t, u = chosen[..., 0], chosen[..., 1:]
    bce_c = -(t * l1 + (1.0 - t) * l0)
    sq_c = ((d - u) ** 2).sum(-1)
    distinct = torch.ones(rows, C, dtype=torch.bool)
    for i, j in itertools.combinations(range(O), 2):
        distinct &= (full[:, :, i] != full[:, :, j]).any(-1)
    return dict(loss=float(best.sum()), parts=(a * float(bce_c.sum()), b * float(sq_c.sum())),
                dsed=(a * (s - t) / (s * (1.0 - s)).clamp(min=1e-12)).reshape(rows, C * O),
                ddoa=(b * 2.0 * (d - u)).reshape(rows, 3 * C * O), perm=perm, costs=costs,
                ambiguous=(other & near).any(-1), choice=(permuted != permuted[:, :, :1]).flatten(3).any(-1).any(-1),
                distinct=distinct, moved=(chosen != full).flatten(2).any(-1))


def plain_reference(sed, doa, target, w_sed=1.0, w_doa=5.0):
    """The slot-bound loss in fp64 (tests/test_gpu_train_step.py: loss_reference): (loss, dsed, ddoa)."""
    rows, n_sed = sed.shape
    n_doa = doa.shape[1]
    s, d, t, td = sed.double(), doa.double(), target[:, :n_sed].double(), target[:, n_sed:].double()
    inv_s, inv_d = 1.0 / (rows * n_sed), 1.0 / (rows * n_doa)
    l1, l0 = torch.log(s).clamp(min=-100.0), torch.log(1.0 - s).clamp(min=-100.0)
    loss = w_sed * inv_s * float(-(t * l1 + (1.0 - t) * l0).sum()) + w_doa * inv_d * float(((d - td) ** 2).sum())
    return loss, w_sed * inv_s * (s - t) / (s * (1.0 - s)).clamp(min=1e-12), w_doa * inv_d * 2.0 * (d - td)


def permute_target(target, classes, overlaps, order):
    """target with the slots of every cell reordered: new slot o = old slot order[r, c, o].  order: (rows, C, O) int64."""
    rows, n_sed = target.shape[0], classes * overlaps
    ts = target[:, :n_sed].reshape(rows, classes, overlaps)
    td = target[:, n_sed:].reshape(rows, classes, overlaps, 3)
    ts = torch.gather(ts, 2, order)
    td = torch.gather(td, 2, order[..., None].expand(rows, classes, overlaps, 3))
    return torch.cat((ts.reshape(rows, n_sed), td.reshape(rows, 3 * n_sed)), 1).contiguous()


def random_orders(rows, classes, overlaps, gen):
    """A uniformly random slot permutation per cell, (rows, C, O) int64."""
    return torch.rand(rows, classes, overlaps, generator=gen).argsort(-1)


def pit_inputs(rows, classes, overlaps, seed):
    """fp32 (sed (rows, C*O), doa (rows, 3*C*O), target (rows, 4*C*O)).
    Active slots per cell: k = 0 with probability 0.6, else uniform in 1..O; the target fills slots 0..k-1 as the encoder
    does, active locations uniform in [-1, 1], inactive ones 0.  75 % of the cells are structured predictions -- the
    target under a uniformly random slot permutation, sed = 0.8 t + 0.1 + 0.05 N(0,1) clamped to [1e-4, 1 - 1e-4], doa =
    t + 0.1 N(0,1) -- the others unstructured: sed = sigmoid(4 N(0,1)), doa uniform in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    R, C, O = rows, classes, overlaps
    k = torch.where(torch.rand(R, C, generator=g) < 0.6, torch.zeros(R, C, dtype=torch.int64),
                    torch.randint(1, O + 1, (R, C), generator=g))
    ts = (torch.arange(O)[None, None, :] < k[..., None]).float()
    td = (torch.rand(R, C, O, 3, generator=g) * 2 - 1) * ts[..., None]
    order = random_orders(R, C, O, g)
    ps = torch.gather(ts, 2, order)
    pd = torch.gather(td, 2, order[..., None].expand(R, C, O, 3))
    sed_s = (0.8 * ps + 0.1 + 0.05 * torch.randn(R, C, O, generator=g)).clamp(1e-4, 1 - 1e-4)
    doa_s = pd + 0.1 * torch.randn(R, C, O, 3, generator=g)
    sed_u = torch.sigmoid(4 * torch.randn(R, C, O, generator=g))
    doa_u = torch.rand(R, C, O, 3, generator=g) * 2 - 1
    structured = torch.rand(R, C, generator=g) < 0.75
    sed = torch.where(structured[..., None], sed_s, sed_u)
    doa = torch.where(structured[..., None, None], doa_s, doa_u)
    target = torch.cat((ts.reshape(R, C * O), td.reshape(R, 3 * C * O)), 1)
    return sed.reshape(R, C * O).contiguous(), doa.reshape(R, 3 * C * O).contiguous(), target.contiguous()
