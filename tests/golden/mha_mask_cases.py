"""Cases of tests/golden/mha_mask.npz: MultiHeadAttention.forward(v, k, q, mask) with a mask and / or
key_len != query_len (model.py:25-51).  Shared by make_golden_mha_mask.py and the tests.

Inputs and masks are closed forms (no RNG): q, k, v and the cotangent from oracle.closed_form_input, the weights from
oracle.closed_form_fill_(amp=0.6).  hd = E / heads; MFMA marks the cases the matrix-core kernels run."""
import torch

from oracle.seld_oracle import closed_form_input

MHA_MASK_CASES = [
    # (N, 1, 1, Tk) bool key padding: sample 1 keeps its first 13 keys (VALU, hd = 6)
    dict(name="kpad_hd6", N=2, E=48, heads=8, Tq=20, Tk=20, mask="key_padding"),
    # (Tq, Tk) int64 causal (MFMA, hd = 16)
    dict(name="causal_hd16", N=2, E=32, heads=2, Tq=32, Tk=32, mask="causal"),
    # (N, heads, Tq, Tk) float with values other than 1, one fully masked query row and one fully masked (sample, head)
    dict(name="float_full_rows", N=2, E=24, heads=3, Tq=20, Tk=20, mask="float_full"),
    # (heads, Tq, Tk) uint8: the first dim lines up with the heads, as in the reference
    dict(name="heads3d", N=2, E=32, heads=4, Tq=18, Tk=18, mask="heads3d"),
    # cross-attention without a mask
    dict(name="cross_valu", N=2, E=48, heads=8, Tq=24, Tk=40, mask=None),
    dict(name="cross_mfma", N=2, E=32, heads=2, Tq=32, Tk=48, mask=None),
]


def mha_mask_inputs(c, dtype=torch.float32):
    """v, k (N, Tk, E) and q (N, Tq, E), the reference's (batch, length, embed) layout."""
    N, E, Tq, Tk = c["N"], c["E"], c["Tq"], c["Tk"]
    v = closed_form_input((N, Tk, E), dtype)
    k = 2.0 * closed_form_input((N, Tk, E), dtype).flip(2)
    q = 3.0 * closed_form_input((N, Tq, E), dtype).flip(1)
    return v, k, q


def mha_mask_cotangent(shape, dtype=torch.float32):
    return closed_form_input(tuple(shape), dtype).flip(1)


def mha_mask(c):
    """The case's mask on the CPU (None for the unmasked cases)."""
    N, H, Tq, Tk = c["N"], c["heads"], c["Tq"], c["Tk"]
    kind = c["mask"]
    if kind is None:
        return None
    if kind == "key_padding":
        m = torch.ones(N, 1, 1, Tk, dtype=torch.bool)
        m[1, ..., 13:] = False
        return m
    if kind == "causal":
        return torch.tril(torch.ones(Tq, Tk, dtype=torch.int64))
    if kind == "float_full":
        n, h, q, k = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(Tq), torch.arange(Tk), indexing="ij")
        code = (3 * n + 5 * h + 7 * q + 11 * k) % 5
        m = torch.where(code == 0, torch.zeros(()), 0.5 + code.to(torch.float32) * torch.where(k % 2 == 0, 1.0, -1.5))
        m[0, 1, 4, :] = 0.0            # one fully masked query row
        m[1, 2] = 0.0                  # one fully masked (sample, head)
        return m
    if kind == "heads3d":
        h, q, k = torch.meshgrid(torch.arange(H), torch.arange(Tq), torch.arange(Tk), indexing="ij")
        return ((h + 2 * q + 3 * k) % 3 != 0).to(torch.uint8)
    raise ValueError(kind)


def mha_core_reference(q, k, v, heads, mask=None):
    """float64 restatement of model.py:39-48 with a mask on (N, E, T) tensors: q (N, E, Tq), k, v (N, E, Tk)."""
    N, E, Tq = q.shape
    Tk = k.shape[2]
    hd = E // heads

    def split(t, T):
        return t.reshape(N, heads, hd, T).transpose(2, 3)          # (N, heads, T, hd)
    energy = split(q, Tq) @ split(k, Tk).transpose(2, 3)
    if mask is not None:
        energy = energy.masked_fill(mask == 0, -1e9)
    att = torch.softmax(energy / hd ** 0.5, dim=3)
    return (att @ split(v, Tk)).transpose(2, 3).reshape(N, E, Tq)
