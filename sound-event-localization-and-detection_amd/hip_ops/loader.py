"""The device-resident epoch loader (csrc/loader.hip): the minibatch gather whose batch number lives in device memory,
the per-step running mean of the loss, and the epoch's sample order as torch's RandomSampler would draw it."""
import torch

from .. import _lib as L
from ._core import _req, timed

__all__ = ["gather_rows", "epoch_step_end", "epoch_permutation"]


def _rows(t, name):
    """(tensor, row length) of a contiguous fp32 device array (rows, ...); None passes."""
    if t is None:
        return None, 0
    if _req(t, name) is not t or t.dim() < 1:
        raise L.SeldHipError(f"{name}: expected a contiguous array of rows, got {tuple(t.shape)} contiguous={t.is_contiguous()}")
    return t, (t.numel() // t.shape[0] if t.shape[0] else 0)


def _scalar(t, name, dtype):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or t.numel() != 1:
        raise L.SeldHipError(f"{name}: expected a device tensor of one {dtype} element")
    return t


def gather_rows(x_all, y_all, index, out_x, out_y, *, cursor=None, start=0, count=None, stride=None):
    """out_x[b] = x_all[index[p + b]] and out_y[b] = y_all[index[p + b]] for b < count, in ONE launch (seld_gather_rows).

    x_all (n, ...), y_all (n, ...): the resident arrays; out_x (B, ...), out_y (B, ...): the batch buffers, all contiguous
    fp32 on one device; index: int64 device tensor.  Either pair may be None.  p = start, or with `cursor` (a device
    int32 of one element, read by the kernel: the launch can be recorded and fetches another batch at every replay)
    p = cursor * stride + start; stride defaults to B.  count defaults to B; rows [count, B) of the buffers are left
    alone.  A position outside `index` or an index outside [0, n) zero-fills its rows."""
    x_all, row_x = _rows(x_all, "gather_rows: x_all")
    y_all, row_y = _rows(y_all, "gather_rows: y_all")
    out_x, orow_x = _rows(out_x, "gather_rows: out_x")
    out_y, orow_y = _rows(out_y, "gather_rows: out_y")
    if (x_all is None) != (out_x is None) or (y_all is None) != (out_y is None):
        raise L.SeldHipError("gather_rows: an array and its batch buffer are given together or not at all")
    arrays = [t for t in (x_all, y_all) if t is not None]
    outs = [t for t in (out_x, out_y) if t is not None]
    if not arrays:
        raise L.SeldHipError("gather_rows: neither predictors nor targets given")
    if row_x != orow_x or row_y != orow_y:
        raise L.SeldHipError(f"gather_rows: row lengths of the arrays ({row_x}, {row_y}) and the buffers ({orow_x}, {orow_y}) differ")
    if len({t.shape[0] for t in arrays}) != 1 or len({t.shape[0] for t in outs}) != 1:
        raise L.SeldHipError("gather_rows: predictors and targets must have the same number of rows")
    if not torch.is_tensor(index) or not index.is_cuda or index.dtype != torch.int64 or not index.is_contiguous():
        raise L.SeldHipError("gather_rows: index must be a contiguous int64 device tensor")
    dev = arrays[0].device
    if any(t.device != dev for t in arrays + outs + [index]):
        raise L.SeldHipError("gather_rows: tensors on different devices")
    if cursor is not None and _scalar(cursor, "gather_rows: cursor", torch.int32).device != dev:
        raise L.SeldHipError("gather_rows: cursor on another device")
    B = outs[0].shape[0]
    count = B if count is None else int(count)
    stride = B if stride is None else int(stride)
    with torch.cuda.device(dev):
        with timed("gather_rows_kernel", lambda: (0.0, float(8 * count * (row_x + row_y)))):
            L.check(L.lib().seld_gather_rows(L.ptr(x_all), row_x, L.ptr(out_x), L.ptr(y_all), row_y, L.ptr(out_y),
                                             L.ptr(index), index.numel(), arrays[0].shape[0], L.ptr(cursor), stride,
                                             int(start), B, count, L.current_stream()), "seld_gather_rows")
    return out_x, out_y


def epoch_step_end(loss, mean, cursor):
    """mean += (loss - mean) / (cursor + 1); cursor += 1 on the device (seld_epoch_step_end): the running mean of
    train.main's epoch loop without a read-back.  loss, mean: fp32 device scalars; cursor: the int32 device scalar of gather_rows."""
    _scalar(loss, "epoch_step_end: loss", torch.float32)
    _scalar(mean, "epoch_step_end: mean", torch.float32)
    _scalar(cursor, "epoch_step_end: cursor", torch.int32)
    with torch.cuda.device(loss.device):
        L.check(L.lib().seld_epoch_step_end(L.ptr(loss), L.ptr(mean), L.ptr(cursor), L.current_stream()),
                "seld_epoch_step_end")


def epoch_permutation(n, generator=None):
    """The order in which torch.utils.data.RandomSampler (no replacement) visits n samples, as an int64 host tensor, from
    the same RNG state: without a generator the sampler draws ONE int64 seed from the default generator
    (`torch.empty((), dtype=torch.int64).random_()`) and permutes with a fresh generator seeded by it; with one, it
    permutes with that generator.  The default generator is consumed exactly as the sampler consumes it."""
    if generator is None:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        generator = torch.Generator()
        generator.manual_seed(seed)
    return torch.randperm(int(n), generator=generator)
