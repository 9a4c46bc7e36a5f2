"""torch.nn-shaped modules whose forward runs on the HIP kernels.

Each class subclasses the torch.nn module it stands in for, so constructor signatures, parameter /
buffer names, default initialisation (and therefore torch RNG consumption and state-dict layout)
are exactly those the reference gets from torch.nn (model.py:20-23, 81-107, 175-202, 276-282,
439-459).  Only `forward` is replaced.
"""
import torch
import torch.nn as nn

from . import _lib as L
from . import hip_ops as H


class Conv1d(nn.Conv1d):
    def forward(self, x):
        if self.groups != 1 and self.groups == self.in_channels and self.out_channels % self.in_channels == 0 \
                and self.padding_mode == "zeros" and not isinstance(self.padding, str):
            return H.depthwise_conv(x, self.weight, self.bias, self.stride, self.padding, self.dilation)
        if self.groups != 1 or self.padding_mode != "zeros" or isinstance(self.padding, str):
            raise L.SeldHipError("Conv1d: only groups=1 or groups=in_channels (depthwise), zero padding given as "
                                 "integers is supported")
        return H.hyper_conv(x, (self.weight,), self.bias, self.stride, self.padding, self.dilation)


class Conv2d(nn.Conv2d):
    def forward(self, x):
        if self.groups != 1 and self.groups == self.in_channels and self.out_channels % self.in_channels == 0 \
                and self.padding_mode == "zeros" and not isinstance(self.padding, str):
            return H.depthwise_conv(x, self.weight, self.bias, self.stride, self.padding, self.dilation)
        if self.groups != 1 or self.padding_mode != "zeros" or isinstance(self.padding, str):
            raise L.SeldHipError("Conv2d: only groups=1 or groups=in_channels (depthwise), zero padding given as "
                                 "integers is supported")
        return H.hyper_conv(x, (self.weight,), self.bias, self.stride, self.padding, self.dilation)


class Linear(nn.Linear):
    def forward(self, x):
        return H.hyper_linear(x, (self.weight,), self.bias, L.SELD_LIN_REAL)


class BatchNorm1d(nn.BatchNorm1d):
    def forward(self, x):
        return H.bn_act(x, self, L.SELD_ACT_NONE)


class BatchNorm2d(nn.BatchNorm2d):
    def forward(self, x):
        return H.bn_act(x, self, L.SELD_ACT_NONE)


class ReLU(nn.ReLU):
    def forward(self, x):
        return H.act(x, L.SELD_ACT_RELU)


class Tanh(nn.Tanh):
    def forward(self, x):
        return H.act(x, L.SELD_ACT_TANH)


class Sigmoid(nn.Sigmoid):
    def forward(self, x):
        return H.act(x, L.SELD_ACT_SIGMOID)


def _window(v, nd):
    if isinstance(v, (tuple, list)):
        return tuple(int(a) for a in v)
    return (int(v),) * nd


class MaxPool1d(nn.MaxPool1d):
    def forward(self, x):
        k = _window(self.kernel_size, 1)[0]
        s = _window(self.stride, 1)[0]
        if s != k or self.padding not in (0, (0,)) or self.ceil_mode:
            raise L.SeldHipError("MaxPool1d: only stride == kernel_size, no padding, floor mode")
        return H.maxpool(x, 1, k)


class MaxPool2d(nn.MaxPool2d):
    def forward(self, x):
        k = _window(self.kernel_size, 2)
        s = _window(self.stride, 2)
        if s != k or self.padding not in (0, (0, 0)) or self.ceil_mode:
            raise L.SeldHipError("MaxPool2d: only stride == kernel_size, no padding, floor mode")
        return H.maxpool(x, k[0], k[1])


class Dropout(nn.Dropout):
    def forward(self, x):
        return H.dropout(x, self.p, self.training)


class Dropout1d(nn.Dropout1d):
    """Zeroes whole channels of a (N, C, T) tensor (model.py:96-97)."""

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        mask = H.channel_dropout_mask(x.shape[0], x.shape[1], self.p, x.device)
        return H.RowScaleFn.apply(x, mask)


class SqueezeExcite(nn.Module):
    """Squeeze-and-excitation gate over `channels` channels of `components` (1, 4 or 8) contiguous hypercomplex component
    blocks: one gate per hypercomplex channel and sample, hidden width max(1, (channels // components) // reduction).
    fc1 / fc2 hold the two layers' parameters with torch.nn.Linear's default initialisation (drawn at construction from
    the global RNG); the forward is hip_ops.squeeze_excite on an (N, channels, *spatial) tensor."""

    def __init__(self, channels, reduction, components=1):
        super().__init__()
        if components not in H.SE_COMPONENTS:
            raise ValueError(f"components must be one of {H.SE_COMPONENTS}, got {components!r}")
        if int(reduction) < 1:
            raise ValueError(f"reduction must be at least 1, got {reduction!r}")
        if channels < components or channels % components:
            raise ValueError(f"{channels} channels are not a positive multiple of {components} components")
        self.channels, self.reduction, self.components = int(channels), int(reduction), int(components)
        self.gated = self.channels // self.components
        self.hidden = max(1, self.gated // self.reduction)
        self.fc1 = nn.Linear(self.gated, self.hidden)
        self.fc2 = nn.Linear(self.hidden, self.gated)

    def extra_repr(self):
        return f"channels={self.channels}, reduction={self.reduction}, components={self.components}"

    def forward(self, x):
        return H.squeeze_excite(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.components)


class TemporalAttention(nn.Module):
    """Temporal attention (AT) block on a (N, channels, T) tensor: y = x + out(read(qkv(x))), a single-head attention over
    the time axis with key width `key_size`, value width `value_size` and an index mask (none | causal | band of +-`band`
    frames; hip_ops.at_core).  qkv is a 1x1 convolution to 2 key_size + value_size channels with torch's default
    initialisation; out, a 1x1 convolution back to `channels`, starts at zero, so a fresh block is the identity and grows
    in from there.  Both run on the real 1x1 convolution path; out and the residual sum are one launch."""

    def __init__(self, channels, key_size, value_size, mask='causal', band=0):
        super().__init__()
        for name, w in (("channels", channels), ("key_size", key_size), ("value_size", value_size)):
            if isinstance(w, bool) or not isinstance(w, int) or w < 1:
                raise ValueError(f"{name} must be a positive integer, got {w!r}")
        if key_size > H.AT_MAX_WIDTH or value_size > H.AT_MAX_WIDTH:
            raise ValueError(f"key_size {key_size} / value_size {value_size}: the kernels hold at most {H.AT_MAX_WIDTH}")
        if mask not in H.AT_MASKS:
            raise ValueError(f"mask must be one of {', '.join(H.AT_MASKS)}, got {mask!r}")
        if isinstance(band, bool) or not isinstance(band, int) or band < 0 or (mask == 'band' and band < 1):
            raise ValueError(f"band must be a non-negative integer, and at least 1 with mask='band', got {band!r}")
        self.channels, self.key_size, self.value_size = channels, key_size, value_size
        self.mask, self.band = mask, band
        self.qkv = Conv1d(channels, 2 * key_size + value_size, 1)
        self.out = Conv1d(value_size, channels, 1)
        nn.init.zeros_(self.out.weight)
        nn.init.zeros_(self.out.bias)

    def extra_repr(self):
        return f"mask={self.mask}, band={self.band}"

    def forward(self, x, lengths=None):
        if x.dim() != 3 or x.shape[1] != self.channels:
            raise L.SeldHipError(f"TemporalAttention: expected (N, {self.channels}, T), got {tuple(x.shape)}")
        read = H.at_core(self.qkv(x), self.key_size, self.value_size, self.mask, self.band, lengths)
        return H.hyper_conv_add(read, (self.out.weight,), self.out.bias, x, self.out.stride, self.out.padding,
                                self.out.dilation)


def _swap01(x):
    """(A, B, C) -> (B, A, C), contiguous, as two transposes of the last two axes."""
    A, B, C = x.shape
    return H.transpose12(H.transpose12(x.reshape(1, A, B * C)).view(B, C, A))


class GRU(nn.GRU):
    """torch.nn.GRU on the HIP kernels (hip_ops.gru): same constructor, parameter names and initial draws, so state dicts
    go either way.  `forward(x, h0=None)` takes a batched 3-D x in the layout `batch_first` names and returns (y, h_n).
    The recurrent weights stay resident in one workgroup's registers, which bounds hidden_size by 128; packed
    variable-length sequences are not supported.  Dropout between the layers draws from the project's Philox stream: the
    distribution is torch's, the mask is not."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.hidden_size > H.GRU_MAX_HIDDEN:
            raise ValueError(f"GRU: hidden_size {self.hidden_size} > {H.GRU_MAX_HIDDEN}: the recurrent weights no longer "
                             "fit one workgroup's registers")

    def flatten_parameters(self):
        """Nothing to do: the kernels read every parameter where it lies (torch's version re-homes them for MIOpen)."""

    def forward(self, x, h0=None):
        if isinstance(x, nn.utils.rnn.PackedSequence):
            raise ValueError("GRU: PackedSequence input is not supported")
        if x.dim() != 3:
            raise L.SeldHipError(f"GRU: expected a batched 3-D input, got {tuple(x.shape)}")
        dirs = 2 if self.bidirectional else 1
        names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
        params = [[tuple(getattr(self, f"{n}_l{layer}{sfx}") if self.bias or n.startswith("weight") else None for n in names)
                   for sfx in ("", "_reverse")[:dirs]] for layer in range(self.num_layers)]
        if not self.batch_first:
            x = _swap01(x)
        y, h_n = H.gru(x, params, self.hidden_size, self.num_layers, dirs, h0, self.dropout, self.training)
        return (y if self.batch_first else _swap01(y)), h_n
