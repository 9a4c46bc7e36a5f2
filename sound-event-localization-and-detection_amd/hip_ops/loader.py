"""The device-resident epoch loader (csrc/loader.hip): the minibatch gather whose batch number lives in device memory,
with or without augmentation on the way (signed channel permutations of first-order Ambisonics with their DOA labels,
frequency and time masks), the per-step running mean of the loss, and the epoch's sample order as torch's RandomSampler
would draw it."""
import dataclasses
import functools
import itertools
import weakref

import numpy as np
import torch

from .. import _lib as L
from ._core import _req, timed

__all__ = ["gather_rows", "gather_rows_aug", "gather_rows_rot", "gather_rows_polar", "gather_rows_mix", "target_occupancy", "Augment",
           "foa_transforms", "foa_triples", "foa_polar", "epoch_step_end", "epoch_permutation"]
AUG_MAX_CHANNELS, AUG_MAX_TRANSFORMS, ROT_MAX_TRIPLES, POLAR_MAX_GROUPS = 16, 64, 5, 2
MIX_MAX_CLASSES, MIX_MAX_OVERLAPS = 64, 8


def _rows(t, what, name):
    """(tensor, row length) of a contiguous fp32 device array (rows, ...); None passes.  The label of an error is put
    together only when there is one: this runs at every fetch."""
    if t is None:
        return None, 0
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() >= 1):
        _req(t, f"{what}: {name}")              # a host tensor or another dtype: its message
        raise L.SeldHipError(f"{what}: {name}: expected a contiguous array of rows, got {tuple(t.shape)} contiguous={t.is_contiguous()}")
    return t, (t.numel() // t.shape[0] if t.shape[0] else 0)


def _scalar(t, what, name, dtype):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or t.numel() != 1:
        raise L.SeldHipError(f"{what}: {name}: expected a device tensor of one {dtype} element")
    return t


def _gather_args(what, x_all, y_all, index, out_x, out_y, cursor, start, count, stride):
    """The checks every gather makes: (x_all, y_all, out_x, out_y, dev, count, bytes moved, lead), `lead` being the arguments
    every entry point of the C ABI starts with."""
    x_all, row_x = _rows(x_all, what, "x_all")
    y_all, row_y = _rows(y_all, what, "y_all")
    out_x, orow_x = _rows(out_x, what, "out_x")
    out_y, orow_y = _rows(out_y, what, "out_y")
    if (x_all is None) != (out_x is None) or (y_all is None) != (out_y is None):
        raise L.SeldHipError(f"{what}: an array and its batch buffer are given together or not at all")
    arrays = [t for t in (x_all, y_all) if t is not None]
    outs = [t for t in (out_x, out_y) if t is not None]
    if not arrays:
        raise L.SeldHipError(f"{what}: neither predictors nor targets given")
    if row_x != orow_x or row_y != orow_y:
        raise L.SeldHipError(f"{what}: row lengths of the arrays ({row_x}, {row_y}) and the buffers ({orow_x}, {orow_y}) differ")
    if len({t.shape[0] for t in arrays}) != 1 or len({t.shape[0] for t in outs}) != 1:
        raise L.SeldHipError(f"{what}: predictors and targets must have the same number of rows")
    if not torch.is_tensor(index) or not index.is_cuda or index.dtype != torch.int64 or not index.is_contiguous():
        raise L.SeldHipError(f"{what}: index must be a contiguous int64 device tensor")
    dev = arrays[0].device
    if any(t.device != dev for t in arrays + outs + [index]):
        raise L.SeldHipError(f"{what}: tensors on different devices")
    if cursor is not None and _scalar(cursor, what, "cursor", torch.int32).device != dev:
        raise L.SeldHipError(f"{what}: cursor on another device")
    B = outs[0].shape[0]
    count = B if count is None else int(count)
    stride = B if stride is None else int(stride)
    lead = (L.ptr(x_all), row_x, L.ptr(out_x), L.ptr(y_all), row_y, L.ptr(out_y), L.ptr(index), index.numel(), arrays[0].shape[0],
            L.ptr(cursor), stride, int(start), B, count)
    return x_all, y_all, out_x, out_y, dev, count, float(8 * count * (row_x + row_y)), lead


def _launch(what, g, own=()):
    """seld_<what>(lead, own, stream) under the timer label <what>_kernel; returns the two batch buffers."""
    _, _, out_x, out_y, dev, _, nbytes, lead = g
    with torch.cuda.device(dev):
        with timed(what + "_kernel", lambda: (0.0, nbytes)):
            L.check(getattr(L.lib(), "seld_" + what)(*lead, *own, L.current_stream()), "seld_" + what)
    return out_x, out_y


def gather_rows(x_all, y_all, index, out_x, out_y, *, cursor=None, start=0, count=None, stride=None):
    """out_x[b] = x_all[index[p + b]] and out_y[b] = y_all[index[p + b]] for b < count, in ONE launch (seld_gather_rows).

    x_all (n, ...), y_all (n, ...): the resident arrays; out_x (B, ...), out_y (B, ...): the batch buffers, all contiguous
    fp32 on one device; index: int64 device tensor.  Either pair may be None.  p = start, or with `cursor` (a device
    int32 of one element, read by the kernel: the launch can be recorded and fetches another batch at every replay)
    p = cursor * stride + start; stride defaults to B.  count defaults to B; rows [count, B) of the buffers are left
    alone.  A position outside `index` or an index outside [0, n) zero-fills its rows."""
    return _launch("gather_rows", _gather_args("gather_rows", x_all, y_all, index, out_x, out_y, cursor, start, count, stride))


_AXES = "XYZ"
_LAYOUTS = ("magphase", "quaternion", "iv", "logpower_iv")


def _axis_positions(what, order, mics):
    """[position of X, of Y, of Z in a 4-channel block] after the checks every preset makes of `order` and `mics`."""
    order = str(order).upper()
    if sorted(order) != sorted("W" + _AXES):
        raise L.SeldHipError(f"{what}: order must name W, X, Y and Z once each, got {order!r}")
    if mics not in (1, 2):
        raise L.SeldHipError(f"{what}: 1 or 2 microphones, got {mics}")
    return [order.index(ch) for ch in _AXES]


def _intensity_channels(what, order, mics, layout):
    """[[channel of the x, y, z intensity component] per microphone] of an intensity layout, after the checks the layouts
    share: `order` names a group [W, D1, D2, D3] as hip_ops.spatial_features reads it, so W comes first."""
    if layout not in _LAYOUTS:
        raise L.SeldHipError(f"{what}: layout is one of {', '.join(_LAYOUTS)}, got {layout!r}")
    pos = _axis_positions(what, order, mics)
    if 0 in pos:
        raise L.SeldHipError(f"{what}: the {layout} layout is made of groups [W, D1, D2, D3]: order starts with W, "
                             f"got {str(order).upper()!r}")
    if layout == "quaternion":
        return [[4 * g + p for p in pos] for g in range(mics)]
    base = 4 * mics if layout == "logpower_iv" else 0
    return [[base + 3 * g + p - 1 for p in pos] for g in range(mics)]   # which of I1, I2, I3 is the component along an axis


def foa_triples(order="WYZX", mics=1, layout="quaternion"):
    """The channel triples (cx, cy, cz) of `Augment(rot_triples=...)` for the layouts in which every directional channel is
    an intensity component: 'quaternion' (C = 4 * mics, per microphone [log-power W, I1, I2, I3]) and 'iv' (C = 3 * mics).
    One triple per microphone; `order` says which of X, Y, Z the components are.  'magphase' and 'logpower_iv' are
    refused: a magnitude, a phase or the log-power of a directional channel is not covariant under a general rotation
    (magnitude and phase TOGETHER are: `foa_polar`, `gather_rows_polar`)."""
    if layout in ("magphase", "logpower_iv"):
        raise L.SeldHipError(f"foa_triples: a rotation is not defined on the {layout} layout (it holds directional channels "
                             "that are no intensity components)")
    return [tuple(t) for t in _intensity_channels("foa_triples", order, mics, layout)]


def foa_polar(order="WYZX", mics=1):
    """The channel groups (mx, my, mz, px, py, pz) of `Augment(rot_polar=...)` for magnitude-phase predictors in the layout
    [magnitude mic A | magnitude mic B | phase mic A | phase mic B] (C = 8 * mics: what `foa_transforms(phase=True)` and
    data.normalize_dataset assume): magnitude and phase channel of the x, y and z axis, one group per microphone.
    `order` names the channels of a 4-channel block; W may sit anywhere in it and is in no group (it is copied)."""
    pos = _axis_positions("foa_polar", order, mics)
    return [tuple(4 * g + p for p in pos) + tuple(4 * (mics + g) + p for p in pos) for g in range(mics)]


def foa_transforms(order="WYZX", mics=1, phase=False, elevation=True, layout="magphase"):
    """The preset transform table of first-order Ambisonics predictors for `Augment`, on the host: int32 (K, 2 * C + 6),
    a row = src[C], flip[C], axis[3], sign[3] (include/seld_hip.h, seld_gather_rows_aug).

    The rows are the signed axis permutations generated by x <-> y, x -> -x, y -> -y and z -> -z: rotations and
    reflections of the sound field that keep the z axis vertical, 16 of them, or the 8 with z fixed when `elevation` is
    False.  The identity is row 0.  A row says for the DOA label  location'[a] = sign[a] * location[axis[a]]  (axes
    x, y, z = 0, 1, 2) and does the same to the directional channels of every microphone's 4-channel block: the channel
    of axis a becomes sign[a] times the channel of axis[a]; W stays.  `order` names the channels of a block.

    Channel layout, as data.normalize_dataset assumes: [magnitude mic A | magnitude mic B | phase mic A | phase mic B]
    (the second microphone with mics == 2, the phase half with phase=True), C = 4 * mics * (2 if phase else 1).
    Magnitude channels get flip 0 (a magnitude has no sign).  Phase channels get flip 2 where the sign is -1: the
    phase turned by pi.  Flip 2 is valid on RAW phase only, values in (-pi, pi]; on standardised phase it is wrong,
    and train.main refuses that combination.  With two spaced microphones one rotation for both blocks is an
    approximation (the arrays do not share a centre): the caller chooses it by passing mics=2.

    `layout` other than 'magphase': the same rows, in the same order, for the channel layouts hip_ops.spatial_features
    writes for `mics` groups [W, D1, D2, D3] (`order` starts with W; `phase` is refused):
      'quaternion'   C = 4 * mics, per microphone [log-power W, I1, I2, I3]
      'iv'           C = 3 * mics, per microphone [I1, I2, I3]
      'logpower_iv'  C = 7 * mics, the 4 * mics log-power planes, then the intensity planes group by group
    An intensity component is a signed quantity: its channel gets flip 1 (negate) where the sign is -1.  Log-power
    planes are permuted like magnitudes, flip 0."""
    # what a row moves: (the channels of the x, y, z axis, the flip of one whose sign is -1)
    if layout == "magphase":
        pos = _axis_positions("foa_transforms", order, mics)
        blocks = mics * (2 if phase else 1)
        C = 4 * blocks
        moved = [([4 * blk + p for p in pos], 2 if blk >= mics else 0) for blk in range(blocks)]     # blocks >= mics hold phases
    else:
        moved = [(t, 1) for t in _intensity_channels("foa_transforms", order, mics, layout)]
        if phase:
            raise L.SeldHipError(f"foa_transforms: the {layout!r} layout has no phase channels")
        C = {"quaternion": 4, "iv": 3, "logpower_iv": 7}[layout] * mics
        if layout == "logpower_iv":
            pos = _axis_positions("foa_transforms", order, mics)
            moved += [([4 * g + p for p in pos], 0) for g in range(mics)]
    rows = []
    for swap, sz, sy, sx in itertools.product((False, True), (1, -1) if elevation else (1,), (1, -1), (1, -1)):
        axis, sign = ([1, 0, 2] if swap else [0, 1, 2]), [sx, sy, sz]
        src, flip = list(range(C)), [0] * C
        for chans, turned in moved:
            for a in range(3):
                src[chans[a]] = chans[axis[a]]
                flip[chans[a]] = turned if sign[a] < 0 else 0
        rows.append(src + flip + axis + sign)
    return np.asarray(rows, dtype=np.int32)


def _check_table(table, channels):
    """Validated int32 host copy (K, 2 * C + 6) of a transform table; raises SeldHipError on anything the kernel must
    not see."""
    t = np.asarray(table.cpu() if torch.is_tensor(table) else table)
    if t.ndim != 2 or t.shape[1] < 8 or (t.shape[1] - 6) % 2 or not np.issubdtype(t.dtype, np.integer):
        raise L.SeldHipError(f"Augment: the table must be an integer array (K, 2 * C + 6), got {t.dtype} {t.shape}")
    K, C = t.shape[0], (t.shape[1] - 6) // 2
    if channels is not None and int(channels) != C:
        raise L.SeldHipError(f"Augment: the table is for {C} channels, not {channels}")
    if not 1 <= K <= AUG_MAX_TRANSFORMS or not 1 <= C <= AUG_MAX_CHANNELS:
        raise L.SeldHipError(f"Augment: 1..{AUG_MAX_TRANSFORMS} transforms of 1..{AUG_MAX_CHANNELS} channels, got {K} of {C}")
    src, flip, axis, sign = t[:, :C], t[:, C:2 * C], t[:, 2 * C:2 * C + 3], t[:, 2 * C + 3:]
    if src.min() < 0 or src.max() >= C:
        raise L.SeldHipError(f"Augment: a source channel outside [0, {C})")
    if flip.min() < 0 or flip.max() > 2:
        raise L.SeldHipError("Augment: a flip outside {0, 1, 2}")
    if not (np.sort(axis, axis=1) == np.arange(3)).all():
        raise L.SeldHipError("Augment: axis must be a permutation of 0, 1, 2 in every row")
    if not (np.abs(sign) == 1).all():
        raise L.SeldHipError("Augment: a sign that is not +1 or -1")
    return np.ascontiguousarray(t, dtype=np.int32)


def _check_channel_sets(sets, name, width, max_sets):
    """((c, ...), ...) of 1..max_sets channel sets of `width` entries each, the value of the Augment field `name`; raises
    SeldHipError unless they are distinct channels in [0, 16)."""
    kind = {3: "triples (cx, cy, cz)", 6: "groups (mx, my, mz, px, py, pz)"}[width]
    t = np.asarray(sets.cpu() if torch.is_tensor(sets) else sets)
    if t.ndim != 2 or t.shape[1] != width or not 1 <= t.shape[0] <= max_sets or not np.issubdtype(t.dtype, np.integer):
        raise L.SeldHipError(f"Augment: {name} must be 1..{max_sets} integer {kind}, got {t.dtype} {t.shape}")
    if t.min() < 0 or t.max() >= AUG_MAX_CHANNELS:
        raise L.SeldHipError(f"Augment: a {name} channel outside [0, {AUG_MAX_CHANNELS})")
    if len(set(t.ravel().tolist())) != t.size:
        raise L.SeldHipError(f"Augment: a channel appears twice in {name}")
    return tuple(tuple(int(c) for c in row) for row in t)


@functools.lru_cache(maxsize=None)
def _least_channels(sets):
    """The least number of channels the sets need, None without sets."""
    return None if sets is None else 1 + max(max(s) for s in sets)


@functools.lru_cache(maxsize=None)
def _packed(sets):
    """Channel sets as the C ABI takes them: 4 bits per entry."""
    return sum(c << (4 * i) for i, c in enumerate(c for s in sets for c in s))


@dataclasses.dataclass(frozen=True)
class Augment:
    """What seld_gather_rows_aug applies to every sample (include/seld_hip.h has the draws).

    table: a transform table (K, 2 * C + 6), e.g. `foa_transforms(...)`, or None for no channel transform; it is
    validated here and held as an int32 tensor on `device`.  p_swap: probability that a sample takes one of the K
    transforms (uniformly).  freq_masks / time_masks: 0, 1 or 2 masks per sample of a width drawn uniformly from
    [0, freq_width] / [0, time_width], filled with `fill`.  A bad table or range raises SeldHipError.

    What seld_gather_rows_rot applies (hip_ops.gather_rows_rot): p_rot, the probability that a sample's sound field is
    rotated about the vertical axis by a uniform angle, mirrored in y with probability 1/2 if rot_mirror and in z with
    probability 1/2 if rot_zflip; rot_triples, 1..5 channel triples (cx, cy, cz) of intensity vectors, e.g.
    `foa_triples(...)`, held as a tuple of tuples.  p_rot > 0 needs triples and excludes p_swap > 0 (the rotations with
    mirror and z-flip contain the signed permutations: one channel transform per sample).  Everything is checked before
    the table goes to the device.

    What seld_gather_rows_polar applies (hip_ops.gather_rows_polar): the same p_rot, rot_mirror and rot_zflip on
    magnitude-phase predictors; rot_polar, 1..2 channel groups (mx, my, mz, px, py, pz), e.g. `foa_polar(...)`, held as a
    tuple of tuples.  p_rot > 0 needs exactly one of rot_triples and rot_polar.

    What seld_gather_rows_mix applies (hip_ops.gather_rows_mix): p_mix, the probability that a second clip of the epoch is
    mixed into a sample of magnitude-phase predictors, with a gain drawn uniformly from mix_gain = (lo, hi),
    0 < lo <= hi.  p_mix > 0 excludes p_rot > 0 and p_swap > 0 (one transforming gather per sample); masks go with it."""
    table: object = None
    p_swap: float = 0.0
    freq_masks: int = 0
    freq_width: int = 0
    time_masks: int = 0
    time_width: int = 0
    fill: float = 0.0
    device: object = "cuda"
    p_rot: float = 0.0
    rot_triples: object = None
    rot_mirror: bool = True
    rot_zflip: bool = True
    rot_polar: object = None
    p_mix: float = 0.0
    mix_gain: tuple = (0.5, 1.0)

    def __post_init__(self):
        host = None if self.table is None else _check_table(self.table, None)
        if not 0.0 <= float(self.p_swap) <= 1.0:
            raise L.SeldHipError(f"Augment: p_swap {self.p_swap} is no probability")
        for name in ("freq_masks", "time_masks"):
            if getattr(self, name) not in (0, 1, 2):
                raise L.SeldHipError(f"Augment: {name} must be 0, 1 or 2, got {getattr(self, name)}")
        if int(self.freq_width) < 0 or int(self.time_width) < 0:
            raise L.SeldHipError("Augment: a negative mask width")
        if not 0.0 <= float(self.p_rot) <= 1.0:
            raise L.SeldHipError(f"Augment: p_rot {self.p_rot} is no probability")
        for name, width, max_sets in (("rot_triples", 3, ROT_MAX_TRIPLES), ("rot_polar", 6, POLAR_MAX_GROUPS)):
            if getattr(self, name) is not None:
                object.__setattr__(self, name, _check_channel_sets(getattr(self, name), name, width, max_sets))
        if float(self.p_rot) > 0.0 and self.rot_triples is None and self.rot_polar is None:
            raise L.SeldHipError("Augment: p_rot > 0 needs rot_triples, the channels of the intensity vectors, or rot_polar, "
                                 "the magnitude and phase channels")
        if float(self.p_rot) > 0.0 and self.rot_triples is not None and self.rot_polar is not None:
            raise L.SeldHipError("Augment: p_rot > 0 with both rot_triples and rot_polar (one kind of predictors per loader)")
        if float(self.p_rot) > 0.0 and float(self.p_swap) > 0.0:
            raise L.SeldHipError("Augment: p_rot > 0 together with p_swap > 0 (one channel transform per sample)")
        if not 0.0 <= float(self.p_mix) <= 1.0:
            raise L.SeldHipError(f"Augment: p_mix {self.p_mix} is no probability")
        try:
            lo, hi = (float(v) for v in self.mix_gain)
        except (TypeError, ValueError):
            raise L.SeldHipError(f"Augment: mix_gain must be a pair (lo, hi), got {self.mix_gain!r}") from None
        if not (0.0 < lo <= hi < float("inf")):
            raise L.SeldHipError(f"Augment: mix_gain needs finite 0 < lo <= hi, got {(lo, hi)}")
        object.__setattr__(self, "mix_gain", (lo, hi))
        if float(self.p_mix) > 0.0 and (float(self.p_rot) > 0.0 or float(self.p_swap) > 0.0):
            raise L.SeldHipError("Augment: p_mix > 0 together with p_rot > 0 or p_swap > 0 (one transforming gather per sample)")
        object.__setattr__(self, "table", None if host is None else torch.from_numpy(host).to(self.device))

    @property
    def kind(self):
        """Which gather a loader fetches with: 'mix' (gather_rows_mix) when p_mix > 0; 'polar' (gather_rows_polar) or 'rot'
        (gather_rows_rot) when p_rot > 0, by the channel sets given; otherwise 'swap' (gather_rows_aug: table and masks)."""
        if float(self.p_mix) > 0.0:
            return "mix"
        if float(self.p_rot) > 0.0:
            return "polar" if self.rot_polar is not None else "rot"
        return "swap"

    @property
    def rot_channels(self):
        """The least number of channels the triples need, None without triples."""
        return _least_channels(self.rot_triples)

    @property
    def rot_packed(self):
        """The triples as seld_gather_rows_rot takes them: 4 bits per entry."""
        return _packed(self.rot_triples)

    @property
    def polar_channels(self):
        """The least number of channels the groups need, None without groups."""
        return _least_channels(self.rot_polar)

    @property
    def polar_packed(self):
        """The groups as seld_gather_rows_polar takes them: 4 bits per entry."""
        return _packed(self.rot_polar)

    @property
    def channels(self):
        return None if self.table is None else (self.table.shape[1] - 6) // 2

    @property
    def transforms(self):
        return 0 if self.table is None else self.table.shape[0]


def _launch_aug(what, gather, epoch, seed, augment, field, own, matrices=None, stats=None, y_cols=None):
    """What the four augmenting gathers do alike.  The checks of `_gather_args` (`gather`: its arguments behind `what`), of
    `augment`, `epoch` and the geometry: predictors (n, C, F, T), targets (n, ..., 4 * n_sed).  `field` names the channel
    sets of a rotating gather, which must be there and fit into C (None: the table, which must be for C channels; 'mix':
    neither, every channel takes part and C is 2 without predictors); without predictors C is what the sets or the table
    need.  `matrices` and `stats` as the rotating entry points read them; `y_cols`: the target columns where there are no
    targets to tell (the mix with an occupancy table).  Then the launch with `own()`, the arguments of this entry point
    alone, between (C, F, T, y_cols, epoch, seed) and the masks."""
    if not isinstance(augment, Augment):
        raise L.SeldHipError(f"{what}: augment must be an Augment, got {type(augment).__name__}")
    mix = field == "mix"
    if mix:
        field = None
    if field is not None and getattr(augment, field) is None:
        raise L.SeldHipError(f"{what}: the Augment has no {field}")
    channels = 2 if mix else augment.channels if field is None else _least_channels(getattr(augment, field))
    g = _gather_args(what, *gather)
    x_all, y_all, _, _, dev, count, _, _ = g
    if _scalar(epoch, what, "epoch", torch.int32).device != dev:
        raise L.SeldHipError(f"{what}: epoch on another device")
    C, F, T = (1 if channels is None else channels), 1, 1
    if x_all is not None:
        if x_all.dim() != 4:
            raise L.SeldHipError(f"{what}: predictors must be (n, C, F, T), got {tuple(x_all.shape)}")
        C, F, T = x_all.shape[1:]
        if field is not None and channels > C:
            raise L.SeldHipError(f"{what}: {field} name channel {channels - 1}, the predictors have {C}")
    y_cols = 4 if y_cols is None else int(y_cols)
    if y_all is not None:
        if y_all.dim() < 2:
            raise L.SeldHipError(f"{what}: targets must be (n, ..., 4 * n_sed), got {tuple(y_all.shape)}")
        y_cols = y_all.shape[-1]
    table = augment.table
    if field is None and not mix and table is not None and (table.device != dev or channels != C):
        raise L.SeldHipError(f"{what}: the transform table is for {channels} channels on {table.device}, "
                             f"the predictors have {C} on {dev}")
    if matrices is not None:
        if (not torch.is_tensor(matrices) or _req(matrices, f"{what}: matrices") is not matrices or matrices.device != dev
                or matrices.dim() < 2 or matrices.shape[0] < count
                or tuple(matrices.shape[1:]) not in ((9,), (3, 3))):
            raise L.SeldHipError(f"{what}: matrices must be a contiguous fp32 tensor ({count}, 9) or ({count}, 3, 3) on {dev}, "
                                 f"got {getattr(matrices, 'shape', type(matrices).__name__)}")
    if stats is not None:
        _check_stats(stats, dev, what)
    return _launch(what, g, (C, F, T, y_cols, L.ptr(epoch), int(seed) & 0xFFFFFFFFFFFFFFFF, *own(), int(augment.freq_masks),
                             int(augment.freq_width), int(augment.time_masks), int(augment.time_width), float(augment.fill)))


def gather_rows_aug(x_all, y_all, index, out_x, out_y, *, epoch, seed, augment, cursor=None, start=0, count=None, stride=None):
    """`gather_rows` with `augment` (an Augment) applied to every sample on the way, in ONE launch
    (seld_gather_rows_aug).  x_all (n, C, F, T) and y_all (n, T_out, 4 * n_sed) name the geometry.  epoch: a device int32
    of one element, read by the kernel; seed: the key of the draws, which depend on (seed, epoch, position in `index`)
    and nothing else.  Rows of invalid positions or indices are zero-filled and not augmented."""
    return _launch_aug("gather_rows_aug", (x_all, y_all, index, out_x, out_y, cursor, start, count, stride), epoch, seed, augment, None,
                       lambda: (L.ptr(augment.table), augment.transforms, float(augment.p_swap)))


def _rotation_args(augment, matrices):
    """(p_rot, rot_mirror, rot_zflip, matrices) as the rotating entry points take them."""
    return float(augment.p_rot), int(bool(augment.rot_mirror)), int(bool(augment.rot_zflip)), L.ptr(matrices)


def gather_rows_rot(x_all, y_all, index, out_x, out_y, *, epoch, seed, augment, matrices=None, cursor=None, start=0, count=None,
                    stride=None):
    """`gather_rows` with a rotation of the sound field applied to every sample on the way, then the masks of `augment`, in
    ONE launch (seld_gather_rows_rot; include/seld_hip.h has the draws).  The channels of `augment.rot_triples` are the
    x, y, z components of intensity vectors: a rotated sample gets x'[c_a] = sum_j R[a][j] x[c_j] per triple and
    location'(s, a) = sum_j R[a][j] location(s, j); every other channel and the activity are copied.  R is drawn per
    sample with probability augment.p_rot from (seed, epoch, position), or, with `matrices` (fp32 device tensor (count, 9)
    or (count, 3, 3), row-major), sample b takes matrices[b] as it is.  augment.table and p_swap are not used.
    Geometry, epoch, cursor, start, count, stride and the zero rows of invalid positions as in `gather_rows_aug`."""
    return _launch_aug("gather_rows_rot", (x_all, y_all, index, out_x, out_y, cursor, start, count, stride), epoch, seed, augment,
                       "rot_triples", lambda: (augment.rot_packed, len(augment.rot_triples)) + _rotation_args(augment, matrices),
                       matrices)


_stats_checked = {}     # id(tensor) -> (weak reference, _version) of the statistics tensors whose content has been read back


def _check_stats(stats, dev, what):
    """`stats` as seld_gather_rows_polar reads it: 4 contiguous fp32 on `dev`, finite, both standard deviations > 0.  The
    content costs a read-back (a synchronisation), so it is looked at once per tensor, and again after an in-place change."""
    if not torch.is_tensor(stats) or _req(stats, f"{what}: stats") is not stats or stats.device != dev or stats.numel() != 4:
        raise L.SeldHipError(f"{what}: stats must be a contiguous fp32 tensor of 4 values (mean_m, sd_m, mean_p, sd_p) on {dev}, "
                             f"got {getattr(stats, 'shape', type(stats).__name__)}")
    seen = _stats_checked.get(id(stats))
    if seen is None or seen[0]() is not stats or seen[1] != stats._version:
        if torch.cuda.is_current_stream_capturing():
            raise L.SeldHipError(f"{what}: the first call with a statistics tensor reads it back: make it outside the capture")
        mean_m, sd_m, mean_p, sd_p = (float(v) for v in stats.reshape(4).tolist())
        if not all(np.isfinite(v) for v in (mean_m, sd_m, mean_p, sd_p)) or sd_m <= 0 or sd_p <= 0:
            raise L.SeldHipError(f"{what}: stats must be finite with both standard deviations > 0, got "
                                 f"{(mean_m, sd_m, mean_p, sd_p)}")
        key = id(stats)
        _stats_checked[key] = (weakref.ref(stats, lambda _, key=key: _stats_checked.pop(key, None)), stats._version)
    return stats


def gather_rows_polar(x_all, y_all, index, out_x, out_y, *, epoch, seed, augment, stats=None, matrices=None, cursor=None, start=0,
                      count=None, stride=None):
    """`gather_rows_rot` for magnitude-phase predictors, in ONE launch (seld_gather_rows_polar; include/seld_hip.h has the
    formula).  The channels of `augment.rot_polar` are (mx, my, mz, px, py, pz) per microphone: a rotated sample gets, per
    group and (f, t), the complex 3-vector m e^(i phi) of its directional channels multiplied by R and written back as
    magnitude and phase; location'(s, a) = sum_j R[a][j] location(s, j); every other channel (W among them) and the
    activity are copied; then the masks of `augment`.  stats: fp32 device tensor (mean_m, sd_m, mean_p, sd_p) when the
    predictors are standardised per half as data.normalize_dataset leaves them (the kernel undoes and redoes it around
    the rotation), None for raw magnitude and phase; its content is checked at the first call with that tensor.  R,
    `matrices`, geometry, epoch, cursor, start, count, stride and the zero rows of invalid positions as in
    `gather_rows_rot`.  augment.table, p_swap and rot_triples are not used."""
    return _launch_aug("gather_rows_polar", (x_all, y_all, index, out_x, out_y, cursor, start, count, stride), epoch, seed, augment,
                       "rot_polar",
                       lambda: (augment.polar_packed, len(augment.rot_polar), L.ptr(stats)) + _rotation_args(augment, matrices),
                       matrices, stats)


def target_occupancy(y_all, overlaps):
    """uint8 (n, classes): per target row and class the largest number of slots that are active (activity > 0.5) in one
    frame (seld_target_occupancy).  y_all (n, ..., 4 * classes * overlaps): contiguous fp32 on the device, the slot of
    (class c, place o) at column c * overlaps + o.  What `gather_rows_mix(occupancy=...)` consults; made once per array,
    outside any capture (it allocates)."""
    y_all, row_y = _rows(y_all, "target_occupancy", "y_all")
    overlaps = int(overlaps)
    if y_all is None or y_all.dim() < 2 or y_all.shape[0] < 1 or row_y < 1:
        raise L.SeldHipError(f"target_occupancy: targets must be (n, ..., 4 * n_sed), got {None if y_all is None else tuple(y_all.shape)}")
    y_cols = y_all.shape[-1]
    if overlaps < 1 or y_cols % (4 * overlaps):
        raise L.SeldHipError(f"target_occupancy: {y_cols} target columns are not 4 * classes * {overlaps} overlaps")
    occ = torch.empty((y_all.shape[0], y_cols // (4 * overlaps)), device=y_all.device, dtype=torch.uint8)
    with torch.cuda.device(y_all.device):
        L.check(L.lib().seld_target_occupancy(L.ptr(y_all), y_all.shape[0], row_y, y_cols, overlaps, L.ptr(occ), L.current_stream()),
                "seld_target_occupancy")
    return occ


def _per_sample(t, what, name, dtype, dev, count):
    if not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or not t.is_contiguous() or t.dim() != 1 or t.shape[0] < count:
        raise L.SeldHipError(f"{what}: {name} must be a contiguous {dtype} tensor of {count} entries on {dev}, "
                             f"got {getattr(t, 'shape', type(t).__name__)}")
    return t


def gather_rows_mix(x_all, y_all, index, out_x, out_y, *, epoch, seed, augment, overlaps, stats=None, partners=None, gains=None,
                    occupancy=None, cursor=None, start=0, count=None, stride=None):
    """`gather_rows` with a second clip mixed into every sample that draws one, then the masks of `augment`, in ONE launch
    (seld_gather_rows_mix; include/seld_hip.h has the draw and the formula).  Predictors are magnitude-phase, channel
    c < C / 2 a magnitude and c + C / 2 its phase: a mixed sample gets, per pair and (f, t), the complex sum
    z_A + g z_B written back as magnitude and phase, which is what the STFT of the mixed waveforms holds.  Its targets
    (..., 4 * classes * overlaps) are merged per (frame, class): A's active slots, then B's, packed into the `overlaps`
    slots; entries beyond them are dropped.  With `occupancy` (`target_occupancy(y_all, overlaps)`) a pair of clips that
    could overflow a class is not mixed at all, so no label is lost.  The partner is drawn with probability
    augment.p_mix among the OTHER positions of `index` and the gain from augment.mix_gain, from (seed, epoch, position);
    or, with `partners` (int64, count) and `gains` (fp32, count) on the device, sample b takes the position partners[b]
    (negative: no mix) and gains[b] as they are.  stats as in `gather_rows_polar`.  Geometry, epoch, cursor, start, count,
    stride and the zero rows of invalid positions as in `gather_rows_aug`; augment.table, p_swap and the rotation fields
    are not used."""
    what = "gather_rows_mix"
    overlaps = int(overlaps)
    if not isinstance(augment, Augment):
        raise L.SeldHipError(f"{what}: augment must be an Augment, got {type(augment).__name__}")
    if not 1 <= overlaps <= MIX_MAX_OVERLAPS:
        raise L.SeldHipError(f"{what}: 1..{MIX_MAX_OVERLAPS} overlaps, got {overlaps}")
    if (partners is None) != (gains is None):
        raise L.SeldHipError(f"{what}: partners and gains are given together or not at all")
    if torch.is_tensor(x_all) and x_all.dim() == 4 and x_all.shape[1] % 2:
        raise L.SeldHipError(f"{what}: magnitude-phase predictors have an even number of channels, got {x_all.shape[1]}")
    y_cols = None
    if torch.is_tensor(y_all) and y_all.dim() >= 2:
        y_cols = y_all.shape[-1]
    if occupancy is not None:
        if not torch.is_tensor(occupancy) or occupancy.dtype != torch.uint8 or not occupancy.is_contiguous() or occupancy.dim() != 2:
            raise L.SeldHipError(f"{what}: occupancy must be the contiguous uint8 table (n, classes) of target_occupancy")
        y_cols = 4 * overlaps * occupancy.shape[1] if y_cols is None else y_cols
        if y_cols != 4 * overlaps * occupancy.shape[1]:
            raise L.SeldHipError(f"{what}: an occupancy table of {occupancy.shape[1]} classes with {y_cols} target columns "
                                 f"and {overlaps} overlaps")
    if y_cols is not None and (y_cols % (4 * overlaps) or y_cols // (4 * overlaps) > MIX_MAX_CLASSES):
        raise L.SeldHipError(f"{what}: {y_cols} target columns are not 4 * (1..{MIX_MAX_CLASSES} classes) * {overlaps} overlaps")

    def own():
        n = (x_all if x_all is not None else y_all).shape[0]
        dev = (x_all if x_all is not None else y_all).device
        rows = (out_x if out_x is not None else out_y).shape[0] if count is None else int(count)
        if partners is not None:
            _per_sample(partners, what, "partners", torch.int64, dev, rows)
            _per_sample(gains, what, "gains", torch.float32, dev, rows)
        if occupancy is not None and (occupancy.device != dev or occupancy.shape[0] != n):
            raise L.SeldHipError(f"{what}: the occupancy table has {occupancy.shape[0]} rows on {occupancy.device}, the arrays {n} on {dev}")
        return (overlaps, L.ptr(stats), float(augment.p_mix), augment.mix_gain[0], augment.mix_gain[1], L.ptr(partners), L.ptr(gains),
                L.ptr(occupancy))
    return _launch_aug(what, (x_all, y_all, index, out_x, out_y, cursor, start, count, stride), epoch, seed, augment, "mix", own,
                       None, stats, y_cols)


def epoch_step_end(loss, mean, cursor):
    """mean += (loss - mean) / (cursor + 1); cursor += 1 on the device (seld_epoch_step_end): the running mean of
    train.main's epoch loop without a read-back.  loss, mean: fp32 device scalars; cursor: the int32 device scalar of gather_rows."""
    _scalar(loss, "epoch_step_end", "loss", torch.float32)
    _scalar(mean, "epoch_step_end", "mean", torch.float32)
    _scalar(cursor, "epoch_step_end", "cursor", torch.int32)
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
