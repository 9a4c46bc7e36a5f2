"""Log-power and first-order-Ambisonics intensity-vector features of complex spectra (csrc/spatial_features.hip), linear
in frequency or projected onto bands, and the mel filterbank that gives the bands.  include/seld_hip.h has the
definitions; `utility_functions.seld_features` is the call from a waveform."""
import functools

import numpy as np
import torch

from .. import _lib as L
from ._core import timed

__all__ = ["mel_filterbank", "band_extents", "spatial_features", "FEATURE_KINDS", "FEATURE_LAYOUTS"]

FEATURE_KINDS = {"logpower": 0, "iv": 1, "logpower_iv": 2}      # SELD_FEAT_*
FEATURE_LAYOUTS = {"grouped": 0, "quaternion": 1}               # SELD_FEAT_LAYOUT_*


def _hz_to_mel(f, htk):
    f = np.asarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    # Slaney: linear at 200/3 Hz per mel below 1 kHz, log steps of log(6.4) / 27 above
    lin = f * (3.0 / 200.0)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) * (27.0 / np.log(6.4)), lin)


def _mel_to_hz(m, htk):
    m = np.asarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * (200.0 / 3.0))


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None, htk=False, norm='slaney'):
    """The (n_mels, n_fft // 2 + 1) float64 table of triangular mel filters over the bins k sr / n_fft of an n_fft-point
    transform: n_mels + 2 frequencies equally spaced in mel between fmin and fmax (default sr / 2), filter m rising from
    f[m] to 1 at f[m + 1] and falling to 0 at f[m + 2].  Slaney mel scale (linear at 200/3 Hz per mel below 1 kHz, log
    steps of log(6.4) / 27 above) or, with htk, 2595 log10(1 + f / 700).  norm='slaney' scales each triangle by
    2 / (f[m + 2] - f[m]) (about constant energy per band), norm=None leaves the peaks at 1.  A host-side constant
    table, like the window's."""
    sr, n_fft, n_mels = float(sr), int(n_fft), int(n_mels)
    fmax = sr / 2.0 if fmax is None else float(fmax)
    if n_fft < 2 or n_mels < 1 or not sr > 0:
        raise ValueError(f"mel_filterbank: sr={sr}, n_fft={n_fft}, n_mels={n_mels} must be positive (n_fft at least 2)")
    if not 0.0 <= fmin < fmax:
        raise ValueError(f"mel_filterbank: need 0 <= fmin < fmax, got {fmin}, {fmax}")
    if norm not in ('slaney', None):
        raise ValueError(f"mel_filterbank: norm must be 'slaney' or None, got {norm!r}")
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (sr / n_fft)
    f = _mel_to_hz(np.linspace(_hz_to_mel(fmin, htk), _hz_to_mel(fmax, htk), n_mels + 2), htk)
    rise = (freqs[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    fall = (f[2:, None] - freqs[None, :]) / (f[2:] - f[1:-1])[:, None]
    fb = np.maximum(0.0, np.minimum(rise, fall))
    if norm == 'slaney':
        fb *= (2.0 / (f[2:] - f[:-2]))[:, None]
    return fb


def band_extents(fb):
    """(lo, hi) int32 arrays: the first and one-past-last nonzero bin of each band of fb (bands, bins); lo == hi == 0
    for an all-zero band."""
    fb = np.asarray(fb)
    if fb.ndim != 2:
        raise ValueError(f"band_extents: expected (bands, bins), got shape {fb.shape}")
    nz = fb != 0
    has = nz.any(axis=1)
    lo = np.where(has, nz.argmax(axis=1), 0).astype(np.int32)
    hi = np.where(has, fb.shape[1] - nz[:, ::-1].argmax(axis=1), 0).astype(np.int32)
    return lo, hi


def _feature_form(what, kind, layout, C, eps):
    """(kind, layout) as the library's numbers; every refusal a ValueError, nothing here touches the device."""
    if kind not in FEATURE_KINDS:
        raise ValueError(f"{what}: kind must be one of {', '.join(FEATURE_KINDS)}, got {kind!r}")
    if layout not in FEATURE_LAYOUTS:
        raise ValueError(f"{what}: layout must be one of {', '.join(FEATURE_LAYOUTS)}, got {layout!r}")
    if layout == 'quaternion' and kind != 'logpower_iv':
        raise ValueError(f"{what}: layout='quaternion' is [log-power of W, I1, I2, I3] per microphone: it needs "
                         f"kind='logpower_iv', got {kind!r}")
    if kind != 'logpower' and C % 4 != 0:
        raise ValueError(f"{what}: the intensity vector needs groups of four channels [W, D1, D2, D3], got {C} channels")
    if not float(eps) > 0.0:
        raise ValueError(f"{what}: eps must be positive, got {eps!r}")
    return FEATURE_KINDS[kind], FEATURE_LAYOUTS[layout]


def _band_tables(what, fb, bins):
    """fb as the host arrays the kernel reads: (fb float32 (bands, bins), lo, hi), or None for linear frequency."""
    if fb is None:
        return None
    fb = np.asarray(fb.detach().cpu() if torch.is_tensor(fb) else fb, dtype=np.float64)
    if fb.ndim != 2 or fb.shape[0] < 1:
        raise ValueError(f"{what}: fb must be (bands, bins), got shape {fb.shape}")
    if fb.shape[1] != bins:
        raise ValueError(f"{what}: fb has {fb.shape[1]} bins, the spectrum {bins} (with the DC bin cut pass fb[:, 1:])")
    fb32 = np.ascontiguousarray(fb, dtype=np.float32)
    return (fb32,) + band_extents(fb32)


def _on_device(tables, device):
    return None if tables is None else tuple(torch.from_numpy(a).to(device) for a in tables)


@functools.lru_cache(maxsize=16)
def _mel_tables(sr, n_fft, n_mels, fmin, fmax, cut_dc, device):
    """The device tables of `seld_features`' mel bands, made once per setting and device."""
    fb = mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    fb = fb[:, 1:] if cut_dc else fb
    return _on_device(_band_tables("seld_features", fb, fb.shape[1]), device)


def _features_of_planes(what, planes, lead, C, kind, layout, tables, eps):
    """The launch: planes (2R, bins, frames) float32 on the device, Re Z of the R = prod(lead) * C rows, then Im Z; kind /
    layout the library's numbers, already checked against C; tables: (fb, lo, hi) on the device, or None.  Returns
    (*lead, C_out, bands, frames).  The rows of a batch are one channel axis to the kernel (groups of four stay groups);
    only kind 2 in the grouped layout, whose planes are ordered across the whole axis, is put back in order per item
    afterwards (one device copy, batched input only)."""
    lib, dev = L.lib(), planes.device
    R, bins, frames = planes.shape[0] // 2, planes.shape[1], planes.shape[2]
    fb, lo, hi = tables if tables is not None else (None, None, None)
    bands = bins if fb is None else fb.shape[0]
    planes_out = lib.seld_spatial_features_channels(R, kind, layout)
    L.check(min(planes_out, 0), "seld_spatial_features_channels")
    out = torch.empty((planes_out, bands, frames), device=dev, dtype=torch.float32)
    nbytes = 4 * (planes.numel() + out.numel())
    with torch.cuda.device(dev):
        with timed("features_banded_kernel" if tables is not None else "features_linear_kernel",
                   lambda: (0.0, float(nbytes))):
            L.check(lib.seld_spatial_features(L.ptr(planes), R, bins, frames, kind, layout, L.ptr(fb), L.ptr(lo), L.ptr(hi),
                                              bands, float(eps), L.ptr(out), L.current_stream()), "seld_spatial_features")
    items = R // C
    if kind == 2 and layout == 0 and items > 1:
        out = torch.cat((out[:R].view(items, C, bands, frames), out[R:].view(items, 3 * C // 4, bands, frames)), dim=1)
    return out.view(tuple(lead) + (planes_out // items, bands, frames))


def spatial_features(z, kind='logpower_iv', layout='grouped', fb=None, eps=1e-10):
    """Log-power and intensity-vector features of complex spectra z (..., C, bins, frames), a complex64 device tensor
    (`utility_functions.stft_complex`).  Per bin, per group of four channels [W, D1, D2, D3] (one first-order-Ambisonics
    microphone):  p_c = |Z_c|^2,  E = eps + |W|^2 + (|D1|^2 + |D2|^2 + |D3|^2) / 3,  i_d = Re(conj(W) D_d) / E.

    kind: 'logpower' -> (..., C, bands, frames), log(P + eps) per channel; 'iv' -> (..., 3C/4, ...), the three components
    per group; 'logpower_iv' -> with layout='grouped' (..., C + 3C/4, ...): every log-power plane, then the intensity
    planes group by group; with layout='quaternion' (..., C, ...): per group [log-power of W, I1, I2, I3], one quaternion
    per microphone (two microphones: the eight channels of one dual quaternion).
    fb: None for linear frequency (bands = bins), or a (bands, bins) table of non-negative weights, e.g.
    `mel_filterbank(...)` (`[:, 1:]` of it where the DC bin is cut): P[m] = sum_k fb[m,k] p[k], I_d[m] = sum_k fb[m,k]
    i_d[k] -- normalised per bin, then projected.  An all-zero band gives log(eps) and a zero vector.

    Returns float32 on z's device.  No backward pass.  Every refusal of an argument is a ValueError raised before the
    device is touched.  The kernel reads planes of real and imaginary parts: z is split once here;
    `utility_functions.seld_features` hands the transform's planes over as they are."""
    what = "spatial_features"
    if not torch.is_tensor(z) or not z.is_complex() or z.dim() < 3:
        raise ValueError(f"{what}: z must be a complex tensor (..., channels, bins, frames)")
    lead, (C, bins, frames) = tuple(z.shape[:-3]), z.shape[-3:]
    k, l = _feature_form(what, kind, layout, C, eps)
    if min(z.shape) < 1:
        raise ValueError(f"{what}: every extent of z must be positive, got {tuple(z.shape)}")
    tables = _band_tables(what, fb, bins)
    if not z.is_cuda:
        raise L.SeldHipError(f"{what}: expected a HIP device tensor (this package has no CPU path)")
    zr = torch.view_as_real(z.to(torch.complex64).reshape((-1, bins, frames)))          # (R, bins, frames, 2)
    planes = zr.permute(3, 0, 1, 2).contiguous().view(-1, bins, frames)
    return _features_of_planes(what, planes, lead, C, k, l, _on_device(tables, z.device), eps)
