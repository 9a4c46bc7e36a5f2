"""float64 numpy statement of the spatial features (include/seld_hip.h, csrc/spatial_features.hip): complex spectra from
scipy.signal.stft, the mel filterbank restated filter by filter, log-power and FOA intensity vector per bin or per band,
and the error bound the device result is held to, propagated from a bound on the complex spectrum's error.  Shared by
tests/test_spatial_features_host.py and tests/test_gpu_spatial_features.py; nothing here imports the package."""
import functools
import math

import numpy as np
import scipy.signal

U24 = 2.0 ** -24          # half an ulp of float32 at 1

# (nperseg, noverlap, L, n_mels, sr): radix-8 (54 frames), radix-2, 7-smooth (39 frames), Bluestein (28 frames)
CASES = [(512, 128, 20000, 64, 32000), (64, 16, 700, 8, 32000), (480, 240, 9000, 40, 24000), (97, 40, 1500, 10, 16000)]
CASE_IDS = ["radix8_512", "radix2_64", "smooth_480", "bluestein_97"]
# (channels, cut_dc, cut_last_timeframe): 8 and 4 channels, both cuts both ways
VARIANTS = [(8, True, True), (8, False, False), (4, True, False), (4, False, True)]
# (kind, layout)
FORMS = [("logpower", "grouped"), ("iv", "grouped"), ("logpower_iv", "grouped"), ("logpower_iv", "quaternion")]


def hz_to_mel(f, htk=False):
    if htk:
        return 2595.0 * math.log10(1.0 + f / 700.0)
    return f * 3.0 / 200.0 if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def mel_to_hz(m, htk=False):
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return m * 200.0 / 3.0 if m < 15.0 else 1000.0 * math.exp((m - 15.0) * math.log(6.4) / 27.0)


def mel_points(sr, n_mels, fmin=0.0, fmax=None, htk=False):
    """The n_mels + 2 edge / centre frequencies in Hz."""
    fmax = sr / 2.0 if fmax is None else fmax
    m0, m1 = hz_to_mel(fmin, htk), hz_to_mel(fmax, htk)
    return [mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1), htk) for i in range(n_mels + 2)]


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None, htk=False, norm='slaney'):
    f = mel_points(sr, n_mels, fmin, fmax, htk)
    fb = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        for k in range(n_fft // 2 + 1):
            hz = k * sr / n_fft
            if f[m] < hz <= f[m + 1]:
                fb[m, k] = (hz - f[m]) / (f[m + 1] - f[m])
            elif f[m + 1] < hz < f[m + 2]:
                fb[m, k] = (f[m + 2] - hz) / (f[m + 2] - f[m + 1])
        if norm == 'slaney':
            fb[m] *= 2.0 / (f[m + 2] - f[m])
    return fb


@functools.lru_cache(maxsize=None)
def case_input(case):
    """RandomState(nperseg).randn(8, L) * 0.3 plus a tone at sr / 20 on channels 0-3 with gains (1, 0.5, -0.3, 0.7):
    the intensity vector of the first group has a definite direction.  float32, read-only."""
    nperseg, _, L, _, sr = case
    x = np.random.RandomState(nperseg).randn(8, L) * 0.3
    x[:4] += np.sin(2 * np.pi * (sr / 20) * np.arange(L) / sr)[None, :] * np.array([1, 0.5, -0.3, 0.7])[:, None]
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def spectrum(x32, nperseg, noverlap, cut_dc, cut_last_timeframe, window='hamming'):
    """complex128 (..., bins, frames) of the float32-rounded input: scipy's scaling is spectrum_fast's."""
    _, _, Z = scipy.signal.stft(np.asarray(x32, dtype=np.float64), window=window, nperseg=nperseg, noverlap=noverlap)
    Z = Z[..., 1:, :] if cut_dc else Z
    return Z[..., :-1] if cut_last_timeframe else Z


@functools.lru_cache(maxsize=None)
def case_spectrum(case, variant):
    C, cut_dc, cut_last = variant
    Z = spectrum(case_input(case)[:C], case[0], case[1], cut_dc, cut_last)
    Z.setflags(write=False)
    return Z


def case_fb(case, cut_dc):
    nperseg, _, _, n_mels, sr = case
    fb = mel_filterbank(sr, nperseg, n_mels)
    return fb[:, 1:] if cut_dc else fb


def _project(fb, a):
    """sum_k fb[m, k] a[..., k, t] (fb None: a itself)."""
    return a if fb is None else np.einsum('mk,...kt->...mt', fb, a)


def components(Z, fb=None, eps=1e-10, d=0.0):
    """Z (C, bins, frames) complex128 -> dict of
      lp (C, bands, frames) = log(P + eps), iv (C // 4, 3, bands, frames) (None when C % 4 != 0),
      lp_tol, iv_tol: the allowed error of each element for a spectrum known to |dZ| <= d per bin:
        dp = 2 |Z| d + d^2,  dP = sum fb dp,  lp_tol = dP / (P + eps) + 8 2^-24 max(1, |lp|);
        dE the same propagation of E,  di = (d (|W| + |D_d|) + d^2 + |i_d| dE) / E,
        iv_tol = sum fb di + 8 2^-24 sum fb |i_d|."""
    p = np.abs(Z) ** 2
    a = np.abs(Z)
    dp = 2 * a * d + d * d
    P = _project(fb, p)
    lp = np.log(P + eps)
    out = dict(lp=lp, lp_tol=_project(fb, dp) / (P + eps) + 8 * U24 * np.maximum(1.0, np.abs(lp)), iv=None, iv_tol=None)
    C = Z.shape[0]
    if C % 4 == 0:
        G = C // 4
        Zg, pg, ag, dpg = (v.reshape((G, 4) + Z.shape[1:]) for v in (Z, p, a, dp))
        E = eps + pg[:, 0] + (pg[:, 1] + pg[:, 2] + pg[:, 3]) / 3
        dE = dpg[:, 0] + (dpg[:, 1] + dpg[:, 2] + dpg[:, 3]) / 3
        i = np.real(np.conj(Zg[:, :1]) * Zg[:, 1:]) / E[:, None]
        di = (d * (ag[:, :1] + ag[:, 1:]) + d * d + np.abs(i) * dE[:, None]) / E[:, None]
        out["iv"] = _project(fb, i)
        out["iv_tol"] = _project(fb, di) + 8 * U24 * _project(fb, np.abs(i))
    return out


def assemble(lp, iv, kind, layout):
    """The planes of (kind, layout) in the order of include/seld_hip.h, of lp (C, ...) and iv (G, 3, ...)."""
    if kind == "logpower":
        return lp
    G = iv.shape[0]
    if kind == "iv":
        return iv.reshape((3 * G,) + iv.shape[2:])
    if layout == "quaternion":
        return np.concatenate((lp[0::4][:, None], iv), axis=1).reshape((4 * G,) + iv.shape[2:])
    return np.concatenate((lp, iv.reshape((3 * G,) + iv.shape[2:])), axis=0)


def features(Z, kind, layout, fb=None, eps=1e-10, d=0.0):
    """(reference, allowed error), both in the layout of (kind, layout)."""
    c = components(Z, fb, eps, d)
    return assemble(c["lp"], c["iv"], kind, layout), assemble(c["lp_tol"], c["iv_tol"], kind, layout)
