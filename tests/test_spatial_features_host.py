"""Host checks of the spatial features (hip_ops/features.py, csrc/spatial_features.hip, seld_stft_complex_ws): the mel
filterbank against anchors and against the reference's restatement, the band extents, and what the library decides
before any HIP call.  No device needed."""
import ctypes
import math

import numpy as np
import pytest

from tests import spatial_features_ref as R
from tests.helpers import pkg

EINVAL, EUNSUPPORTED = -1, -4
# (sr, n_fft, n_mels) of the device cases
BANKS = [(c[4], c[0], c[3]) for c in R.CASES]


def test_mel_scale_anchors():
    F = pkg().hip_ops.features
    assert float(F._hz_to_mel(1000.0, False)) == 15.0
    assert float(F._hz_to_mel(200.0, False)) == pytest.approx(3.0, abs=1e-12)
    assert float(F._hz_to_mel(6400.0, False)) == pytest.approx(42.0, abs=1e-12)          # 27 log steps above 1 kHz
    assert float(F._hz_to_mel(700.0, True)) == pytest.approx(2595.0 * math.log10(2.0), abs=1e-12)
    for htk in (False, True):
        for f in (0.0, 50.0, 999.0, 1000.0, 1001.0, 4000.0, 16000.0):
            assert float(F._mel_to_hz(F._hz_to_mel(f, htk), htk)) == pytest.approx(f, abs=1e-9)
            assert float(F._hz_to_mel(f, htk)) == pytest.approx(R.hz_to_mel(f, htk), abs=1e-12)


@pytest.mark.parametrize("sr,n_fft,n_mels", BANKS)
@pytest.mark.parametrize("htk", [False, True])
def test_filterbank_is_triangular(sr, n_fft, n_mels, htk):
    H = pkg().hip_ops
    fb = H.mel_filterbank(sr, n_fft, n_mels, htk=htk, norm=None)
    assert fb.shape == (n_mels, n_fft // 2 + 1) and fb.dtype == np.float64
    assert (fb >= 0).all() and (fb <= 1 + 1e-12).all()
    f = R.mel_points(sr, n_mels, htk=htk)
    hz = np.arange(n_fft // 2 + 1) * sr / n_fft
    for m in range(n_mels):
        nz = np.flatnonzero(fb[m])
        assert nz.size > 0, m
        assert (np.diff(nz) == 1).all(), m                               # one stretch
        row = fb[m, nz[0]:nz[-1] + 1]
        peak = int(row.argmax())
        assert (np.diff(row[:peak + 1]) > 0).all() and (np.diff(row[peak:]) < 0).all(), m       # rising, then falling
        assert f[m] < hz[nz[0]] and hz[nz[-1]] < f[m + 2], m
    # neighbouring triangles sum to 1 between the first and the last centre frequency
    inside = (hz >= f[1]) & (hz <= f[n_mels])
    assert inside.any()
    assert np.abs(fb.sum(axis=0)[inside] - 1.0).max() < 1e-12
    # Slaney normalisation: the same triangles, each scaled by 2 / (f[m + 2] - f[m])
    fs = H.mel_filterbank(sr, n_fft, n_mels, htk=htk)
    scale = 2.0 / (np.array(f[2:]) - np.array(f[:-2]))
    assert (fs.max(axis=1) <= scale * (1 + 1e-12)).all()
    assert np.abs(fs - fb * scale[:, None]).max() <= 1e-12 * scale.max()


@pytest.mark.parametrize("sr,n_fft,n_mels", BANKS + [(44100, 2048, 128), (16000, 255, 7)])
def test_filterbank_equals_the_reference_restatement(sr, n_fft, n_mels):
    H = pkg().hip_ops
    for kw in (dict(), dict(htk=True), dict(norm=None), dict(fmin=50.0, fmax=0.4 * sr)):
        assert np.abs(H.mel_filterbank(sr, n_fft, n_mels, **kw) - R.mel_filterbank(sr, n_fft, n_mels, **kw)).max() <= 1e-12


def test_filterbank_refusals():
    H = pkg().hip_ops
    for kw in (dict(n_mels=0), dict(n_fft=1), dict(sr=0), dict(fmin=-1.0), dict(fmin=9000.0, fmax=8000.0), dict(norm='l2')):
        with pytest.raises(ValueError):
            H.mel_filterbank(**{**dict(sr=32000, n_fft=512, n_mels=8), **kw})


def test_band_extents_bracket_the_nonzero_bins():
    H = pkg().hip_ops
    for sr, n_fft, n_mels in BANKS:
        fb = H.mel_filterbank(sr, n_fft, n_mels)
        lo, hi = H.band_extents(fb)
        assert lo.dtype == np.int32 and hi.dtype == np.int32 and lo.shape == hi.shape == (n_mels,)
        for m in range(n_mels):
            nz = np.flatnonzero(fb[m])
            assert (lo[m], hi[m]) == (nz[0], nz[-1] + 1)
    fb = np.zeros((3, 9))
    fb[0, [2, 6]] = 1.0            # an interior zero stretch stays inside the extent
    fb[2, 8] = 0.5
    lo, hi = H.band_extents(fb)
    assert lo.tolist() == [2, 0, 8] and hi.tolist() == [7, 0, 9]


def test_python_refusals_are_value_errors_without_a_device():
    """Everything is refused before the device is touched: these run on a machine without one."""
    import torch
    H = pkg().hip_ops
    z = torch.zeros(8, 5, 7, dtype=torch.complex64)
    for kw in (dict(kind='power'), dict(layout='packed'), dict(eps=0.0), dict(eps=-1e-3), dict(eps=float('nan')),
               dict(kind='iv', layout='quaternion'), dict(kind='logpower', layout='quaternion'),
               dict(fb=np.ones((3, 6))), dict(fb=np.ones(5))):
        with pytest.raises(ValueError):
            H.spatial_features(z, **kw)
    with pytest.raises(ValueError):
        H.spatial_features(z[:6], kind='iv')
    with pytest.raises(ValueError):
        H.spatial_features(z.real)
    UF = pkg().utility_functions
    for kw in (dict(kind='power'), dict(layout='quaternion', kind='iv'), dict(eps=0.0), dict(n_mels=-1)):
        with pytest.raises(ValueError):
            UF.seld_features(np.zeros((8, 4000), np.float32), **kw)
    with pytest.raises(ValueError):
        UF.seld_features(np.zeros((6, 4000), np.float32))
    with pytest.raises(ValueError):
        UF.stft_complex(np.zeros(4000, np.float32))


# ---- the library, before any launch -----------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    L = pkg()._lib
    with open(L.HEADER_PATH) as f:
        declared = L.prototypes(f.read())
    i32, ptr, f32, sz = ctypes.c_int32, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t
    assert declared["seld_stft_complex_ws"] == (ctypes.c_int, [ptr, i32, i32, i32, i32, i32, i32, ptr, ptr, ptr, sz, ptr])
    assert declared["seld_spatial_features_channels"] == (ctypes.c_int, [i32, i32, i32])
    assert declared["seld_spatial_features"] == (ctypes.c_int, [ptr, i32, i32, i32, i32, i32, ptr, ptr, ptr, i32, f32, ptr,
                                                                ptr])
    lib = L.lib()
    for name in ("seld_stft_complex_ws", "seld_spatial_features_channels", "seld_spatial_features"):
        assert getattr(lib, name).argtypes == declared[name][1]


def test_channel_counts():
    lib = pkg()._lib.lib()
    for C in (4, 8, 12, 64):
        assert lib.seld_spatial_features_channels(C, 0, 0) == C
        assert lib.seld_spatial_features_channels(C, 1, 0) == 3 * C // 4
        assert lib.seld_spatial_features_channels(C, 2, 0) == C + 3 * C // 4
        assert lib.seld_spatial_features_channels(C, 2, 1) == C
    for C in (1, 3, 6):
        assert lib.seld_spatial_features_channels(C, 0, 0) == C          # log-power alone takes any channel count
        for kind in (1, 2):
            assert lib.seld_spatial_features_channels(C, kind, 0) == EINVAL
    for kind in (0, 1):
        assert lib.seld_spatial_features_channels(8, kind, 1) == EINVAL   # the quaternion layout is kind 2's
    for kind in (-1, 3, 7):
        assert lib.seld_spatial_features_channels(8, kind, 0) == EINVAL
    for layout in (-1, 2):
        assert lib.seld_spatial_features_channels(8, 2, layout) == EINVAL
    for C in (0, -4):
        assert lib.seld_spatial_features_channels(C, 0, 0) == EINVAL


def test_spatial_features_refusals_before_any_launch():
    """Decided before any HIP call: the pointers are never dereferenced on the host, so any non-null value does."""
    lib = pkg()._lib.lib()
    p = ctypes.c_void_p(4096)

    def call(z=p, C=8, bins=16, frames=10, kind=2, layout=0, fb=None, lo=None, hi=None, bands=16, eps=1e-10, out=p):
        return lib.seld_spatial_features(z, C, bins, frames, kind, layout, fb, lo, hi, bands, eps, out, None)
    assert call(z=None) == EINVAL and call(out=None) == EINVAL
    assert call(C=6) == EINVAL and call(C=6, kind=1) == EINVAL and call(C=0, kind=0) == EINVAL
    assert call(kind=3) == EINVAL and call(kind=-1) == EINVAL and call(layout=2) == EINVAL
    assert call(kind=0, layout=1) == EINVAL and call(kind=1, layout=1) == EINVAL
    assert call(bins=0) == EINVAL and call(frames=0) == EINVAL and call(bands=0) == EINVAL
    assert call(eps=0.0) == EINVAL and call(eps=-1.0) == EINVAL and call(eps=float('nan')) == EINVAL
    assert call(bands=8) == EINVAL                                       # fb == NULL: bands == bins
    assert call(fb=p, bands=8) == EINVAL and call(fb=p, lo=p, bands=8) == EINVAL      # fb without its extents
    assert call(bins=1 << 16, frames=1 << 15, bands=1 << 16) == EUNSUPPORTED          # a plane of 2^31 floats
    assert call(C=65536 * 4, kind=1) == EUNSUPPORTED and call(C=65536, kind=0) == EUNSUPPORTED


def test_stft_complex_refusals_before_any_launch():
    lib = pkg()._lib.lib()
    p = ctypes.c_void_p(4096)

    def call(x=p, C=2, L=9000, nperseg=512, noverlap=128, out=p, ws=None, ws_bytes=0):
        return lib.seld_stft_complex_ws(x, C, L, nperseg, noverlap, 1, 1, None, out, ws, ws_bytes, None)
    assert call(x=None) == EINVAL and call(out=None) == EINVAL
    assert call(C=0) == EINVAL and call(L=0) == EINVAL and call(nperseg=1) == EINVAL
    assert call(noverlap=512) == EINVAL and call(noverlap=-1) == EINVAL
    assert call(nperseg=4097, noverlap=2048) == EUNSUPPORTED
    # a Bluestein length without its workspace, or with one a byte short
    need = lib.seld_stft_workspace(97)
    assert need > 0
    assert call(nperseg=97, noverlap=40) == -2 and call(nperseg=97, noverlap=40, ws=p, ws_bytes=need - 1) == -2
