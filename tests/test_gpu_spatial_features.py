"""stft_complex, hip_ops.spatial_features and utility_functions.seld_features (csrc/stft.hip, csrc/stft_any.hip,
csrc/spatial_features.hip) against the float64 statement of tests/spatial_features_ref.py: the complex spectra to DELTA
of the largest bin, every feature element to the bound propagated from DELTA (no free tolerance), plane waves against
their closed form, exact symmetries, a user-supplied filterbank, refusals and conventions."""
import functools

import numpy as np
import pytest
import torch

from tests import spatial_features_ref as R
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# max |Z_hip - Z_ref| / max |Z_ref| measured on the MI355X over the variants of each case (DESIGN.md has the run):
#   radix8_512 1.098e-07, radix2_64 7.442e-08, smooth_480 1.352e-07, bluestein_97 1.976e-07
# DELTA = 4 x the largest, rounded up to one significant digit; it must stay <= 2e-6, what the magnitude is held to.
DELTA = 8e-7
assert DELTA <= 2e-6


def _dev(a):
    return torch.tensor(a, device=DEV)


def _kw(case, variant):
    return dict(nperseg=case[0], noverlap=case[1], cut_dc=variant[1], cut_last_timeframe=variant[2])


@functools.lru_cache(maxsize=None)
def _device_spectrum(case, variant):
    UF = pkg().utility_functions
    x = _dev(R.case_input(case)[:variant[0]])
    return UF.stft_complex(x, **_kw(case, variant))


def _fb(case, variant, mel):
    return R.case_fb(case, variant[1]) if mel else None


def _assert_within(got, ref, tol, what):
    """Per element |got - ref| <= tol, after the caps that keep the bound from hiding a failure."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    wide = float((tol > 1e-2).mean())
    med = float(np.median(tol))
    err = np.abs(got - ref)
    ratio = np.divide(err, tol, out=np.where(err > 0, np.inf, 0.0), where=tol > 0)       # an allowed error of 0: exact
    worst = float(ratio.max())
    print(f"{what}: worst error / allowed {worst:.3f}, allowed > 1e-2 on {100 * wide:.3f} %, median allowed {med:.2e}")
    assert wide <= 2e-3 and med < 1e-3, (what, wide, med)
    assert np.isfinite(got).all(), what
    assert worst <= 1.0, (what, worst, np.unravel_index(ratio.argmax(), err.shape))


# ---- 1: the complex spectra -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_complex_spectra(case):
    worst = 0.0
    for variant in R.VARIANTS:
        ref = R.case_spectrum(case, variant)
        z = _device_spectrum(case, variant)
        assert z.dtype == torch.complex64 and z.is_cuda and tuple(z.shape) == ref.shape, (variant, z.shape, ref.shape)
        top = np.abs(ref).max()
        rel = float(np.abs(z.cpu().numpy().astype(np.complex128) - ref).max() / top)
        print(f"{R.CASE_IDS[R.CASES.index(case)]} {variant}: max |Z_hip - Z_ref| / top = {rel:.3e} (top {top:.3e})")
        worst = max(worst, rel)
    assert worst <= DELTA, worst


def test_complex_spectra_follow_spectrum_fast():
    """|Z| and angle(Z) of the complex form against the magnitude / phase form of the same transform, a window table
    and batch axes included (the reference is spectrum_fast itself: same kernels, other epilogue)."""
    UF = pkg().utility_functions
    case = R.CASES[2]
    x = _dev(R.case_input(case)[:6])
    for window in ('hamming', 'hann'):
        z = UF.stft_complex(x.view(2, 3, -1), case[0], case[1], window=window)
        mp = UF.spectrum_fast(x, case[0], case[1], window=window)
        assert tuple(z.shape) == (2, 3) + tuple(mp.shape[1:])
        z = z.reshape((6,) + tuple(mp.shape[1:]))
        top = float(mp[:6].max())
        assert float((z.abs() - mp[:6]).abs().max()) <= 8 * R.U24 * top
        strong = mp[:6] > 1e-3 * top
        dphi = torch.angle(z * torch.polar(torch.ones_like(mp[6:]), -mp[6:]))
        assert float(dphi[strong].abs().max()) < 1e-5


# ---- 2: the features, per element -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mel", [True, False], ids=["mel", "linear"])
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_features_within_the_propagated_bound(case, mel):
    H = pkg().hip_ops
    for variant in R.VARIANTS:
        Z = R.case_spectrum(case, variant)
        d = DELTA * np.abs(Z).max()
        fb = _fb(case, variant, mel)
        for kind, layout in R.FORMS:
            ref, tol = R.features(Z, kind, layout, fb, 1e-10, d)
            out = H.spatial_features(_device_spectrum(case, variant), kind, layout, fb=fb)
            assert out.dtype == torch.float32 and out.is_cuda
            _assert_within(out.cpu().double().numpy(), ref, tol, f"{R.CASE_IDS[R.CASES.index(case)]} {variant} {kind}/{layout}")


def test_logpower_of_channel_counts_off_four():
    """Log-power alone takes any channel count."""
    H = pkg().hip_ops
    case, variant = R.CASES[1], (8, True, True)
    Z = R.case_spectrum(case, variant)[:5]
    z = _device_spectrum(case, variant)[:5]
    for fb in (None, _fb(case, variant, True)):
        ref, tol = R.features(Z, "logpower", "grouped", fb, 1e-10, DELTA * np.abs(Z).max())
        _assert_within(H.spatial_features(z, "logpower", fb=fb).cpu().double().numpy(), ref, tol, "5 channels")


# ---- 3: plane waves ---------------------------------------------------------------------------------------------------
GAINS = ((0.5, -0.25, 0.125), (-1.0, 0.5, 2.0))      # powers of two: s * g is exact in float32


@pytest.mark.parametrize("case", R.CASES[:1] + R.CASES[3:], ids=R.CASE_IDS[:1] + R.CASE_IDS[3:])
def test_plane_wave_direction(case):
    """x = s (1, a, b, c) per group: I_d = g_d |W|^2 / (eps + |W|^2 (1 + (a^2 + b^2 + c^2) / 3)).  eps = 1e-20 is far below
    every |W|^2 the test looks at (> 1e-6 of the largest), so this is g_d / (1 + (a^2 + b^2 + c^2) / 3) to the bound."""
    UF = pkg().utility_functions
    nperseg, noverlap, L, n_mels, sr = case
    s = (np.random.RandomState(nperseg + 1).randn(2, L) * 0.3).astype(np.float32)
    x = np.concatenate([s[g:g + 1] * np.array((1.0,) + GAINS[g], np.float32)[:, None] for g in range(2)])
    Z = R.spectrum(x, nperseg, noverlap, True, True)
    d, eps = DELTA * np.abs(Z).max(), 1e-20
    want = np.array([[g_d / (1.0 + sum(v * v for v in g) / 3.0) for g_d in g] for g in GAINS])          # (2, 3)
    kw = dict(nperseg=nperseg, noverlap=noverlap, sr=sr, eps=eps, kind="iv")
    lin = UF.seld_features(_dev(x), **kw).cpu().double().numpy().reshape(2, 3, *Z.shape[1:])
    c = R.components(Z, None, eps, d)
    W2 = np.abs(Z[0::4]) ** 2
    for g in range(2):
        keep = W2[g] > 1e-6 * W2[g].max()
        assert keep.mean() > 0.9
        for i in range(3):
            assert (np.abs(lin[g, i] - want[g, i])[keep] <= c["iv_tol"][g, i][keep]).all(), (g, i)
    fb = R.case_fb(case, True)
    mel = UF.seld_features(_dev(x), n_mels=n_mels, **kw).cpu().double().numpy()
    cm = R.components(Z, fb, eps, d)
    mel = mel.reshape(cm["iv"].shape)
    assert (np.abs(mel - want[:, :, None, None] * fb.sum(axis=1)[None, None, :, None]) <= cm["iv_tol"]).all()


# ---- 4: exact symmetries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_exact_symmetries(case):
    UF = pkg().utility_functions
    nperseg, noverlap, L, n_mels, sr = case
    x = _dev(R.case_input(case))
    for mels in (n_mels, 0):
        kw = dict(nperseg=nperseg, noverlap=noverlap, n_mels=mels, sr=sr)
        grouped = UF.seld_features(x, layout="grouped", **kw)                    # 8 log-power planes, then 2 x 3 IV planes
        assert torch.equal(grouped, UF.seld_features(x, layout="grouped", **kw))
        quat = UF.seld_features(x, layout="quaternion", **kw)
        assert quat.shape[0] == 8
        for g in range(2):
            assert torch.equal(quat[4 * g], grouped[4 * g])
            assert torch.equal(quat[4 * g + 1:4 * g + 4], grouped[8 + 3 * g:8 + 3 * g + 3])
        assert torch.equal(UF.seld_features(x, kind="logpower", **kw), grouped[:8])
        assert torch.equal(UF.seld_features(x, kind="iv", **kw), grouped[8:])
        # negating one directional channel negates its intensity plane and nothing else
        for ch in (1, 6):
            xn = x.clone()
            xn[ch] = -xn[ch]
            flipped = UF.seld_features(xn, layout="grouped", **kw)
            plane = 8 + 3 * (ch // 4) + ch % 4 - 1
            want = grouped.clone()
            want[plane] = -want[plane]
            assert torch.equal(flipped, want), (mels, ch)
        # four channels alone are the first group of eight; a batch is its items
        four = UF.seld_features(x[:4], layout="grouped", **kw)
        assert torch.equal(four, torch.cat((grouped[:4], grouped[8:11])))
        for layout, kind in (("grouped", "logpower_iv"), ("quaternion", "logpower_iv"), ("grouped", "iv")):
            both = UF.seld_features(x.view(2, 4, L), kind=kind, layout=layout, **kw)
            for item in range(2):
                assert torch.equal(both[item], UF.seld_features(x[4 * item:4 * item + 4], kind=kind, layout=layout, **kw))


# ---- 5: a filterbank that is no triangle ------------------------------------------------------------------------------
def test_user_supplied_filterbank():
    H = pkg().hip_ops
    case, variant = R.CASES[2], (8, True, True)
    Z = R.case_spectrum(case, variant)
    bins = Z.shape[1]
    rng = np.random.RandomState(5)
    fb = rng.rand(11, bins) * (rng.rand(11, bins) < 0.3)
    fb[3] = 0.0
    fb[3, [10, 11, 50, 51]] = (0.7, 0.2, 1.5, 0.1)      # an interior zero stretch
    fb[7] = 0.0                                           # an all-zero band
    fb[9, :] = rng.rand(bins)                             # a band over every bin
    fb /= fb.sum(axis=1).max()                            # weights of a filterbank's size: the bound scales with them
    d = DELTA * np.abs(Z).max()
    for kind, layout in R.FORMS:
        ref, tol = R.features(Z, kind, layout, fb, 1e-10, d)
        out = H.spatial_features(_device_spectrum(case, variant), kind, layout, fb=fb).cpu()
        _assert_within(out.double().numpy(), ref, tol, f"user fb {kind}/{layout}")
    out = H.spatial_features(_device_spectrum(case, variant), "logpower_iv", "grouped", fb=fb).cpu()
    log_eps = float(np.log(1e-10))
    assert float((out[:8, 7].double() - log_eps).abs().max()) <= 8 * R.U24 * abs(log_eps)
    assert (out[:8, 7] == out[0, 7, 0]).all() and (out[8:, 7] == 0).all()


# ---- 6: refusals ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    P = pkg()
    UF, H, L = P.utility_functions, P.hip_ops, P._lib
    lib, stream = L.lib(), L.current_stream()
    out = torch.full((16, 24, 28), float("nan"), device=DEV)
    z = torch.randn(12, 24, 28, device=DEV)
    assert lib.seld_spatial_features(L.ptr(z), 6, 24, 28, 1, 0, None, None, None, 24, 1e-10, L.ptr(out), stream) == -1
    assert lib.seld_spatial_features(L.ptr(z), 6, 24, 28, 2, 0, None, None, None, 24, 1e-10, L.ptr(out), stream) == -1
    x = torch.randn(2, 1500, device=DEV)
    N, nov = 97, 40
    assert lib.seld_stft_frames_ex(1500, N, nov, 1) == 27 and out.numel() >= 4 * 48 * 27
    need = lib.seld_stft_workspace(N)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.seld_stft_complex_ws(L.ptr(x), 2, 1500, N, nov, 1, 1, None, L.ptr(out), L.ptr(ws), need - 1, stream) == -2
    assert lib.seld_stft_complex_ws(L.ptr(x), 2, 1500, N, nov, 1, 1, None, L.ptr(out), None, 0, stream) == -2
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    zc = torch.complex(z[:8], z[:8])
    for kw in (dict(kind="power"), dict(layout="dual"), dict(fb=np.ones((4, 23))), dict(eps=0.0), dict(eps=-1.0),
               dict(layout="quaternion", kind="iv"), dict(layout="quaternion", kind="logpower")):
        with pytest.raises(ValueError):
            H.spatial_features(zc, **kw)
    with pytest.raises(ValueError):
        UF.seld_features(x, kind="iv")                   # two channels are no FOA group


# ---- 7: conventions ---------------------------------------------------------------------------------------------------
def test_numpy_in_numpy_out():
    UF = pkg().utility_functions
    case = R.CASES[1]
    x = np.array(R.case_input(case))
    kw = dict(nperseg=case[0], noverlap=case[1], n_mels=case[3], sr=case[4], layout="quaternion")
    a = UF.seld_features(x, **kw)
    b = UF.seld_features(_dev(x), **kw)
    frames = pkg()._lib.lib().seld_stft_frames_ex(case[2], case[0], case[1], 1)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (8, case[3], frames)
    assert torch.is_tensor(b) and b.is_cuda and b.dtype == torch.float32
    assert np.array_equal(a, b.cpu().numpy())
