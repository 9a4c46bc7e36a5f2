"""Host checks of the any-length STFT (csrc/stft_any.hip): the fixture of the reference's spectrum_fast at segment
lengths other than 512 against the float64 oracle (or scipy for a non-Hamming window), the frame count of
seld_stft_frames_ex against scipy.signal.stft, and the workspace query.  No device needed."""
import numpy as np
import pytest
import scipy.signal

from oracle import seld_oracle as O
from tests.golden.stft_lengths_cases import STFT_LENGTH_CASES, stft_input, stft_kwargs
from tests.helpers import pkg


@pytest.mark.parametrize("case", STFT_LENGTH_CASES, ids=[c["name"] for c in STFT_LENGTH_CASES])
def test_fixture_matches_oracle(case, golden):
    g = golden("stft_lengths")[case["name"]]
    x = stft_input(case)
    kw = stft_kwargs(case)
    assert g.dtype == (np.float32 if x.dtype == np.float32 else np.float64)
    window = kw.pop("window", "hamming")
    if window == "hamming":
        ref = O.spectrum_fast(x.astype(np.float64), **kw)
    else:
        _, _, Z = scipy.signal.stft(x.astype(np.float64), window=window, nperseg=kw["nperseg"], noverlap=kw["noverlap"])
        ref = np.concatenate((np.abs(Z), np.angle(Z)), axis=-3)[:, 1:, :-1]
    assert ref.shape == g.shape
    tol = 1e-5 if g.dtype == np.float32 else 1e-12
    top = np.abs(ref).max()
    C = x.shape[-2] if kw.get("output_phase", True) and x.ndim == 2 else ref.shape[-3]
    assert np.abs(g[..., :C, :, :] - ref[..., :C, :, :]).max() <= tol * top
    if x.ndim == 2 and kw.get("output_phase", True):
        mask = ref[:C] > 1e-3 * top
        dphi = np.angle(np.exp(1j * (g[C:] - ref[C:])))
        assert np.abs(dphi[mask]).max() < 1e-3


def _scipy_frames(L, N, noverlap):
    _, t, _ = scipy.signal.stft(np.zeros(L), nperseg=N, noverlap=noverlap)
    return t.size


def test_frame_count_matches_scipy():
    """seld_stft_frames_ex = scipy's frame count (minus the cut), odd and even N: the zero boundary is N // 2 on each
    side, so for odd N the extended signal is L + N - 1 long, not L + N."""
    lib = pkg()._lib.lib()
    bad = []
    for N in (2, 3, 4, 5, 7, 8, 9, 64, 255, 256, 480, 481, 997, 999, 1000, 1001, 4095):
        for nov in sorted({0, 1, N // 4, N // 2, N - 2, N - 1} & set(range(N))):
            for L in (N, N + 1, 2 * N + 3, 6400, 7 * N + N // 3):
                want = _scipy_frames(L, N, nov)
                for cut in (0, 1):
                    got = lib.seld_stft_frames_ex(L, N, nov, cut)
                    if got != want - cut:
                        bad.append((L, N, nov, cut, got, want - cut))
    assert not bad, bad[:10]
    assert lib.seld_stft_frames_ex(6400, 481, 480, 0) == _scipy_frames(6400, 481, 480)


def test_workspace_query():
    """0 for the lengths the power-of-two kernels and the 7-smooth transform take, positive for the Bluestein lengths
    (the chirp and its spectrum), the same on every call."""
    lib = pkg()._lib.lib()
    for N in (4, 8, 16, 32, 64, 128, 256, 512, 1024):
        assert lib.seld_stft_workspace(N) == 0, N
    for N in (2, 3, 6, 480, 882, 960, 1000, 1764, 2048, 4096):
        assert lib.seld_stft_workspace(N) == 0, N
    for N in (11, 13, 997, 1023, 4095):
        ws = lib.seld_stft_workspace(N)
        M = 1 << int(np.ceil(np.log2(2 * N - 1)))
        assert ws >= 8 * (M + N), (N, ws)
        assert all(lib.seld_stft_workspace(N) == ws for _ in range(3))
