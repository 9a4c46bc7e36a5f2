"""spectrum_fast at every segment length 2 <= nperseg <= 4096 (csrc/stft.hip, csrc/stft_any.hip) against the
reference's outputs (tests/golden/stft_lengths.npz) and the float64 oracle."""

import numpy as np
import pytest
import torch

from oracle import seld_oracle as O
from tests.golden.stft_lengths_cases import STFT_LENGTH_CASES, stft_input, stft_kwargs
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check_spectrum(out, ref, C, phase, what):
    """Magnitude: 2e-6 of the largest magnitude.  Phase: 1e-3 rad wherever the bin carries signal, |Z| > 1e-3 * max|Z|
    -- below that the angle of an fp32 transform is rounding noise."""
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    top = float(np.abs(ref[:C]).max())
    assert np.abs(out[:C] - ref[:C]).max() < 2e-6 * max(1.0, top) + 2e-7, what
    if phase:
        mask = ref[:C] > 1e-3 * top
        assert mask.mean() > 0.05, what
        dphi = np.angle(np.exp(1j * (out[C:] - ref[C:])))
        assert np.abs(dphi[mask]).max() < 1e-3, (what, float(np.abs(dphi[mask]).max()))


FLAT_CASES = [c for c in STFT_LENGTH_CASES if len(c["x"]) == 2]
BATCHED_CASES = [c for c in STFT_LENGTH_CASES if len(c["x"]) == 3]


@pytest.mark.parametrize("case", FLAT_CASES, ids=[c["name"] for c in FLAT_CASES])
def test_spectrum_fast_lengths_match_reference(case, golden):
    UF = pkg().utility_functions
    ref = golden("stft_lengths")[case["name"]]
    x = stft_input(case)
    kw = stft_kwargs(case)
    C, phase = x.shape[0], kw.get("output_phase", True)
    out = UF.spectrum_fast(x, **kw)
    assert isinstance(out, np.ndarray) and out.dtype == ref.dtype
    _check_spectrum(out.astype(np.float64), ref.astype(np.float64), C, phase, case["name"])
    other = x.astype(np.float64 if x.dtype == np.float32 else np.float32)
    o2 = UF.spectrum_fast(other, **kw)
    assert o2.dtype == other.dtype
    _check_spectrum(o2.astype(np.float64), ref.astype(np.float64), C, phase, case["name"] + " other dtype")
    t = UF.spectrum_fast(torch.from_numpy(x.astype(np.float32)).to(DEV), **kw)
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
    _check_spectrum(t.cpu().double().numpy(), ref.astype(np.float64), C, phase, case["name"] + " tensor")


@pytest.mark.parametrize("case", BATCHED_CASES, ids=[c["name"] for c in BATCHED_CASES])
def test_spectrum_fast_lengths_batched(case, golden):
    """(2, 3, samples): the reference's literal axis handling (phase on axis -3, the cuts on axes 1 and 2): planes 0-1
    are the magnitudes of channels 1-2, planes 3-4 their phases."""
    UF = pkg().utility_functions
    ref = golden("stft_lengths")[case["name"]]
    out = UF.spectrum_fast(stft_input(case), **stft_kwargs(case))
    assert out.shape == ref.shape
    for n_ in range(out.shape[0]):
        _check_spectrum(np.concatenate((out[n_, :2], out[n_, 3:5])), np.concatenate((ref[n_, :2], ref[n_, 3:5])), 2,
                        True, f"batched item {n_}")


def _sweep_lengths():
    ns = set(range(2, 65))
    for k in range(1, 13):
        ns |= {1 << k, (1 << k) - 1, (1 << k) + 1}
    rng = np.random.RandomState(7)
    ns |= set(int(n) for n in rng.choice(np.arange(65, 4097), 40, replace=False))
    return sorted(n for n in ns if 2 <= n <= 4096)


@pytest.mark.parametrize("N", _sweep_lengths())
def test_spectrum_fast_length_sweep(N):
    """Every N in 2..64, the powers of two up to 4096 and their neighbours, 40 seeded N in (64, 4096]: seeded noise at
    a seeded overlap against the float64 oracle (of the float32-rounded input)."""
    UF = pkg().utility_functions
    rng = np.random.RandomState(N)
    noverlap = int(rng.randint(0, N))
    L = int(rng.randint(N, 4 * N + 40))
    x = rng.randn(2, L).astype(np.float32)
    out = UF.spectrum_fast(torch.from_numpy(x).to(DEV), N, noverlap).cpu().double().numpy()
    ref = O.spectrum_fast(x.astype(np.float64), N, noverlap)
    _check_spectrum(out, ref, 2, True, f"N={N} noverlap={noverlap} L={L}")


def test_spectrum_fast_full_clip_480():
    """8 channels x 60 s at 24 kHz, nperseg 480, hop 240 -> (16, 240, 6000): two stretches of frames against the oracle
    (the last 40 run into the zero padding at the end of the signal), and timed (bytes = input + output)."""
    import time
    UF = pkg().utility_functions
    N, hop, L_ = 480, 240, 24000 * 60
    rng = np.random.RandomState(11)
    x = (rng.randn(8, L_) * (0.2 + np.abs(np.sin(np.arange(L_) * 1e-5)))).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    out = UF.spectrum_fast(xd, nperseg=N, noverlap=N - hop)
    assert tuple(out.shape) == (16, 240, 6000)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        out = UF.spectrum_fast(xd, nperseg=N, noverlap=N - hop)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    nbytes = xd.numel() * 4 + out.numel() * 4
    print(f"spectrum_fast (8, 1440000) nperseg 480 -> (16, 240, 6000): {dt * 1e6:.0f} us, {nbytes / dt / 1e9:.0f} GB/s")
    # a stretch starting on a hop boundary 2 frames early has its frame j at global frame f0 - 2 + j; from j = 1 on no
    # frame touches the stretch's own left zero boundary
    got = out.cpu().double().numpy()
    for f0, nf in ((1000, 64), (5960, 40)):
        s0 = hop * (f0 - 2)
        s1 = min(L_, s0 + hop * (nf + 4) + N)
        ref = O.spectrum_fast(x[:, s0:s1].astype(np.float64), N, N - hop, output_phase=True, cut_last_timeframe=False)
        _check_spectrum(np.concatenate((got[:8, :, f0:f0 + nf], got[8:, :, f0:f0 + nf])),
                        np.concatenate((ref[:8, :, 2:2 + nf], ref[8:, :, 2:2 + nf])), 8, True, f"frames {f0}..{f0 + nf - 1}")


@pytest.mark.parametrize("N", [960, 997])
def test_spectrum_fast_lengths_repeatable(N):
    UF = pkg().utility_functions
    x = torch.from_numpy(np.random.RandomState(3).randn(3, 20000).astype(np.float32)).to(DEV)
    a = UF.spectrum_fast(x, N, N // 2)
    b = UF.spectrum_fast(x, N, N // 2)
    assert torch.equal(a, b)


def test_stft_refusals_write_nothing():
    """nperseg > 4096 raises; a Bluestein length without a workspace, or with one too small, returns SELD_EWORKSPACE
    and launches nothing."""
    P = pkg()
    UF, L = P.utility_functions, P._lib
    lib = L.lib()
    x = torch.randn(2, 9000, device=DEV)
    with pytest.raises(L.SeldHipError):
        UF.spectrum_fast(x, 4097, 2048)
    N, nov = 997, 500
    frames = lib.seld_stft_frames_ex(9000, N, nov, 1)
    out = torch.full((4, N // 2, frames), float("nan"), device=DEV)
    stream = L.current_stream()
    assert lib.seld_stft_magphase_ex(L.ptr(x), 2, 9000, N, nov, 1, 1, 1, None, L.ptr(out), stream) == -2
    need = lib.seld_stft_workspace(N)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.seld_stft_magphase_ws(L.ptr(x), 2, 9000, N, nov, 1, 1, 1, None, L.ptr(out), L.ptr(ws), need - 1,
                                     stream) == -2
    assert lib.seld_stft_magphase_ws(L.ptr(x), 2, 9000, 4097, 2048, 1, 1, 1, None, L.ptr(out), L.ptr(ws), need,
                                     stream) == -4
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
