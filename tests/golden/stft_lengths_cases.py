"""Case table of `spectrum_fast` (utility_functions.py:129-155 of the reference) at segment lengths other than the
reference's 512, shared by the fixture generator (make_golden_stft_lengths.py, runs against the reference) and the
tests.  Pure data + seeded inputs."""
import numpy as np

# N = nperseg.  x: input shape (channels, samples), or (batch, channels, samples).  kw: spectrum_fast's flags off their
# defaults.  dtype: the input's dtype (float32 input gives the reference's float32 output).
STFT_LENGTH_CASES = [
    dict(name="n3_nov2", N=3, noverlap=2, x=(2, 40)),                                    # hop 1: noverlap = N - 1
    dict(name="n5_nov1_dc", N=5, noverlap=1, x=(2, 53), kw=dict(cut_dc=False)),
    dict(name="n6_nov3_mag", N=6, noverlap=3, x=(1, 47), kw=dict(output_phase=False)),
    dict(name="n7_nov2_last", N=7, noverlap=2, x=(2, 60), kw=dict(cut_last_timeframe=False)),
    dict(name="n480_nov240_f32", N=480, noverlap=240, x=(2, 2400), dtype="float32"),
    dict(name="n882_nov441", N=882, noverlap=441, x=(1, 3000)),                          # odd hop
    dict(name="n960_nov480_hann", N=960, noverlap=480, x=(2, 2900), kw=dict(window="hann")),
    dict(name="n1000_nov500_dc_last", N=1000, noverlap=500, x=(1, 3500),
         kw=dict(cut_dc=False, cut_last_timeframe=False)),
    dict(name="n997_nov500", N=997, noverlap=500, x=(2, 3000)),                          # prime: Bluestein, odd hop
    dict(name="n1023_nov300_mag", N=1023, noverlap=300, x=(1, 3500), kw=dict(output_phase=False)),
    dict(name="n1024_nov512", N=1024, noverlap=512, x=(1, 4000)),
    dict(name="n2048_nov1024", N=2048, noverlap=1024, x=(1, 5000)),
    dict(name="n4095_nov2047", N=4095, noverlap=2047, x=(1, 8200)),                      # Bluestein at M = 8192
    dict(name="n4096_nov2048_f32", N=4096, noverlap=2048, x=(1, 9000), dtype="float32"),
    dict(name="batched_n882_nov441", N=882, noverlap=441, x=(2, 3, 2000)),
]


def stft_input(case):
    """Seeded noise plus one sinusoid per channel (so that every frame carries signal), in the case's dtype."""
    shape = case["x"]
    rng = np.random.RandomState(sum(map(ord, case["name"])))
    n = np.arange(shape[-1])
    ch = np.arange(int(np.prod(shape[:-1]))).reshape(shape[:-1] + (1,))
    x = 0.3 * rng.randn(*shape) + np.sin(2 * np.pi * (0.013 + 0.011 * ch) * n)
    return x.astype(case.get("dtype", "float64"))


def stft_kwargs(case):
    return dict(nperseg=case["N"], noverlap=case["noverlap"], **case.get("kw", {}))
