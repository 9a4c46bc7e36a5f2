#!/usr/bin/env python3
"""Micro-benchmark of the feature chain on an 8 channel x 60 s clip at 32 kHz (HIP events, same stream), nperseg 512
(noverlap 128, the reference's) and 480 (noverlap 240): the transform in its complex form against
spectrum_fast(output_phase=True) -- the same bytes written, no sqrt / atan2 --, and the feature launch of
csrc/spatial_features.hip, 64 mel bands and linear frequency.  Bytes of the feature launch = z read once + out.
Every timing is taken `--runs` times (default 3) so the spread is on the same line.
   python tools/features_bench.py [--iters 20] [--runs 3] [--spectrum-fast-only]
--spectrum-fast-only times spectrum_fast alone: what a commit without the complex form can run."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402

UF, H = seld_amd.utility_functions, seld_amd.hip_ops
SR, SECONDS, CHANNELS, N_MELS = 32000, 60, 8, 64
SEGMENTS = [(512, 128), (480, 240)]


def timed(f, iters):
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spectrum-fast-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    x = torch.randn(CHANNELS, SECONDS * SR, device=dev, generator=torch.Generator(device=dev).manual_seed(0))

    def runs(f):
        return [round(timed(f, args.iters), 1) for _ in range(args.runs)]

    for N, nov in SEGMENTS:
        mp = UF.spectrum_fast(x, N, nov)
        row = dict(nperseg=N, noverlap=nov, out=list(mp.shape), out_mbytes=round(mp.numel() * 4 / 1e6, 1),
                   spectrum_fast_us=runs(lambda: UF.spectrum_fast(x, N, nov)))
        if not args.spectrum_fast_only:
            def planes():
                return UF._stft_planes("features_bench", x, N, nov, 'hamming', True, True, 'complex')
            row["stft_complex_planes_us"] = runs(planes)                                  # the launch spectrum_fast's is
            row["stft_complex_us"] = runs(lambda: UF.stft_complex(x, N, nov))             # + interleaving to complex64
        print(json.dumps(row), flush=True)
        if args.spectrum_fast_only:
            continue
        z = planes()
        for n_mels in (N_MELS, 0):
            tables = H._mel_tables(float(SR), N, n_mels, 0.0, None, True, dev) if n_mels else None
            for kind, layout in (("logpower_iv", "quaternion"), ("logpower_iv", "grouped"), ("logpower", "grouped")):
                k, l = H.FEATURE_KINDS[kind], H.FEATURE_LAYOUTS[layout]

                def launch():
                    return H._features_of_planes("features_bench", z, (), CHANNELS, k, l, tables, 1e-10)
                out = launch()
                nbytes = 4 * (z.numel() + out.numel())
                us = runs(launch)
                print(json.dumps(dict(nperseg=N, n_mels=n_mels, kind=kind, layout=layout, out=list(out.shape),
                                      mbytes=round(nbytes / 1e6, 1), us=us, gbs=round(nbytes / min(us) / 1e3, 1))),
                      flush=True)
            kw = dict(nperseg=N, noverlap=nov, n_mels=n_mels, sr=SR, layout="quaternion")
            print(json.dumps(dict(nperseg=N, n_mels=n_mels, seld_features_us=runs(lambda: UF.seld_features(x, **kw)))),
                  flush=True)


if __name__ == "__main__":
    main()
