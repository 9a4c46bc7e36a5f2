#!/usr/bin/env python3
"""Times the target encoding and the segmentation (csrc/labels.hip) at the L3DAS21 shape: encode_events for 1 and 64
recordings of 600 frames x 14 x 3 slots with about 60 events each, and segment on one recording's (16, 256, 4800) float32
features and (600, 168) float64 target at the defaults of segment_task2 (24 chunks of 400 / 50, hop 200 / 25).

HIP events around each call, a warm-up, the median of `--reps` runs.  Beside the segment kernel: the same cut written with
stock torch device ops (pad + unfold + contiguous), which is what a user would otherwise write.  Bytes are the algorithmic
ones (the output written once, the source read once); rates are a fraction of the 6.3 TB/s float4-copy ceiling of
DESIGN.md.  With --reference DIR (a checkout of the reference; needs pandas and no GPU) the reference's host functions
csv_to_matrix_task2 and segment_task2 are timed on the same inputs with time.perf_counter; --host-only skips the device.
Prints one JSON line per measurement."""
import argparse
import importlib
import importlib.machinery
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.3e12


def events_of(recordings, per_rec=60, seed=0):
    """About `per_rec` events per recording that never put more than three of a class in one frame."""
    rng = np.random.RandomState(seed)
    first, last, cls, xyz, offsets = [], [], [], [], [0]
    for _ in range(recordings):
        busy = np.zeros((600, 14), dtype=np.int64)
        n = 0
        while n < per_rec:
            a = int(rng.uniform(0, 580))
            b = min(a + int(rng.uniform(1, 60)), 599)
            c = int(rng.randint(14))
            if busy[a:b + 1, c].max() >= 3:
                continue
            busy[a:b + 1, c] += 1
            first.append(a), last.append(b), cls.append(c), xyz.append(rng.uniform(-2, 2, 3))
            n += 1
        offsets.append(len(first))
    return np.asarray(first), np.asarray(last), np.asarray(cls), np.asarray(xyz), np.asarray(offsets)


def device_timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return dict(us=round(statistics.median(ts), 1), us_min_max=[round(min(ts), 1), round(max(ts), 1)])


def host_timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return dict(us=round(statistics.median(ts), 1), us_min_max=[round(min(ts), 1), round(max(ts), 1)])


def torch_ops_segment(x, seg_len, hop, segments):
    """dst[s, ..., j] = x[..., s * hop + j], zero past the end, with stock ops: pad, unfold (a view), one copy."""
    need = (segments - 1) * hop + seg_len
    if need > x.shape[-1]:
        x = torch.nn.functional.pad(x, (0, need - x.shape[-1]))
    return x.unfold(-1, seg_len, hop)[..., :segments, :].movedim(-2, 0).contiguous()


def device_part(reps):
    import seld_amd
    H, L = seld_amd.hip_ops, seld_amd._lib
    dev = torch.device("cuda:0")
    lib = L.lib()
    for R in (1, 64):
        first, last, cls, xyz, offsets = events_of(R)
        E = len(first)
        args = [torch.from_numpy(a.astype(np.int32)).to(dev) for a in (first, last, cls)]
        args += [torch.from_numpy(xyz).to(dev), torch.from_numpy(offsets.astype(np.int64)).to(dev)]
        for dtype, code in ((torch.float64, L.SELD_DECODE_F64), (torch.float32, L.SELD_DECODE_F32)):
            out = torch.empty((R, 600, 168), device=dev, dtype=dtype)
            counters = torch.zeros(2, device=dev, dtype=torch.int32)
            max_rec = int(np.diff(offsets).max())

            def kernel():
                L.check(lib.seld_encode_events(*[L.ptr(a) for a in args], E, max_rec, R, 600, 14, 3, 2.0, 0, code, L.ptr(out),
                                               L.ptr(counters), L.current_stream()), "seld_encode_events")
            k = device_timed(kernel, reps)
            whole = device_timed(lambda: H.encode_events(*args, 600, dtype=dtype), reps)
            nbytes = out.numel() * out.element_size()
            print(json.dumps(dict(op="encode_events", recordings=R, events=E, dtype=str(dtype), kernel=k, whole_call=whole,
                                  bytes_written=nbytes, counters=counters.tolist(),
                                  fraction_of_copy_ceiling=round(nbytes / (k["us"] * 1e-6) / COPY_CEILING, 4))), flush=True)
    g = torch.Generator().manual_seed(3)
    feats = torch.rand(16, 256, 4800, generator=g).to(dev)
    target = torch.rand(600, 168, generator=g, dtype=torch.float64).to(dev)
    for name, x, seg_len, hop in (("features", feats, 400, 200), ("target", target.view(168, 600), 50, 25)):
        ours = H.segment(x, seg_len, hop)
        same = bool(torch.equal(ours, torch_ops_segment(x, seg_len, hop, ours.shape[0])))
        k = device_timed(lambda: H.segment(x, seg_len, hop), reps)
        t = device_timed(lambda: torch_ops_segment(x, seg_len, hop, ours.shape[0]), reps)
        nbytes = (ours.numel() + x.numel()) * x.element_size()
        print(json.dumps(dict(op="segment", what=name, src=list(x.shape), dst=list(ours.shape), dtype=str(x.dtype), ours=k,
                              torch_ops=t, equals_torch_ops=same, torch_ops_over_ours=round(t["us"] / k["us"], 2),
                              bytes=nbytes, fraction_of_copy_ceiling=round(nbytes / (k["us"] * 1e-6) / COPY_CEILING, 3))),
              flush=True)


def reference_part(ref_dir, reps):
    sys.path.insert(0, ref_dir)
    while True:
        try:
            RUF = importlib.import_module("utility_functions")
            break
        except ModuleNotFoundError as e:            # librosa, unused by these functions: an empty stand-in
            sys.modules[e.name] = types.ModuleType(e.name)
            sys.modules[e.name].__spec__ = importlib.machinery.ModuleSpec(e.name, None)
    first, last, cls, xyz, _ = events_of(1)
    names = [f"sound_{k:02d}" for k in range(14)]
    lines = ["File,Start,End,Class,X,Y,Z"] + [f"rec,{a * 60 / 599 + 0.05:.3f},{b * 60 / 599 + 0.05:.3f},{names[c]},{p[0]:.6f},"
                                               f"{p[1]:.6f},{p[2]:.6f}" for a, b, c, p in zip(first, last, cls, xyz)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "labels.csv")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        cd = {n: i for i, n in enumerate(names)}
        print(json.dumps(dict(op="reference csv_to_matrix_task2 (host, one recording, file read included)", events=len(first),
                              **host_timed(lambda: RUF.csv_to_matrix_task2(path, cd), reps))), flush=True)
    rng = np.random.RandomState(3)
    feats = rng.rand(16, 256, 4800).astype(np.float32)
    target = rng.rand(600, 168)
    print(json.dumps(dict(op="reference segment_task2 (host, one recording)", src=[16, 256, 4800],
                          **host_timed(lambda: RUF.segment_task2(feats, target), reps))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    if not a.host_only:
        device_part(a.reps)
    if a.reference:
        reference_part(a.reference, max(3, a.reps // 4))


if __name__ == "__main__":
    main()
