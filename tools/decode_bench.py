#!/usr/bin/env python3
"""Times the event decoding (csrc/decode.hip, hip_ops.decode_events) on 500 recordings x 600 frames x 42 slots at about
5 % and about 50 % active slots, beside the same decode written with stock torch ops on the device (round, nonzero,
index_select), which is what a user would otherwise write.

HIP events around each phase, a warm-up, the median of `--reps` runs.  Bytes are the algorithmic ones: the count phase
reads sed once and writes one 8-byte mask per frame; the write phase reads the masks, 12 bytes of doa per row, and
writes 44 bytes per row (the row and its event index).  Rates are given as a fraction of the 6.3 TB/s float4-copy
ceiling of DESIGN.md.  Prints one JSON line per density."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import seld_amd  # noqa: E402

H, L = seld_amd.hip_ops, seld_amd._lib
COPY_CEILING = 6.3e12
dev = torch.device("cuda:0")


def timed(fn, reps):
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
    return statistics.median(ts), min(ts), max(ts)


def torch_ops_decode(sed, doa, max_loc_value=2., max_overlaps=3):
    """The same rows with stock ops: several passes and a materialised mask."""
    R, T, n = sed.shape
    r = torch.round(sed)
    active = (r != 0) & (r.sum(-1, keepdim=True) != 0)
    idx = torch.nonzero(active.reshape(-1)).squeeze(1)                  # synchronises: the size depends on the data
    xyz = (doa.reshape(-1, 3).index_select(0, idx) * max_loc_value).double()
    slot = idx % n
    frame = (idx // n) % T
    rows = torch.cat((frame.double()[:, None], (slot // max_overlaps).double()[:, None], xyz), 1)
    counts = active.reshape(R, -1).sum(1)
    offsets = torch.cat((counts.new_zeros(1), counts.cumsum(0)))
    return rows, (slot % max_overlaps).int(), offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=500)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    R, T, classes, overlaps = a.recordings, a.frames, 14, 3
    n = classes * overlaps
    lib = L.lib()
    for density in (0.05, 0.5):
        g = torch.Generator().manual_seed(3)
        u = torch.rand(R, T, n, generator=g)
        sed = torch.where(u < density, 0.5 + 0.5 * u / density + 0.001, 0.499 * (u - density) / (1 - density)).to(dev)
        doa = (torch.rand(R, T, 3 * n, generator=g) * 2 - 1).to(dev)
        rows, event, offsets = H.decode_events(sed, doa)
        E = rows.shape[0]
        t_rows, t_event, t_offsets = torch_ops_decode(sed, doa)
        same = bool(torch.equal(rows, t_rows) and torch.equal(event, t_event) and torch.equal(offsets, t_offsets))
        nbytes = lib.seld_decode_workspace(R, T, classes, overlaps)
        ws = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
        s = L.current_stream()

        def count():
            L.check(lib.seld_decode_count(L.ptr(sed), 0, R, T, classes, overlaps, L.ptr(ws), nbytes,
                                          s), "seld_decode_count")

        def write():
            L.check(lib.seld_decode_write(L.ptr(doa), 0, R, T, classes, overlaps, 2.0, L.ptr(ws), nbytes, L.ptr(rows),
                                          L.ptr(event), E, L.ptr(offsets), s), "seld_decode_write")
        count_us = timed(count, a.reps)
        write_us = timed(write, a.reps)
        whole_us = timed(lambda: H.decode_events(sed, doa), a.reps)
        torch_us = timed(lambda: torch_ops_decode(sed, doa), a.reps)
        count_bytes = sed.numel() * 4 + R * T * 8
        write_bytes = R * T * 8 + E * (12 + 44) + (R + 1) * 8
        print(json.dumps(dict(
            shape=[R, T, n], density=density, rows=E, active_fraction=round(E / sed.numel(), 4), equals_torch_ops=same,
            count_us=round(count_us[0], 1), count_us_min_max=[round(count_us[1], 1), round(count_us[2], 1)],
            write_us=round(write_us[0], 1), write_us_min_max=[round(write_us[1], 1), round(write_us[2], 1)],
            whole_call_us=round(whole_us[0], 1), whole_call_us_min_max=[round(whole_us[1], 1), round(whole_us[2], 1)],
            torch_ops_us=round(torch_us[0], 1), torch_ops_us_min_max=[round(torch_us[1], 1), round(torch_us[2], 1)],
            torch_ops_over_whole_call=round(torch_us[0] / whole_us[0], 2),
            count_bytes=count_bytes, write_bytes=write_bytes,
            count_fraction_of_copy_ceiling=round(count_bytes / (count_us[0] * 1e-6) / COPY_CEILING, 3),
            write_fraction_of_copy_ceiling=round(write_bytes / (write_us[0] * 1e-6) / COPY_CEILING, 3),
            kernels_fraction_of_copy_ceiling=round((count_bytes + write_bytes) / ((count_us[0] + write_us[0]) * 1e-6)
                                                   / COPY_CEILING, 3))), flush=True)


if __name__ == "__main__":
    main()
