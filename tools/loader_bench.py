#!/usr/bin/env python3
"""Times the device-resident epoch loader (csrc/loader.hip, train.ResidentLoader) at config 3.

gather:  hip_ops.gather_rows of one batch (32 x 8 x 128 x 512 fp32 predictors + 32 x 64 x 168 targets) out of a resident
         array of --rows samples in a shuffled order, beside torch.index_select on the same tensors (predictors, then
         targets) and a device-to-device copy_ of the same bytes.  HIP events around each call, a warm-up, the median
         of --reps runs; bytes are the algorithmic ones (every batch byte read once and written once).
         gather_rows_aug of the same batch in three settings: nothing to apply (no table, no masks), the 8-channel FOA
         preset at p_swap = 1, and the preset at p_swap = 0.5 with two frequency masks (up to 16 bins) and two time
         masks (up to 64 frames): the same bytes, so its time stands beside gather_rows' from the same run.
main:    wall time per training step of train.main with config/BENCH_c3_DQSELD-TCN_8ch_F128.txt on synthetic pickles
         (--samples training samples, one validation batch), in three modes: flags off (DataLoader + eager step),
         --resident_loader, and --resident_loader --graph_step.  A step's time is the time from `model.train()` at the
         start of an epoch to the entry of the validation pass (device synchronised at both), over the epoch's steps;
         the first epoch of each mode is warm-up, the median of the others is reported.
Prints one JSON line per measurement."""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.3e12       # bytes/s read + written of a float4 copy kernel on an MI355X (8 TB/s is the HBM3E spec)
CONFIG = os.path.join(ROOT, "sound-event-localization-and-detection_amd", "config", "BENCH_c3_DQSELD-TCN_8ch_F128.txt")
BATCH, X_SHAPE, Y_SHAPE = 32, (8, 128, 512), (64, 168)


def device_timed(fn, reps):
    for _ in range(3):
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


def gather_part(rows, reps):
    import seld_amd
    H = seld_amd.hip_ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x_all = torch.randn((rows,) + X_SHAPE, generator=g).to(dev)
    y_all = torch.randn((rows,) + Y_SHAPE, generator=g).to(dev)
    index = torch.randperm(rows, generator=g).to(dev)
    out_x, out_y = torch.empty((BATCH,) + X_SHAPE, device=dev), torch.empty((BATCH,) + Y_SHAPE, device=dev)
    cursor = torch.ones(1, device=dev, dtype=torch.int32)
    batch = index[BATCH:2 * BATCH]
    H.gather_rows(x_all, y_all, index, out_x, out_y, cursor=cursor)
    same = bool(torch.equal(out_x, x_all[batch])) and bool(torch.equal(out_y, y_all[batch]))
    nbytes = 2 * 4 * (out_x.numel() + out_y.numel())
    src_x, src_y = x_all[:BATCH], y_all[:BATCH]
    epoch = torch.zeros(1, device=dev, dtype=torch.int32)
    preset = H.foa_transforms(mics=2)
    augments = dict(gather_rows_aug_idle=H.Augment(device=dev),
                    gather_rows_aug_swap=H.Augment(table=preset, p_swap=1.0, device=dev),
                    gather_rows_aug_swap_masks=H.Augment(table=preset, p_swap=0.5, freq_masks=2, freq_width=16, time_masks=2,
                                                         time_width=64, device=dev))

    def aug_run(augment):
        return lambda: H.gather_rows_aug(x_all, y_all, index, out_x, out_y, epoch=epoch, seed=1, augment=augment, cursor=cursor)
    aug_run(augments["gather_rows_aug_idle"])()
    same = same and bool(torch.equal(out_x, x_all[batch])) and bool(torch.equal(out_y, y_all[batch]))
    runs = dict(
        gather_rows=device_timed(lambda: H.gather_rows(x_all, y_all, index, out_x, out_y, cursor=cursor), reps),
        **{name: device_timed(aug_run(augment), reps) for name, augment in augments.items()},
        index_select=device_timed(lambda: (torch.index_select(x_all, 0, batch, out=out_x),
                                           torch.index_select(y_all, 0, batch, out=out_y)), reps),
        copy_=device_timed(lambda: (out_x.copy_(src_x), out_y.copy_(src_y)), reps))
    for r in runs.values():
        r["GBps"] = round(nbytes / (r["us"] * 1e-6) / 1e9, 1)
        r["fraction_of_copy_ceiling"] = round(nbytes / (r["us"] * 1e-6) / COPY_CEILING, 3)
        r["time_over_copy_"] = round(r["us"] / runs["copy_"]["us"], 3)      # against the copy_ measured in this very run
    print(json.dumps(dict(op="gather", rows=rows, batch=BATCH, bytes_read_plus_written=nbytes, equals_torch_indexing=same,
                          **runs)), flush=True)


def main_part(samples, epochs):
    import seld_amd
    T, H = seld_amd.train, seld_amd.hip_ops
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for split, n in (("training", samples), ("validation", BATCH)):
            x = rng.standard_normal((n,) + X_SHAPE, dtype=np.float32)
            y = np.concatenate([(rng.random((n, 64, 42)) < 0.1).astype(np.float32),
                                rng.uniform(-1, 1, (n, 64, 126)).astype(np.float32)], axis=2)
            for kind, arr in (("predictors", x), ("target", y)):
                paths[f"{split}_{kind}_path"] = os.path.join(tmp, f"{split}_{kind}.pkl")
                with open(paths[f"{split}_{kind}_path"], "wb") as f:
                    pickle.dump(arr, f, protocol=4)
        del x, y
        stamps = []

        def stamp(kind):
            torch.cuda.synchronize()
            stamps.append((kind, time.perf_counter()))

        build_model, evaluate = T.model_from_args, T.evaluate

        def model_from_args(args):
            model = build_model(args)
            train = model.train
            model.train = lambda *a, **k: (stamp("train"), train(*a, **k))[1]
            return model

        def timed_evaluate(*a, **k):
            stamp("validate")
            return evaluate(*a, **k)
        T.model_from_args, T.evaluate = model_from_args, timed_evaluate
        steps = -(-samples // BATCH)
        for mode, extra in (("flags_off", []), ("resident_loader", ["--resident_loader=True"]),
                            ("resident_loader+graph_step", ["--resident_loader=True", "--graph_step=True"])):
            del stamps[:]
            H.philox.set_offset(0)
            argv = [f"--TextArgs={CONFIG}", f"--epochs={epochs}", f"--min_n_epochs={epochs}", "--test_step=0", "--checkpoint_step=0",
                    f"--checkpoint_dir={os.path.join(tmp, mode, 'ck')}", f"--results_path={os.path.join(tmp, mode, 'res')}",
                    "--test_predictors_path=none", "--test_target_path=none"] + [f"--{k}={v}" for k, v in paths.items()] + extra
            history = []
            T.main(T.parse_args(argv), history=history)
            per_step = []
            for (k0, t0), (k1, t1) in zip(stamps[:-1], stamps[1:]):
                if k0 == "train" and k1 == "validate":
                    per_step.append((t1 - t0) / steps * 1e3)
            timed = per_step[1:]
            print(json.dumps(dict(op="main", mode=mode, samples=samples, batch=BATCH, steps_per_epoch=steps, epochs_timed=len(timed),
                                  ms_per_step=round(statistics.median(timed), 3),
                                  ms_per_step_min_max=[round(min(timed), 3), round(max(timed), 3)],
                                  first_epoch_ms_per_step=round(per_step[0], 3),
                                  train_loss_last_epoch=history[-1][1])), flush=True)
            torch.cuda.empty_cache()
        T.model_from_args, T.evaluate = build_model, evaluate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rows", type=int, default=256, help="gather: samples in the resident array (2 MB each)")
    ap.add_argument("--samples", type=int, default=256, help="main: training samples (a multiple of 32: no partial batch)")
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--skip", choices=["gather", "main"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench.py needs a HIP device")
    if a.skip != "gather":
        gather_part(a.rows, a.reps)
    if a.skip != "main":
        main_part(a.samples, a.epochs)


if __name__ == "__main__":
    main()
