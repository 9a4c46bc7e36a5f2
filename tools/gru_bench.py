#!/usr/bin/env python3
"""Times the GRU layer (csrc/gru.hip, hip_nn.GRU) with HIP events at two shapes (B, T, I, H):

  (32, 64, 128, 128)   the benchmark clip after the CNN's pooling
  (4, 600, 128, 128)   a whole L3DAS21 clip

Per shape: the two recurrence launches alone (seld_gru_fwd with the saved tensors, seld_gru_bwd; both directions in one
launch) and the time per step they imply; forward (gradients enabled) and forward + backward of hip_nn.GRU, bidirectional,
with 1 layer and with 2 layers; and, as context only, the device time of torch.nn.GRU (MIOpen) on the same shapes and
weights.  A measurement is the mean over --reps calls between two events after a warm-up; the figure is the median of
three.  There is no pass mark.  Prints ONE JSON line and writes it to --out (default profiles/gru_bench_1.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((32, 64, 128, 128), (4, 600, 128, 128))       # (B, T, I, H)


def _median_us(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    vals = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        vals.append(e0.elapsed_time(e1) * 1e3 / reps)
    return round(statistics.median(vals), 1)


def _recurrence(B, T, H, reps, dev, g):
    import seld_amd
    L = seld_amd._lib
    lib, p = L.lib(), L.ptr
    dirs = 2
    w = [(torch.rand(3 * H, H, generator=g) * 2 - 1).to(dev) / H ** 0.5 for _ in range(dirs)]
    b = [(torch.rand(3 * H, generator=g) * 2 - 1).to(dev) / H ** 0.5 for _ in range(dirs)]
    wpack = torch.empty(int(lib.seld_gru_pack_floats(dirs, H)), device=dev)
    st = L.current_stream()
    L.check(lib.seld_gru_pack(dirs, H, p(w[0]), p(w[1]), p(b[0]), p(b[1]), p(wpack), st), "seld_gru_pack")
    gx = torch.randn(dirs, B, T, 3 * H, generator=g).to(dev)
    dy = torch.randn(B, T, dirs * H, generator=g).to(dev)
    y, h_n = torch.empty_like(dy), torch.empty(dirs, B, H, device=dev)
    n = int(lib.seld_gru_saved_floats(dirs, B, T, H))
    saved, dgx, dgh = torch.empty(n, device=dev), torch.empty_like(gx), torch.empty_like(gx)
    fwd = lambda: L.check(lib.seld_gru_fwd(dirs, B, T, H, p(gx), p(wpack), None, p(y), p(h_n), p(saved), n, st), "seld_gru_fwd")
    bwd = lambda: L.check(lib.seld_gru_bwd(dirs, B, T, H, p(dy), None, p(wpack), p(saved), n, p(dgx), p(dgh), None, st),
                          "seld_gru_bwd")
    out = {}
    for name, call, op in (("gru_fwd", fwd, 0), ("gru_bwd", bwd, 1)):
        us = _median_us(call, reps)
        out[name] = dict(kernel=seld_amd.hip_ops.gru_kernel_label(op, H), us=us, us_per_step=round(us / T, 3),
                         workgroups=dirs * ((B + 15) // 16))
    return out


def _module(make, B, T, I, H, layers, reps, dev, g, state=None):
    m = make(I, H, layers, batch_first=True, bidirectional=True)
    if state is not None:
        m.load_state_dict(state)
    m = m.to(dev).train()
    x = torch.randn(B, T, I, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(B, T, 2 * H, generator=g).to(dev)

    def fwd():
        return m(x)[0]

    def fwd_bwd():
        for q in m.parameters():
            q.grad = None
        x.grad = None
        fwd().backward(dy)
    return dict(fwd_us=_median_us(fwd, reps), fwd_bwd_us=_median_us(fwd_bwd, reps)), m.state_dict()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_bench_1.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru_bench.py needs a HIP device")
    if a.reps < 5:
        raise SystemExit("at least 5 repetitions")
    import seld_amd
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(6)
    rows = []
    for B, T, I, H in SHAPES:
        row = dict(B=B, T=T, I=I, H=H, dirs=2, recurrence=_recurrence(B, T, H, a.reps, dev, g))
        for layers in (1, 2):
            torch.manual_seed(layers)
            ours, state = _module(seld_amd.hip_nn.GRU, B, T, I, H, layers, a.reps, dev, g)
            try:
                theirs = _module(torch.nn.GRU, B, T, I, H, layers, a.reps, dev, g, {k: v.cpu() for k, v in state.items()})[0]
            except RuntimeError as e:       # context only: a build of torch without a device GRU does not stop the tool
                theirs = dict(error=str(e).splitlines()[0][:200])
            row[f"layers_{layers}"] = dict(hip_nn=ours, torch_nn=theirs)
        rows.append(row)
    line = dict(tool="gru_bench", reps=a.reps, device=torch.cuda.get_device_name(0), rows=rows)
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
