"""train.main with --resident_loader / --graph_step against train.main with the flags off (today's DataLoader + eager
loop): the same training run.  Tiny DQ model, dropout off, 5 pickled samples, batch 2 (two full batches and a partial
one per epoch), 2 epochs, SELD_DETERMINISTIC=1."""
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODEL_FLAGS = dict(use_cuda="True", gpu_id=0, patience=1, test_step=0, checkpoint_step=0, num_frames=8,
                   dataset_normalization="UnitNorm", n_mics=2, domain="DQ", domain_classifier="DQ", phase="False",
                   input_channels=8, time_dim=64, freq_dim=128, output_classes=14, class_overlaps=3,
                   cnn_filters="[16, 16, 16]", pool_size="[[8, 2], [8, 2], [2, 2]]", pool_time="TCN", D="[10]",
                   dilation_mode="fibonacci", G=32, U=16, V="[16, 16]", V_kernel_size=3, fc_layers="[16]",
                   fc_activations="linear", fc_dropout="Last", use_bias_conv="False", use_bias_linear="True", batch_norm="BN",
                   dropout_perc=0.0, spatial_dropout_rate=0.0, lr=1e-3, use_lr_scheduler="True", lr_scheduler_step_size=1,
                   lr_scheduler_gamma=0.5, min_lr=1e-6, TextArgs="none")


def write_pickles(directory, n_train, n_val=2):
    rng = np.random.default_rng(5)
    paths = {}
    for split, n in (("training", n_train), ("validation", n_val)):
        x = (rng.random((n, 8, 128, 64)) + 0.05).astype(np.float32)
        act = (rng.random((n, 8, 42)) < 0.15).astype(np.float32)
        loc = rng.uniform(-1, 1, (n, 8, 126)).astype(np.float32) * np.repeat(act, 3, axis=2)
        for kind, arr in (("predictors", x), ("target", np.concatenate([act, loc], axis=2))):
            paths[f"{split}_{kind}_path"] = os.path.join(str(directory), f"{split}_{kind}.pkl")
            with open(paths[f"{split}_{kind}_path"], "wb") as f:
                pickle.dump(arr, f)
    paths["test_predictors_path"] = paths["test_target_path"] = os.path.join(str(directory), "absent.pkl")
    return paths


def _main(paths, out, epochs, **extra):
    """One train.main; returns (history, the last checkpoint as written by rank 0, the checkpoint's path)."""
    T, H = pkg().train, pkg().hip_ops
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    flags = dict(MODEL_FLAGS, **paths, results_path=os.path.join(out, "res"), checkpoint_dir=os.path.join(out, "ck"),
                 batch_size=2, epochs=epochs, min_n_epochs=epochs, **extra)
    history = []
    state = T.main(T.parse_args([f"--{k}={v}" for k, v in flags.items()]), history=history)
    torch.cuda.synchronize()
    assert state["epochs"] == epochs and state["step"] == 3 * epochs
    ck_root = os.path.join(out, "ck")
    path = os.path.join(ck_root, os.listdir(ck_root)[0], "checkpoint")
    return history, torch.load(path, map_location="cpu", weights_only=False), path


_runs = {}


def _run(mode, tmp_path_factory):
    """The reference run (flags off) and the runs under test, each made once and shared, never modified."""
    if "paths" not in _runs:
        _runs["paths"] = write_pickles(tmp_path_factory.mktemp("pickles"), 5)
    if mode not in _runs:
        extra = {"off": {}, "resident": dict(resident_loader="True"),
                 "graph": dict(resident_loader="True", graph_step="True")}[mode]
        _runs[mode] = _main(_runs["paths"], str(tmp_path_factory.mktemp(mode)), 2, **extra)
    return _runs[mode]


def _tensors(ck):
    out = dict(ck["model_state_dict"])
    for i, st in ck["optimizer_state_dict"]["state"].items():
        out[f"adam.{i}.exp_avg"], out[f"adam.{i}.exp_avg_sq"], out[f"adam.{i}.step"] = st["exp_avg"], st["exp_avg_sq"], st["step"]
    return out


def _compare_graph_to_eager(a, b):
    """Integer state (num_batches_tracked, Adam's step) equal; parameters and BatchNorm statistics at the tolerance of
    tests/test_gpu_deterministic.py for recorded against eager steps.  Adam's moments: the same gradients to rounding go
    into both, so they are held to 1e-3 of the tensor's largest entry; one leaked warm-up step would add (1 - beta1) = 10 %
    of a gradient to exp_avg, and (1 - beta2) g^2 to an exp_avg_sq that holds about six such terms (17 %)."""
    for k in a:
        if not a[k].is_floating_point() or k.endswith(".step"):
            assert torch.equal(a[k], b[k]), k
        elif k.startswith("adam."):
            assert torch.allclose(b[k], a[k], rtol=1e-3, atol=1e-3 * float(a[k].abs().max())), \
                (k, float((a[k] - b[k]).abs().max()), float(a[k].abs().max()))
        else:
            assert torch.allclose(b[k], a[k], rtol=1e-6, atol=1e-7 * float(a[k].abs().max()) + 1e-12), \
                (k, float((a[k] - b[k]).abs().max()))


def test_resident_loader_run_is_bit_identical_to_the_dataloader_run(seld_env, tmp_path_factory):
    """Same batches in the same order through the same eager kernels: parameters, BatchNorm buffers, Adam moments and
    step counts, and both losses of both epochs are equal bit for bit."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    (h_off, ck_off, _), (h_res, ck_res, _) = _run("off", tmp_path_factory), _run("resident", tmp_path_factory)
    a, b = _tensors(ck_off), _tensors(ck_res)
    assert a.keys() == b.keys() and len(a) > 400
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert h_res == h_off and len(h_off) == 2, (h_res, h_off)
    drop = {"best_checkpoint"}                  # a path under each run's own directory
    assert {k: v for k, v in ck_off["state"].items() if k not in drop} == {k: v for k, v in ck_res["state"].items() if k not in drop}


def test_graph_step_run_matches_the_eager_run(seld_env, tmp_path_factory):
    """Full batches replayed, the partial batch eager between the replays, against the flags-off run, at the tolerance of
    tests/test_gpu_deterministic.py for recorded against eager steps in deterministic mode.  A warm-up step that leaked
    into the run would show in Adam's step count (7 against 6) and move every parameter by ~lr = 1e-3."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    (h_off, ck_off, _), (h_g, ck_g, _) = _run("off", tmp_path_factory), _run("graph", tmp_path_factory)
    a, b = _tensors(ck_off), _tensors(ck_g)
    assert a.keys() == b.keys()
    _compare_graph_to_eager(a, b)
    print("losses (epoch, train, val): flags off", h_off, "graph", h_g)
    assert [e for e, _, _ in h_g] == [1, 2]
    assert np.allclose([t for _, t, _ in h_g], [t for _, t, _ in h_off], rtol=1e-6, atol=0), (h_g, h_off)
    assert np.allclose([v for _, _, v in h_g], [v for _, _, v in h_off], rtol=1e-6, atol=0), (h_g, h_off)


def test_graph_step_resume_matches_the_uninterrupted_run(seld_env, tmp_path_factory):
    """One epoch, checkpoint, a new main that loads it and runs the second epoch (its recording warms up AFTER the
    load and is undone again), against two epochs in one go, both in graph mode."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    h_two, ck_two, _ = _run("graph", tmp_path_factory)
    out = str(tmp_path_factory.mktemp("resume"))
    flags = dict(resident_loader="True", graph_step="True")
    h_one, _, path = _main(_runs["paths"], out, 1, **flags)
    T = pkg().train
    history = []
    args = dict(MODEL_FLAGS, **_runs["paths"], results_path=os.path.join(out, "res"), checkpoint_dir=os.path.join(out, "ck"),
                batch_size=2, epochs=2, min_n_epochs=2, load_model=path, **flags)
    state = T.main(T.parse_args([f"--{k}={v}" for k, v in args.items()]), history=history)
    assert state["epochs"] == 2 and state["step"] == 6
    ck = torch.load(path, map_location="cpu", weights_only=False)
    a, b = _tensors(ck_two), _tensors(ck)
    _compare_graph_to_eager(a, b)
    assert np.allclose([h_one[0][1:], history[0][1:]], [h_two[0][1:], h_two[1][1:]], rtol=1e-6, atol=0), (h_one, history, h_two)


def test_graph_step_needs_the_resident_loader(tmp_path):
    T = pkg().train
    with pytest.raises(ValueError, match="resident_loader"):
        T.main(T.parse_args(["--TextArgs=none", "--graph_step=True"]))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n", [9, 11])
def test_two_rank_main_trains_replicas_and_rank0_writes_the_checkpoint(tmp_path, n):
    """2 ranks, global batch 4, graph mode.  n = 9: two full global batches per epoch, the ninth sample left out.  n = 11: a
    last batch of 3 cut to 2, one row per rank through the eager data-parallel step between the replays, one sample left
    out.  The count is printed once, by rank 0; all ranks end with identical parameters; only rank 0 wrote checkpoints.
    One rank per GPU over RCCL where two GPUs are visible, else both ranks on the one GPU over gloo (main's
    SELD_DP_BACKEND / SELD_DP_SINGLE_DEVICE), as tests/test_gpu_dp.py runs its ranks."""
    paths = write_pickles(tmp_path, n)
    steps = 2 * (2 if n == 9 else 3)
    one_gpu = {} if torch.cuda.device_count() >= 2 else dict(SELD_DP_BACKEND="gloo", SELD_DP_SINGLE_DEVICE="1")
    flags = dict(MODEL_FLAGS, **paths, results_path=str(tmp_path / "res"), checkpoint_dir=str(tmp_path / "ck"), batch_size=4,
                 epochs=2, min_n_epochs=2, resident_loader="True", graph_step="True")
    with open(tmp_path / "flags.json", "w") as f:
        json.dump(flags, f)
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                   LOCAL_RANK=str(rank), SELD_DETERMINISTIC="1", **one_gpu)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "loader_dp_worker.py"), str(tmp_path)],
                                      env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=420)[0])
            assert p.returncode == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(2))
    assert torch.equal(r0["param"], r1["param"]), "replicas diverged"
    assert r0["step"] == r1["step"] == steps and r0["step_count"] == r1["step_count"] == steps
    left = [line for line in outs[0].splitlines() if "left out" in line]
    assert len(left) == 1 and f" 1 of {n} samples" in left[0], outs[0]
    assert "left out" not in outs[1] and "epoch 1:" in outs[0] and "epoch 1:" not in outs[1]
    ck_root = str(tmp_path / "ck")
    ck = torch.load(os.path.join(ck_root, os.listdir(ck_root)[0], "checkpoint"), map_location="cpu", weights_only=False)
    assert ck["state"]["epochs"] == 2 and r0["wrote_checkpoint"] and not r1["wrote_checkpoint"]
