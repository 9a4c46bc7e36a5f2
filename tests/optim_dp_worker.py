"""Child process of tests/test_gpu_optim.py: one data-parallel rank of the tiny model on the one GPU of the box (gloo
backend, every rank on cuda:0), training eagerly with gradient clipping, decoupled weight decay and the moving average of
the weights on.  Started fresh by the test with RANK / WORLD_SIZE / MASTER_* in the environment; writes its results to
<out_dir>/rank<r>.pt.

    python tests/optim_dp_worker.py <out_dir> <steps>
"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    out_dir, steps = sys.argv[1], int(sys.argv[2])
    import torch
    from oracle import seld_oracle as O          # closed-form fill / input only (test infrastructure)
    from tests.golden.cases import MODEL_CASES, train_target
    from tests.helpers import PKG, build_model
    pkg = importlib.import_module(PKG)
    DP, T = pkg.dp, pkg.train
    rank, _, world = DP.init_from_env("gloo")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    case = dict(next(c for c in MODEL_CASES if c["name"] == "tiny_DQ"), B=4)
    m = build_model(case)
    O.closed_form_fill_(list(m.state_dict().items()))
    if rank != 0:                                 # replicas start different: the broadcast must fix that, the average too
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(1.5)
    m = m.to(dev).train()
    DP.seed_rank_streams(rank)
    opt = T.FlatAdam(m.parameters(), lr=1e-3, late=DP.late_parameters(m), weight_decay=1e-2, decoupled=True,
                     max_grad_norm=0.05, ema_decay=0.999)
    DP.broadcast_parameters(opt.flat_param)
    opt.ema_reset()                               # as train.main does after the broadcast
    sync = DP.BucketedGradSync(opt, m)
    x = O.closed_form_input((case["B"], case["input_channels"], case["freq_dim"], case["time_dim"]))
    target = train_target(case)
    lo, hi = DP.shard_batch(case["B"])
    xs, ts = x[lo:hi].contiguous().to(dev), target[lo:hi].contiguous().to(dev)
    n_sed = int(case["output_classes"] * 3)
    losses = []
    for _ in range(steps):
        losses.append(float(DP.dp_train_step(m, opt, sync, xs, ts, n_sed, T.seld_loss_fn).item()))
    torch.cuda.synchronize()
    torch.save(dict(param=opt.flat_param.detach().cpu(), ema=opt.ema.cpu(), clip=opt.clip.cpu(), exp_avg=opt.exp_avg.cpu(),
                    losses=losses, step_count=opt.step_count), os.path.join(out_dir, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
