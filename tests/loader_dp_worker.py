"""Child process of tests/test_gpu_train_loader.py: one data-parallel rank of train.main.  Started fresh by the test with
RANK / WORLD_SIZE / MASTER_* in the environment; reads <dir>/flags.json, writes its results to <dir>/rank<r>.pt.

    python tests/loader_dp_worker.py <dir>
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    directory = sys.argv[1]
    import torch
    from tests.helpers import PKG
    T = importlib.import_module(PKG).train
    with open(os.path.join(directory, "flags.json")) as f:
        flags = json.load(f)
    rank = int(os.environ["RANK"])
    saves = []
    save_model = T.save_model
    importlib.import_module(PKG).checkpoint.save_model = lambda *a, **k: (saves.append(rank), save_model(*a, **k))[1]
    made = {}
    adam = T.FlatAdam
    T.FlatAdam = lambda *a, **k: made.setdefault("opt", adam(*a, **k))
    state = T.main(T.parse_args([f"--{k}={v}" for k, v in flags.items()]))
    torch.cuda.synchronize()
    opt = made["opt"]
    torch.save(dict(param=opt.flat_param.detach().cpu(), step=state["step"], step_count=opt.step_count,
                    wrote_checkpoint=bool(saves)), os.path.join(directory, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
