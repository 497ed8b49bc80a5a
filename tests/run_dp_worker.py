"""Worker of tests/test_gpu_run.py -- one rank of a 2-rank ``train.fit`` (both ranks on cuda:0 over gloo, as tests/dp_split_worker.py:
the GPU box has one GPU, the collective semantics are backend-independent) -- and the place where that test's splits, models and
settings are defined, so that the test and the worker build the very same ones.

    python -m torch.distributed.run --nproc-per-node 2 ... tests/run_dp_worker.py OUT_DIR

Every rank runs fit(CMFlow, DP_EPOCHS epochs, DP_BATCH / DP_VAL_BATCH frames per rank) with ``out_dir = OUT_DIR/out<rank>`` and
saves its history, the parameters and buffers after every epoch (from on_epoch) and the modes it trained in to OUT_DIR/rank<r>.pt.
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dp_split_worker as W                                         # noqa: E402  (items(), model(): seeded synthetic scenes and weights)

SEED = 1234
NPOINTS, BATCH, VAL_BATCH, EPOCHS = 256, 4, 3, 3
TRAIN_N1 = (180, 256, 400, 300, 255, 257, 330, 210, 64, 20)       # 10 frames: two batches of 4, two frames dropped
TRAIN_N2 = (217, 282, 390, 226, 256, 300, 190, 260, 33, 120)
VAL_N1 = (40, 256, 311, 88, 257, 64, 400)                         # 7 frames: validation batches of 3, 3, 1
VAL_N2 = (118, 255, 290, 66, 256, 120, 21)
CLIP_N1 = TRAIN_N1 + (145, 290)                                    # CMFlow-T: 12 frames, clips of 7 and 5; L = 2: mini-clips at
CLIP_N2 = TRAIN_N2 + (301, 77)                                     # 0, 2, 4 | 7, 9 (frames 6 and 11 dropped) -- steps of 4 and 1
TRAIN_CLIPS = [(0, 7), (7, 12)]
VAL_CLIPS = [(0, 3), (3, 7)]                                       # mini-clips at 0 | 3, 5 (frame 2 dropped): steps of 2 and 1
MINI_CLIP_LEN, CLIP_VAL_BATCH = 2, 2
DP_BATCH, DP_VAL_BATCH, DP_EPOCHS = 2, 2, 2                        # per rank: global batches of 4 (training), 4, 3 (validation)


def train_split_of(dev):
    from cmflow_amd.dataset import DeviceSplit
    return DeviceSplit.from_items(W.items(TRAIN_N1, TRAIN_N2, 6100), dev)


def val_split_of(dev):
    from cmflow_amd.dataset import DeviceSplit
    return DeviceSplit.from_items(W.items(VAL_N1, VAL_N2, 7300), dev, clips=VAL_CLIPS)


def clip_split_of(dev):
    from cmflow_amd.dataset import DeviceSplit
    return DeviceSplit.from_items(W.items(CLIP_N1, CLIP_N2, 6100), dev, clips=TRAIN_CLIPS)


def model(name, dev):
    """A fresh network with the seeded synthetic weights, in train mode."""
    if name != "raflow":
        return W.model(name, dev).train()
    import bench
    from cmflow_amd.raflow import RaFlow
    net = RaFlow(bench.Args())
    net.load_state_dict(bench.load_weights("raflow"))
    return net.to(dev).train()


def state_of(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def main():
    import torch.distributed as dist
    from cmflow_amd.dp import broadcast_module
    from cmflow_amd.train import fit
    out_dir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    net = model("cmflow", dev)
    broadcast_module(net)
    states, modes = [], []
    net.register_forward_pre_hook(lambda m, a: modes.append(bool(m.training)) if torch.is_grad_enabled() else None)
    history = fit(net, train_split_of(dev), val_split_of(dev), epochs=DP_EPOCHS, batch_size=DP_BATCH, val_batch_size=DP_VAL_BATCH,
                  num_points=NPOINTS, seed=SEED, out_dir=os.path.join(out_dir, "out%d" % rank),
                  on_epoch=lambda e, rec: states.append({k: v.cpu() for k, v in state_of(net).items()}), rank=rank, world=world)
    torch.save({"history": history, "states": states, "modes": modes}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
