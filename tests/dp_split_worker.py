"""Worker of tests/test_gpu_device_split_dp.py -- one rank of a 2-rank run fed from a DeviceSplit (both ranks on cuda:0 over gloo,
as tests/dp_worker.py: the GPU box has one GPU, the collective semantics are backend-independent).

    python -m torch.distributed.run --nproc-per-node 2 ... tests/dp_split_worker.py OUT_DIR eval|train

eval:  eval_split (CMFlow) and eval_split_clips (CMFlow-T) with (rank, world) on the splits below; each rank saves what it got.
train: two TrainStep steps on split.epoch(..., rank, world); each rank saves its batches, its LOCAL gradient bucket (copied right
       before the all-reduce), the all-reduced bucket (copied right before the optimizer step) and the final parameters.

The splits are built here, from the seeded synthetic scenes of cmflow_amd/synth.py, so that the test builds the very same ones.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SEED = 0x1234567887654321
EVAL_N1 = (40, 120, 57, 88, 101, 64, 119, 43, 75, 96)             # 10 whole frames of 40 .. 120 points
EVAL_N2 = (118, 41, 90, 66, 40, 120, 52, 99, 83, 71)
EVAL_CLIPS = [(0, 4), (4, 7), (7, 10)]                             # update_len 3: segments [0-2] [3-5] [6] [7-8] [9]
EVAL_BATCH, UPDATE_LEN = 2, 3
TRAIN_N1 = (180, 256, 400, 300, 255, 257, 330, 210)               # 8 frames around npoints = 256: two global batches of 4
TRAIN_N2 = (217, 282, 415, 226, 256, 300, 190, 260)
TRAIN_BATCH, TRAIN_POINTS, TRAIN_STEPS = 2, 256, 2


def items(n1s, n2s, seed):
    """Whole-frame 11-tuples (the layout of dataset._sample_item under ds.eval) cut from synth.make_batch scenes; frame k's
    transform is shifted by k mm so that no two frames share one."""
    from cmflow_amd import synth
    out = []
    for k, (n1, n2) in enumerate(zip(n1s, n2s)):
        b = synth.make_batch(1, N=max(n1, n2), seed=seed + k, train_extras=True)
        rows = lambda key, n: np.ascontiguousarray(b[key][0].t().numpy()[:n])
        trans = b["gt_trans"][0].numpy().copy()
        trans[0, 3] += 1e-3 * k
        out.append((rows("pc1", n1), rows("pc2", n2), rows("ft1", n1), rows("ft2", n2), trans, b["flow_label"][0].numpy()[:n1],
                    b["fg_mask"][0].numpy()[:n1], 0.1, b["radar_u"][0].numpy()[:n1], b["radar_v"][0].numpy()[:n1],
                    b["opt_flow"][0].numpy()[:n1]))
    return out


def eval_split_of(dev):
    from cmflow_amd.dataset import DeviceSplit
    return DeviceSplit.from_items(items(EVAL_N1, EVAL_N2, 4100), dev, clips=EVAL_CLIPS)


def train_split_of(dev):
    from cmflow_amd.dataset import DeviceSplit
    return DeviceSplit.from_items(items(TRAIN_N1, TRAIN_N2, 5200), dev)


def model(name, dev):
    import bench
    from cmflow_amd.cmflow import CMFlow, CMFlow_T
    net = {"cmflow": CMFlow, "cmflow_t": CMFlow_T}[name](bench.Args())
    net.load_state_dict(bench.load_weights(name))
    return net.to(dev)


def cpu_result(result):
    sf, seg, pose, gt, pre = result
    return {"metrics": {k: v.cpu() for d in (sf, seg, pose) for k, v in d.items()}, "gt_trans_all": gt.cpu(), "pre_trans_all": pre.cpu()}


def run_eval(dev, rank, world):
    from cmflow_amd import evaluate as EV
    split = eval_split_of(dev)
    seen, seen_t = [], []
    whole = EV.eval_split(model("cmflow", dev).train(), split, EVAL_BATCH, on_batch=lambda b, o: seen.append(b["frames"].tolist()),
                          rank=rank, world=world)
    clips = EV.eval_split_clips(model("cmflow_t", dev).train(), split, EVAL_BATCH, UPDATE_LEN,
                                on_batch=lambda b, o: seen_t.append(b["frames"].tolist()), rank=rank, world=world)
    return {"eval_split": cpu_result(whole), "eval_split_clips": cpu_result(clips), "batches": seen, "clip_batches": seen_t}


def run_train(dev, rank, world):
    import bench
    from cmflow_amd.dp import broadcast_module
    from cmflow_amd.train import TrainStep
    split = train_split_of(dev)
    net = model("cmflow", dev).train()
    broadcast_module(net)
    step = TrainStep(net, vr_thres=bench.Args.vr_thres)
    step.overlap_allreduce = False                  # one all-reduce after backward: the local bucket is whole right before it
    kept = {}
    reduce_, opt_step = step.bucket.all_reduce_mean, step.opt.step
    step.bucket.all_reduce_mean = lambda *a, **k: (kept.update(local=step.bucket.flat.detach().clone()), reduce_(*a, **k))[1]
    step.opt.step = lambda: (kept.update(averaged=step.bucket.flat.detach().clone()), opt_step())[1]
    steps = []
    for batch in split.epoch(TRAIN_BATCH, TRAIN_POINTS, SEED, 0, rank=rank, world=world):
        loss = step(batch)[0]
        torch.cuda.synchronize()
        steps.append({"batch": {k: v.cpu() for k, v in batch.items()}, "local": kept.pop("local").cpu(),
                      "averaged": kept.pop("averaged").cpu(), "loss": loss.cpu()})
    assert len(steps) == TRAIN_STEPS, len(steps)
    return {"steps": steps, "params": {k: v.detach().cpu() for k, v in net.named_parameters()}}


def main():
    import torch.distributed as dist
    out_dir, mode = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    rec = {"eval": run_eval, "train": run_train}[mode](dev, rank, world)
    torch.save(rec, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
