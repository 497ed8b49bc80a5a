"""The ragged TRAINING batches of tests/test_gpu_ragged_train.py and tests/test_ragged_train_host.py (a test fixture, not a test): the
frames of tests/ragged_loss_case.py (sample i of synth.make_batch(B, 300, seed, train_extras=True) truncated to its counts), the
reference gradient of a ragged step -- the mean over the samples of the CPU oracle's B = 1 eval-mode-BatchNorm gradients on the
truncated samples, in fp32 or fp64 -- and the gradient comparison of tests/test_gpu_model.py::_check_gradients with every bound a
parameter.  tests/ragged_train_grad_floor.py measures the oracle's own fp32-vs-fp64 distance for exactly these mean gradients
(profiles/ragged_train_grad_floor.txt); FLOORS below are those figures."""
import contextlib
import os

import torch

import ragged_loss_case as RC
from cmflow_amd import synth
from oracle import cmflow_oracle as O, ops, train_oracle as TO

DEFAULT_BOUNDS = (1e-2, 2e-4, 6e-2)                     # tests/test_gpu_model.py::_check_gradients: norm, 1 - cos, largest element
WHOLE_GRADIENT_BOUND = (6e-3, 2e-5)                     # tests/test_gpu_model.py: the concatenated gradient, relative error and 1 - cos
SECOND_FRAME_BOUNDS = (1.5e-2, 1e-3, 0.12)              # test_full_size_cmflow_t_clip_matches_oracle: frames behind the first ...
SECOND_FRAME_MP = (("mp.",), (4e-2, 5e-3, 0.4))         # ... and the motion head there
SEED_T2 = 4                                            # second frame of the CMFlow-T clip: RC.make_case(COUNTS5, 4), both classes per sample
CASES = {"counts6": (RC.COUNTS6, RC.SEED6), "counts5": (RC.COUNTS5, RC.SEED5)}
# The oracle's fp32 mean gradient against its fp64 mean gradient (tests/ragged_train_grad_floor.py, 8 threads): worst tensor's
# (norm, 1 - cos, element), then the whole vector's (relative error, 1 - cos).  Two correct fp32 evaluations cannot agree tighter.
FLOORS = {
    "counts6": ((8.4e-05, 7.55e-07, 0.00766), (7.33e-05, 2.68e-09)),
    # sample (33, 9) of COUNTS5 saturates the motion head: in fp32 a score rounds to exactly 0 or 1 and the class-balanced BCE runs into
    # its log clamp (maskLoss 25.29 in fp32, 7.33 in fp64; totals 256.79 vs 238.83), so the motion head's fp32 and fp64 gradients differ
    # -- the floor of this case is that of the clamp, not of summation order
    "counts5": ((0.3, 0.0228, 0.356), (0.00425, 8.7e-06)),
    "clip_t": ((0.0197, 0.000495, 0.0493), (0.0013, 7.96e-07)),
}


CLAMP_FLOORED = ("counts5",)                            # cases whose fp32-vs-fp64 floor is the BCE clamp of a saturated score


def bounds_for(case, default=DEFAULT_BOUNDS, ref_dtype=torch.float64):
    """Each bound: the larger of the project's default and 3 x the measured floor (the margin _check_gradients documents for the
    summation-order dependence of the cancellation-prone column sums).  Against the FP32 reference a CLAMP_FLOORED case keeps the
    project's defaults: its floor is not summation order but a score that saturates in fp32 and not in fp64, an fp32 implementation
    saturates like the fp32 oracle, and at 3 x that floor (0.9 / 0.068 / 1.07) the per-tensor check would hold nothing.
    -> (per-tensor bounds, whole-gradient bounds)"""
    if ref_dtype == torch.float32 and case in CLAMP_FLOORED:
        return default, WHOLE_GRADIENT_BOUND
    ft, fw = FLOORS[case]
    return (tuple(max(d, 3.0 * f) for d, f in zip(default, ft)), tuple(max(d, 3.0 * f) for d, f in zip(WHOLE_GRADIENT_BOUND, fw)))


def weights(t=False):
    import json
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    man = json.load(open(os.path.join(gold, "state_manifest_cmflow_t.json" if t else "state_manifest_cmflow.json")))
    return synth.synth_state_dict(man, seed=1234, calib=os.path.join(gold, "bn_calib_cmflow_t.npz" if t else "bn_calib_cmflow.npz"))


class Args:
    num_points, stat_thres, vr_thres = 256, 0.5, 0.3


def stable_topk(x, k, dim=-1, largest=False, sorted=True):
    """tests/test_gpu_loss.py::_stable_topk: ties among equal distances go to the lowest index, as in the kernels."""
    assert not largest
    v, i = torch.sort(x, dim=dim, stable=True)
    return v.narrow(dim, 0, k), i.narrow(dim, 0, k)


def _gather_group(points, idx):
    B, N, K = idx.shape
    return torch.gather(points.unsqueeze(1).expand(B, N, points.shape[1], points.shape[2]), 2,
                        idx.long().unsqueeze(-1).expand(B, N, K, points.shape[2]))


@contextlib.contextmanager
def oracle_patches():
    """torch.topk stable (the loss's smoothness neighbours); the oracle's C ops dtype-generic as tests/grad_noise_floor.py makes them:
    index ops on fp32 coordinates, grouping through gather / scatter_add in any other dtype than fp32."""
    keep = (torch.topk, ops.ball_query, ops.knn, ops.group_points, ops.group_points_grad, TO.index_points_group)
    bq0, knn0, gp0, gpg0, ipg0 = keep[1:]

    def gp(points, idx):
        if points.dtype == torch.float32:
            return gp0(points, idx)
        B, C, N = points.shape
        _, P, S = idx.shape
        return torch.gather(points, 2, idx.long().view(B, 1, P * S).expand(-1, C, -1)).view(B, C, P, S)

    def gpg(go, idx, N):
        if go.dtype == torch.float32:
            return gpg0(go, idx, N)
        B, C, P, S = go.shape
        out = torch.zeros(B, C, N, dtype=go.dtype)
        out.scatter_add_(2, idx.long().view(B, 1, P * S).expand(-1, C, -1), go.reshape(B, C, P * S))
        return out

    torch.topk = stable_topk
    ops.ball_query = lambda r, ns, xyz, new: bq0(r, ns, xyz.float(), new.float())
    ops.knn = lambda ns, xyz, new, return_dist=False: knn0(ns, xyz.float(), new.float(), return_dist)
    ops.group_points, ops.group_points_grad = gp, gpg
    TO.index_points_group = lambda p, i: ipg0(p, i) if p.dtype == torch.float32 else _gather_group(p, i)
    try:
        yield
    finally:
        torch.topk, ops.ball_query, ops.knn, ops.group_points, ops.group_points_grad, TO.index_points_group = keep


def truncated(batch, counts, i):
    """Sample i of the full-size batch truncated to its counts, as a B = 1 batch."""
    return RC.sample(batch, {"pred_f": batch["pc1"], "pre_trans": batch["gt_trans"], "mseg_pre": batch["pc1"][:, :1]}, counts, i)[0]


def padded(batch, counts, nmax1, nmax2, fill="big", fill_seed=0):
    """The ragged batch dict (CPU): valid slots from `batch`; behind a sample's count +-1e4 (fill 'big') or zeros."""
    stand_in = {"pred_f": batch["pc1"], "pre_trans": batch["gt_trans"], "mseg_pre": batch["pc1"][:, :1]}
    pb, _ = RC.padded(batch, stand_in, counts, nmax1, nmax2, fill_seed=fill_seed)
    if fill == "zeros":
        for k, v in pb.items():
            col = 0 if (k in ("pc1", "ft1") or k in RC.ROW_KEYS1) else (1 if k in ("pc2", "ft2") else None)
            if col is None:
                continue
            for i, c in enumerate(counts):
                if k in RC.ROW_KEYS1:
                    v[i, c[col]:] = 0
                else:
                    v[i, :, c[col]:] = 0
    return pb


def oracle_sample_step(ref, b, dtype, gfeat=None):
    """The oracle's B = 1 training step (labels -> forward('train') -> loss -> backward, no optimizer) on one truncated sample with the
    network as it stands (eval mode: BatchNorm on its running statistics).  -> total, items, outputs"""
    b = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in b.items()}
    P, Tcr = torch.as_tensor(synth.CAMERA_PROJECTION, dtype=dtype), torch.as_tensor(synth.T_CAMERA_RADAR, dtype=dtype)
    dyn, mseg = TO.make_labels(b)
    if gfeat is None and not hasattr(ref, "gru"):
        out = ref(b["pc1"], b["pc2"], b["ft1"], b["ft2"], mseg, "train")
    else:
        out = ref(b["pc1"], b["pc2"], b["ft1"], b["ft2"], mseg, "train", gfeat)
    total, items = TO.radar_flow_loss(b, out[0], out[2], out[1], mseg, dyn, P, Tcr)
    return total, items, out


def oracle_mean_gradient(sd, batch, counts, dtype, t=False, batch2=None):
    """The reference of a ragged step: mean over the samples of the oracle's B = 1 eval-mode gradients on the truncated samples.
    t: CMFlow-T; batch2: a second frame -- the clip's loss is frame 1 + frame 2 with the recurrent feature handed over UNdetached, so
    the second frame's loss reaches the first frame's parameters through gfeat.
    -> (grads: name -> fp64 tensor or None, per-sample totals, per-sample items, per-sample outputs of the (last) frame)"""
    ref = (O.CMFlow_T if t else O.CMFlow)(Args())
    ref.load_state_dict(sd)
    ref = ref.to(dtype).eval()
    B = len(counts)
    acc = {k: None for k, _ in ref.named_parameters()}
    totals, items, outs = [], [], []
    with oracle_patches():
        for i in range(B):
            ref.zero_grad()
            total, it, out = oracle_sample_step(ref, truncated(batch, counts, i), dtype)
            if batch2 is not None:
                total2, it, out = oracle_sample_step(ref, truncated(batch2, counts, i), dtype, out[4])
                total = total + total2
            total.backward()
            for k, p in ref.named_parameters():
                if p.grad is not None:
                    g = p.grad.detach().double() / B
                    acc[k] = g.clone() if acc[k] is None else acc[k] + g
            totals.append(float(total.detach())); items.append(it); outs.append(tuple(o.detach() for o in out))
    return acc, totals, items, outs


def gradient_metrics(got, ref):
    """got, ref: name -> tensor (None: no gradient).  -> rows (name, norm error, 1 - cos, element error), (whole relative error,
    whole 1 - cos): the three per-tensor figures and the concatenated vector of _check_gradients."""
    rows, ga, gr = [], [], []
    for k, r in ref.items():
        if r is None:
            assert got[k] is None, k
            continue
        a, r = got[k].detach().double().cpu().reshape(-1), r.double().reshape(-1)
        na, nr = float(a.norm()), float(r.norm())
        en = abs(na - nr) / max(nr, 1e-3)
        ec = 1.0 - float(a @ r) / (na * nr) if nr > 1e-6 else 0.0
        ee = float((a - r).abs().max()) / max(float(r.abs().max()), 1e-6)
        rows.append((k, en, ec, ee))
        ga.append(a); gr.append(r)
    ga, gr = torch.cat(ga), torch.cat(gr)
    return rows, (float((ga - gr).norm() / gr.norm()), 1.0 - float(ga @ gr) / float(ga.norm() * gr.norm()))


def check_gradients(got, ref, what, bounds, whole_bounds, loose=None):
    """Print the worst figures, then assert every tensor within `bounds` (`loose`: (name prefixes, bounds) for named exceptions) and the
    whole vector within `whole_bounds`.  -> number of tensors compared"""
    rows, whole = gradient_metrics(got, ref)
    worst = [max(rows, key=lambda t: t[j]) for j in (1, 2, 3)]
    print("%s: %d tensors; worst norm %.3g (%s), 1 - cos %.3g (%s), element %.3g (%s); whole gradient relative error %.3g, 1 - cos %.3g"
          % (what, len(rows), worst[0][1], worst[0][0], worst[1][2], worst[1][0], worst[2][3], worst[2][0], whole[0], whole[1]))
    over = []
    for k, en, ec, ee in rows:
        bd = loose[1] if (loose is not None and k.startswith(tuple(loose[0]))) else bounds
        if en > bd[0] or ec > bd[1] or ee > bd[2]:
            over.append((k, en, ec, ee))
    assert not over, (what, "tensors over their bounds (name, norm, 1 - cos, element)", bounds, over)
    assert whole[0] <= whole_bounds[0] and whole[1] <= whole_bounds[1], (what, whole, whole_bounds)
    return len(rows)
