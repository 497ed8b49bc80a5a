"""The ragged batches of tests/test_gpu_ragged_loss.py and tests/test_ragged_loss_host.py (a test fixture, not a test): B synthetic
frames with their own point counts -- sample i of synth.make_batch(B, full, seed, train_extras=True) truncated to (n1, n2) -- plus
network-output stand-ins as tests/test_gpu_loss.py::_case builds them, padded to (nmax1, nmax2) with large finite garbage."""
import torch

from cmflow_amd import synth

# (n1, n2) from (256, 256) down to (33, 9) as tests/test_gpu_ragged.py::MODEL_COUNTS; two samples with n1 == n2
COUNTS6 = ((256, 256), (211, 187), (97, 130), (130, 130), (64, 40), (33, 9))
COUNTS5 = ((256, 256), (211, 187), (130, 130), (64, 40), (33, 9))        # B not a power of two
SEED6, SEED5 = 2, 3              # seeds for which every truncated sample holds both motion-seg classes and a dynamic point
#                                  (tests/test_ragged_loss_host.py asserts it on the oracle's labels)
# the LDS form above 512 points, where pass 3 scans and keeps no inverse list: frames of 600 points padded to (600, 600); three samples
# with n1 == n2, 257 puts one point into a thread's second slot, (9, 9) is the smallest size both forms accept
COUNTS4, SEED4, FULL4 = ((600, 600), (513, 513), (257, 300), (9, 9)), 4, 600
POINT_KEYS1 =("pc1", "ft1", "pred_f", "gt_f", "mseg_pre")               # (B,C,N1) channel-major
ROW_KEYS1 = ("flow_label", "fg_mask", "radar_u", "radar_v", "opt_flow")  # (B,N1[,C]) point-major


def make_case(counts, seed, full=300):
    """-> (batch, outs): dicts of CPU tensors at the full size (nothing truncated or padded yet)."""
    B = len(counts)
    batch = synth.make_batch(B, full, seed=seed, train_extras=True)
    g = torch.Generator().manual_seed(seed + 7)
    gt_f = batch["flow_label"].transpose(2, 1).contiguous()
    pred_f = gt_f + 0.3 * torch.randn(B, 3, full, generator=g)
    pre_trans = batch["gt_trans"].clone()
    pre_trans[:, :3, :] += 0.01 * torch.randn(B, 3, 4, generator=g)
    mseg_pre = torch.sigmoid(2.0 * torch.randn(B, 1, full, generator=g))
    return batch, dict(pred_f=pred_f, pre_trans=pre_trans, mseg_pre=mseg_pre)


def sample(batch, outs, counts, i):
    """Sample i truncated to its counts as a B = 1 batch (what the dense kernel and the oracle take)."""
    n1, n2 = counts[i]
    b = {}
    for k, v in batch.items():
        v = v[i:i + 1]
        if k in ("pc1", "ft1"):
            v = v[:, :, :n1]
        elif k in ("pc2", "ft2"):
            v = v[:, :, :n2]
        elif k in ROW_KEYS1:
            v = v[:, :n1]
        b[k] = v.contiguous()
    o = dict(pred_f=outs["pred_f"][i:i + 1, :, :n1].contiguous(), pre_trans=outs["pre_trans"][i:i + 1].contiguous(),
             mseg_pre=outs["mseg_pre"][i:i + 1, :, :n1].contiguous())
    return b, o


def _garbage(shape, g):
    return 1e4 * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def padded(batch, outs, counts, nmax1, nmax2, fill_seed=0):
    """The ragged batch: valid slots from (batch, outs), everything behind a sample's count +-1e4 (squares and sums stay finite in
    fp32).  -> (batch dict with n1 / n2, outs dict), CPU tensors."""
    B = len(counts)
    g = torch.Generator().manual_seed(1000 + fill_seed)
    pb, po = {}, {}

    def pad(v, axis, col, nmax):
        shape = list(v.shape)
        shape[axis] = nmax
        out = _garbage(shape, g)
        for i, c in enumerate(counts):
            n = c[col]
            if axis == 2:
                out[i, :, :n] = v[i, :, :n]
            else:
                out[i, :n] = v[i, :n]
        return out

    for k, v in batch.items():
        if k in ("pc1", "ft1"):
            pb[k] = pad(v, 2, 0, nmax1)
        elif k in ("pc2", "ft2"):
            pb[k] = pad(v, 2, 1, nmax2)
        elif k in ROW_KEYS1:
            pb[k] = pad(v, 1, 0, nmax1)
        else:
            pb[k] = v.clone()
    pb["n1"] = torch.tensor([c[0] for c in counts], dtype=torch.int32)
    pb["n2"] = torch.tensor([c[1] for c in counts], dtype=torch.int32)
    po["pred_f"], po["mseg_pre"] = pad(outs["pred_f"], 2, 0, nmax1), pad(outs["mseg_pre"], 2, 0, nmax1)
    po["pre_trans"] = outs["pre_trans"].clone()
    return pb, po
