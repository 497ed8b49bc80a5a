"""The seven cross-modal loss terms and the label prep of the reference's training step.

Mirrors ``losses/radar_loss.py`` (RadarFlowLoss :260-292 and its components :17-258) and the label prep of
``main_util.py`` (:209-225 extract_dynamic_from_fg, :253-265 mseg_label_RRV).

ONE execution path: ``RadarFlowLoss`` runs the fused HIP kernels behind ``cmf_radar_loss`` (csrc/loss.hip: all seven terms and
their gradients w.r.t. the network outputs in one call), ``make_labels`` runs ``cmf_pseudo_labels`` (csrc/eval.hip).  Like the
reference's loss (radar_loss.py:17-97) the call takes any cloud size: up to 704 points with the reference's 8 smoothness
neighbours (it trains at N = 256) a sample lives in one workgroup's LDS (3 launches); larger clouds and num_nb in {4, 16} take
the tiled kernels of the same file (the cloud streamed through LDS, a sample's lists in a workspace; 4 launches) -- same terms,
same per-point arithmetic.  On CPU tensors the call RAISES: there is no torch-op fallback in the product (the torch-op
restatement of the terms is a test fixture, tests/loss_torch.py).  Unlike the reference the loss items stay on the device (no 8
``.item()`` host syncs per step, radar_loss.py:156-159,285-288) until the caller asks.
"""
import ctypes

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib


def _make_labels(batch, vr_thres, n1, who):
    """cmf_pseudo_labels (n1 None) / cmf_pseudo_labels_counted (csrc/eval.hip) on device tensors -> dyn_mask, mseg_gt"""
    pc1 = batch["pc1"]
    if not pc1.is_cuda:
        raise RuntimeError("cmflow_amd.losses.%s runs on the GPU only (got %s tensors)" % (who, pc1.device))
    B, _, N = pc1.shape
    f32 = torch.float32
    c = lambda t: t.to(f32).contiguous()
    pc, T, vel, dt = c(pc1), c(batch["gt_trans"]), c(batch["ft1"][:, 0]), c(batch["interval"])
    fg, fl = c(batch["fg_mask"]), c(batch["flow_label"])
    dyn_mask, mseg_gt = torch.empty(B, N, dtype=f32, device=pc1.device), torch.empty(B, N, dtype=f32, device=pc1.device)
    p = lambda t: _lib.dev_ptr(t, f32)
    rest = (p(pc), p(T), p(vel), p(dt), p(fg), p(fl), vr_thres, p(dyn_mask), p(mseg_gt), None, _lib.stream_ptr())
    if n1 is None:
        _lib.check(_lib.lib().cmf_pseudo_labels(B, N, *rest), "cmf_pseudo_labels")
    else:
        _lib.check(_lib.lib().cmf_pseudo_labels_counted(B, N, _lib.dev_ptr(n1.contiguous(), torch.int32), *rest), "cmf_pseudo_labels_counted")
    return dyn_mask.to(batch["fg_mask"].dtype), mseg_gt


def make_labels(batch, vr_thres):
    """main_util.py:63-67: dyn_mask and the merged pseudo motion-segmentation label -- one launch of
    cmf_pseudo_labels (csrc/eval.hip) on device tensors."""
    return _make_labels(batch, vr_thres, None, "make_labels")


def make_labels_ragged(batch, vr_thres):
    """make_labels for a RAGGED batch (``dataset.as_batch_dict_ragged``: pc1 / ft1 (B,3,Nmax1), fg_mask (B,Nmax1), flow_label
    (B,Nmax1,3) padded, ``n1`` (B,) int32 on the device): one launch of cmf_pseudo_labels_counted.  Sample i's slices [:n1[i]] are
    bit-identical to make_labels on the truncated sample at B = 1 (the one reduction over a sample, the mean residual of
    main_util.py:260, runs over its valid points); padded slots of both outputs are 0."""
    pc1, n1 = batch["pc1"], batch["n1"]
    if n1.dtype != torch.int32 or n1.shape != (pc1.shape[0],) or n1.device != pc1.device:
        raise ValueError("make_labels_ragged: n1 is a (B,) int32 tensor on the inputs' device")
    return _make_labels(batch, vr_thres, n1, "make_labels_ragged")


MAX_N = 65536                                # include/cmflow_hip.h CMF_RADAR_LOSS_MAX_N
NUM_NB = (4, 8, 16)                          # csrc/loss.hip: the neighbour counts the kernels are instantiated for
ITEM_KEYS = ('Loss', 'smoothnessLoss', 'chamferLoss', 'veloLoss', 'egoLoss', 'maskLoss', 'opticalLoss', 'superviseLoss')


def _call_loss(ctx, d, name, size_name, sizes, outs, pred_f, pre_trans, mseg_pre, data, hyper):
    """Fills what RadarLossDesc and RadarLossCountedDesc share -- input pointers, weights, hyper-parameters, the gradient buffers
    (kept in ctx.grads), the workspace -- and calls ``name`` with ``size_name(*sizes, num_nb)`` floats of workspace (hyper["tiled"]:
    ``name + "_tiled"`` with ``name + "_workspace_tiled"``).  outs: descriptor field -> output tensor."""
    f32 = torch.float32
    t = {k: v.contiguous() for k, v in data.items()}
    pred_f = pred_f.contiguous()
    pre_trans = pre_trans.contiguous() if pre_trans is not None else None
    mseg_pre = mseg_pre.contiguous() if mseg_pre is not None else None
    for k, v in list(t.items()) + [("pred_f", pred_f), ("pre_trans", pre_trans), ("mseg_pre", mseg_pre)]:
        _lib.dev_ptr(v, torch.int32 if k in ("n1", "n2") else f32)       # device / dtype / density checks (no CPU fallback)
    d.self_only = int(hyper.get("self_only", False))
    d.pc1, d.pc2, d.pred_f, d.vel1 = t["pc1"].data_ptr(), t["pc2"].data_ptr(), pred_f.data_ptr(), t["vel1"].data_ptr()
    if not d.self_only:
        d.gt_f, d.mseg_pre, d.mseg_gt = t["gt_f"].data_ptr(), mseg_pre.data_ptr(), t["mseg_gt"].data_ptr()
        d.dyn_mask, d.radar_u, d.radar_v = t["dyn_mask"].data_ptr(), t["radar_u"].data_ptr(), t["radar_v"].data_ptr()
        d.opt, d.pre_trans, d.gt_trans = t["opt"].data_ptr(), pre_trans.data_ptr(), t["gt_trans"].data_ptr()
        d.camera_inverse, d.t_camera_radar = t["camera_inverse"].data_ptr(), t["t_camera_radar"].data_ptr()
        if "t_camera_radar_batch" in t:                      # a calibration per sample (dataset.augment_batch); else NULL: the shared one
            d.t_camera_radar_batch = t["t_camera_radar_batch"].data_ptr()
    d.w_self, d.w_em, d.w_ms, d.w_opt, d.w_dyn = hyper["w"]
    d.zeta, d.alpha, d.num_nb, d.lower_bound = hyper["zeta"], hyper["alpha"], hyper["num_nb"], hyper["lower_bound"]
    for field, out in outs.items():
        setattr(d, field, out.data_ptr())
    tiled = bool(hyper.get("tiled", False))                  # tests: the tiled kernels at a size the LDS kernel would take
    L = _lib.lib()
    size = getattr(L, name + "_workspace_tiled" if tiled else size_name)
    ws = torch.empty(size(*sizes, int(hyper["num_nb"])), dtype=f32, device=pred_f.device)
    d.workspace = ws.data_ptr()
    if any(ctx.needs_input_grad[:3]):
        g_f = torch.empty(pred_f.shape, dtype=f32, device=pred_f.device)
        g_t = torch.empty(pred_f.shape[0], 4, 4, dtype=f32, device=pred_f.device) if pre_trans is not None else None
        g_m = torch.empty(mseg_pre.shape, dtype=f32, device=pred_f.device) if mseg_pre is not None else None
        d.d_pred_f = g_f.data_ptr()
        d.d_pre_trans = g_t.data_ptr() if g_t is not None else None
        d.d_mseg_pre = g_m.data_ptr() if g_m is not None else None
        ctx.grads = (g_f, g_t, g_m)
    call = getattr(L, name + "_tiled" if tiled else name)
    _lib.check(call(ctypes.addressof(d), _lib.stream_ptr()), name)
    ctx.mark_non_differentiable(*outs.values())


class RadarFlowLossFn(Function):
    """total, items = cmf_radar_loss(...); the kernel writes d total / d (pred_f, pre_trans, mseg_pre) in the same
    pass, backward only scales them by the incoming gradient."""

    @staticmethod
    def forward(ctx, pred_f, pre_trans, mseg_pre, data, hyper):
        B, _, N = data["pc1"].shape
        items = torch.empty(9, dtype=torch.float32, device=data["pc1"].device)
        d = _lib.RadarLossDesc()
        d.B, d.N = B, N
        _call_loss(ctx, d, "cmf_radar_loss", "cmf_radar_loss_workspace_nb", (B, N), dict(items=items), pred_f, pre_trans, mseg_pre,
                   data, hyper)
        return items[0], items

    @staticmethod
    def backward(ctx, g_total, _g_items):
        g_f, g_t, g_m = ctx.grads
        need = ctx.needs_input_grad
        live = [i for i, (g, n) in enumerate(((g_f, need[0]), (g_t, need[1]), (g_m, need[2]))) if n and g is not None]
        # out of place (one launch for the three): the saved buffers stay what the kernel wrote, so a second backward through
        # the node (retain_graph=True) scales them by ITS incoming gradient, not by the product of both
        scaled = torch._foreach_mul([(g_f, g_t, g_m)[i] for i in live], g_total)
        out = [None, None, None]
        for i, g in zip(live, scaled):
            out[i] = g
        return out[0], out[1], out[2], None, None


class RadarFlowLossRaggedFn(Function):
    """mean total, mean items, per-sample items = cmf_radar_loss_counted(...) on a padded batch with per-sample counts; the kernel
    writes d (mean total) / d (pred_f, pre_trans, mseg_pre) in the same pass (padded slots 0), backward only scales them."""

    @staticmethod
    def forward(ctx, pred_f, pre_trans, mseg_pre, data, hyper):
        B, _, N1 = data["pc1"].shape
        N2 = data["pc2"].shape[2]
        per_sample = torch.empty(B, 9, dtype=torch.float32, device=data["pc1"].device)
        items = torch.empty(9, dtype=torch.float32, device=data["pc1"].device)
        n1, n2 = data["n1"].contiguous(), data["n2"].contiguous()
        d = _lib.RadarLossCountedDesc()
        d.B, d.N1max, d.N2max = B, N1, N2
        d.n1, d.n2 = n1.data_ptr(), n2.data_ptr()
        _call_loss(ctx, d, "cmf_radar_loss_counted", "cmf_radar_loss_counted_workspace", (B, N1, N2),
                   dict(items=per_sample, items_mean=items), pred_f, pre_trans, mseg_pre, data, hyper)
        return items[0], items, per_sample

    @staticmethod
    def backward(ctx, g_total, _g_items, _g_per_sample):
        return RadarFlowLossFn.backward(ctx, g_total, None)


SELF_ITEM_KEYS = ITEM_KEYS[:4]


class RadarFlowLoss(Module):
    """radar_loss.py:260-292 for model in {'cmflow','cmflow_t'}; weights (1,1,1,0.1,1) (:262); hyper-parameters of the terms as the
    reference constructs them (zeta = 0.005 :20, alpha = 0.5 / num_nb = 8 :63, lower_bound = 0.25 :210).
    Returns (total_loss, items) with items as 0-d device tensors (call .item() when needed)."""

    tiled = False                # tests: force the tiled kernels (cmf_radar_loss_tiled) at any size

    def __init__(self, camera_projection, t_camera_radar, w_self=1, w_em=1, w_ms=1, w_opt=0.1, w_dyn=1,
                 zeta=0.005, alpha=0.5, num_nb=8, lower_bound=0.25):
        super().__init__()
        self.w_self, self.w_em, self.w_ms, self.w_opt, self.w_dyn = w_self, w_em, w_ms, w_opt, w_dyn
        self.zeta, self.alpha, self.num_nb, self.lower_bound = zeta, alpha, num_nb, lower_bound
        self.register_buffer("camera_projection", torch.as_tensor(camera_projection, dtype=torch.float32))
        self.register_buffer("camera_inverse", torch.inverse(self.camera_projection[:3, :3].cpu()))
        self.register_buffer("t_camera_radar", torch.as_tensor(t_camera_radar, dtype=torch.float32))

    def _check(self, pc1):
        N = pc1.shape[2]
        if not pc1.is_cuda:
            raise RuntimeError("cmflow_amd.losses.RadarFlowLoss runs on the GPU only (got %s tensors)" % pc1.device)
        if self.num_nb not in NUM_NB or not (self.num_nb < N <= MAX_N):
            raise RuntimeError("cmf_radar_loss: num_nb in %s and num_nb < N <= %d points (got N = %d, num_nb = %d)"
                               % (NUM_NB, MAX_N, N, self.num_nb))

    def forward(self, pc1, pc2, pred_f, vel1, gt_f=None, pre_trans=None, mseg_pre=None, gt_trans=None, mseg_gt=None,
                dyn_mask=None, radar_u=None, radar_v=None, opt=None, t_camera_radar=None):
        """With only (pc1, pc2, pred_f, vel1) this is the loss of model 'raflow' (radar_loss.py:274-276): the three
        self-supervised terms; items then has the four keys of SelfSupervisedLoss (:153-158).
        ``t_camera_radar`` (B,4,4), optional: a radar-to-camera transform per sample -- the optical-flow term of sample i projects
        through row i instead of the module's shared matrix (an augmented batch's ``batch["t_camera_radar"]``).  None: the shared
        one, exactly as before."""
        self._check(pc1)
        data, hyper, keys = self._data_hyper(pc1, pc2, vel1, gt_f, gt_trans, mseg_gt, dyn_mask, radar_u, radar_v, opt, t_camera_radar)
        if gt_f is None:
            pre_trans = mseg_pre = None
        total, items = RadarFlowLossFn.apply(pred_f, pre_trans, mseg_pre, data, hyper)
        return total, {k: items[i + 1] for i, k in enumerate(keys)}

    def _data_hyper(self, pc1, pc2, vel1, gt_f, gt_trans, mseg_gt, dyn_mask, radar_u, radar_v, opt, t_camera_radar=None):
        """-> the Functions' data and hyper dictionaries and the keys of the reported items; without gt_f the self-only case (which
        has no camera term and ignores a per-sample calibration)"""
        if gt_f is None:
            return dict(pc1=pc1, pc2=pc2, vel1=vel1), dict(
                w=(self.w_self, 0.0, 0.0, 0.0, 0.0), zeta=self.zeta, alpha=self.alpha, num_nb=self.num_nb, lower_bound=0.0,
                self_only=True, tiled=self.tiled), SELF_ITEM_KEYS
        data = dict(pc1=pc1, pc2=pc2, gt_f=gt_f, vel1=vel1, gt_trans=gt_trans, mseg_gt=mseg_gt.to(pc1.dtype),
                    dyn_mask=dyn_mask.to(pc1.dtype), radar_u=radar_u, radar_v=radar_v, opt=opt,
                    camera_inverse=self.camera_inverse, t_camera_radar=self.t_camera_radar)
        if t_camera_radar is not None:
            if t_camera_radar.shape != (pc1.shape[0], 4, 4):
                raise ValueError("RadarFlowLoss: t_camera_radar is (B,4,4), one matrix per sample (got %s)" % (tuple(t_camera_radar.shape),))
            data["t_camera_radar_batch"] = t_camera_radar
        hyper = dict(w=(self.w_self, self.w_em, self.w_ms, self.w_opt, self.w_dyn), zeta=self.zeta, alpha=self.alpha,
                     num_nb=self.num_nb, lower_bound=self.lower_bound, tiled=self.tiled)
        return data, hyper, ITEM_KEYS

    # ---- ragged batches: whole frames of their own sizes (CMFlow.forward_ragged, dataset.collate_ragged) ----------------------------
    def _check_ragged(self, pc1, pc2, pred_f, npoints1, npoints2, validate):
        if pc1.dim() != 3 or pc2.dim() != 3 or pc1.shape[1] != 3 or pc2.shape[1] != 3 or pc2.shape[0] != pc1.shape[0] or \
                pred_f.shape != pc1.shape:
            raise ValueError("forward_ragged: pc1 / pred_f are (B,3,Nmax1), pc2 (B,3,Nmax2)")
        B, _, N1 = pc1.shape
        N2 = pc2.shape[2]
        for n in (npoints1, npoints2):
            if not torch.is_tensor(n) or n.dtype != torch.int32 or n.shape != (B,) or n.device != pc1.device:
                raise ValueError("forward_ragged: npoints1 / npoints2 are (B,) int32 tensors on the inputs' device")
        if self.num_nb not in NUM_NB or not (self.num_nb < N1 <= MAX_N) or not (1 <= N2 <= MAX_N):
            raise ValueError("cmf_radar_loss_counted: num_nb in %s, num_nb < Nmax1 <= %d and 1 <= Nmax2 <= %d (got Nmax1 = %d, "
                             "Nmax2 = %d, num_nb = %d)" % (NUM_NB, MAX_N, MAX_N, N1, N2, self.num_nb))
        if validate:                                                # a device -> host sync
            lo1, hi1, lo2, hi2 = (int(v) for v in torch.stack((npoints1.min(), npoints1.max(), npoints2.min(), npoints2.max())).tolist())
            if lo1 <= self.num_nb or hi1 > N1:
                raise ValueError("forward_ragged: npoints1 must lie in [%d, %d] (the smoothness term takes %d neighbours besides the "
                                 "point itself; the reference's top-k raises below that); got [%d, %d]"
                                 % (self.num_nb + 1, N1, self.num_nb, lo1, hi1))
            if lo2 < 1 or hi2 > N2:
                raise ValueError("forward_ragged: npoints2 must lie in [1, %d]; got [%d, %d]" % (N2, lo2, hi2))
        if not pc1.is_cuda:
            raise RuntimeError("cmflow_amd.losses.RadarFlowLoss runs on the GPU only (got %s tensors)" % pc1.device)

    def forward_ragged(self, pc1, pc2, pred_f, vel1, npoints1, npoints2, gt_f=None, pre_trans=None, mseg_pre=None, gt_trans=None,
                       mseg_gt=None, dyn_mask=None, radar_u=None, radar_v=None, opt=None, validate=False, t_camera_radar=None):
        """The loss of B whole frames of their own sizes in one call (cmf_radar_loss_counted).  pc1, pred_f, gt_f (B,3,Nmax1), pc2
        (B,3,Nmax2), per-point tensors of cloud 1 (B,Nmax1[,2]) padded; npoints1, npoints2 (B,) int32 on the device,
        num_nb < npoints1[i] <= Nmax1, 1 <= npoints2[i] <= Nmax2.
        -> (total, items, per_sample): per_sample (B,9) holds for sample i what ``forward`` returns at B = 1 on the truncated sample
        (column 0 the total, columns 1.. in the order of ITEM_KEYS); items / total are their means over the B samples (the
        reference's test protocol at batch size 1) -- NOT the dense batch loss, which pools the three masked terms over the batch.
        total is differentiable w.r.t. pred_f, pre_trans, mseg_pre; padded slots of the gradients are 0.  Padded input slots must
        be finite and influence nothing.  validate=True checks the counts on the host (ValueError; a device -> host sync), otherwise
        they are trusted: the kernels clamp them to [num_nb + 1, Nmax1] / [1, Nmax2], so a wrong count gives wrong numbers, not a
        wild access.  Without gt_f: the three self-supervised terms (model 'raflow'), as in ``forward``.  ``t_camera_radar`` (B,4,4):
        a calibration per sample, as in ``forward``."""
        self._check_ragged(pc1, pc2, pred_f, npoints1, npoints2, validate)
        data, hyper, keys = self._data_hyper(pc1, pc2, vel1, gt_f, gt_trans, mseg_gt, dyn_mask, radar_u, radar_v, opt, t_camera_radar)
        if gt_f is None:
            pre_trans = mseg_pre = None
        total, items, per_sample = RadarFlowLossRaggedFn.apply(pred_f, pre_trans, mseg_pre, dict(data, n1=npoints1, n2=npoints2), hyper)
        return total, {k: items[i + 1] for i, k in enumerate(keys)}, per_sample
