"""Data parallelism for the training step: one process per GPU, one RCCL all-reduce per step.

The reference's only multi-GPU mode is single-process ``nn.DataParallel``
(models/model.py:40-42): per step it broadcasts all parameters, scatters the batch, gathers
outputs to GPU 0 and reduces gradients there; BatchNorm statistics are per replica.  The
MI355X-native equivalent keeps the same semantics (per-rank BN statistics, mean gradient)
with ``torch.distributed`` (backend "nccl" = RCCL over xGMI): gradients of all parameters are
views into ONE flat fp32 bucket (16.9 MB for CMFlow, 18.5 MB for CMFlow-T), reduced with a
single ``all_reduce(SUM)`` per optimizer step and scaled by 1/world.  Nothing is exchanged in
the forward pass.  Parameters that never receive a gradient (the 12 unused WeightNet-BN
tensors) stay outside the bucket with grad=None, so Adam skips them as it does in the reference.
"""
import contextlib
import math

import torch
import torch.distributed as dist


class FlatGradBucket:
    def __init__(self, module: torch.nn.Module):
        allp = list(module.parameters())
        keep = [i for i, p in enumerate(allp) if p.requires_grad and not getattr(p, '_cmf_unused', False)]
        self.params = [allp[i] for i in keep]
        # position of every bucket parameter in module.parameters() order, and that list's length: an optimizer checkpoint saved over
        # ALL parameters of the module (the reference's torch.optim.Adam(net.parameters()), main.py:107) is indexed that way
        self.module_index, self.module_params = keep, len(allp)
        n = sum(p.numel() for p in self.params)
        p0 = self.params[0]
        self.flat = torch.zeros(n, dtype=p0.dtype, device=p0.device)
        off = 0
        self.views = []
        for p in self.params:
            k = p.numel()
            p.grad = self.flat[off:off + k].view_as(p)        # gradients accumulate in place into the bucket
            self.views.append(p.grad)
            off += k
        self.numel = n
        for p in self.params:                                 # = fused_blocks.enable_grad_sinks: the backward kernels
            p._cmf_sink = True                                # accumulate straight into the bucket

    def zero(self):
        """optimizer.zero_grad() equivalent that keeps the views (set_to_none would break them).  The check is an
        identity comparison per parameter (this runs on the host between forward and backward, every step)."""
        self.flat.zero_()
        for p, v in zip(self.params, self.views):
            if p.grad is not v:
                raise RuntimeError("a gradient left the flat bucket (zero_grad(set_to_none=True)?)")

    def all_reduce_mean(self, group=None, force=False):
        if dist.is_available() and dist.is_initialized() and (force or dist.get_world_size(group) > 1):
            if dist.get_backend(group) == "nccl":
                # RCCL averages inside the collective (ncclAvg, as SegmentedReducer does): no scaling kernel behind it
                dist.all_reduce(self.flat, op=dist.ReduceOp.AVG, group=group)
            else:                                             # gloo (CPU tests, the one-GPU two-rank tests) has no AVG
                dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
                self.flat.mul_(1.0 / dist.get_world_size(group))

    # ---- segments: all-reduce overlapped with the backward pass ---------------------------------------------------
    def segment_of(self, modules):
        """(offset, length) of the contiguous stretch of the bucket that holds the parameters of `modules` (they must be
        adjacent in module.parameters() order, which is how the bucket is laid out)."""
        ids = {id(p) for m in modules for p in m.parameters()}
        off, lo, hi = 0, None, None
        for p in self.params:
            if id(p) in ids:
                lo = off if lo is None else lo
                if hi is not None and hi != off:
                    raise ValueError("parameters of the given modules are not contiguous in the bucket")
                hi = off + p.numel()
            off += p.numel()
        if lo is None:
            raise ValueError("no bucket parameter belongs to the given modules")
        return lo, hi - lo


def guard_options(max_grad_norm=None, skip_nonfinite=False):
    """The two options of the guarded optimizer step, checked: -> (max_grad_norm as a float or None, skip_nonfinite as a bool).
    ``max_grad_norm`` is a positive finite number or None (no clipping); 0, a negative number, NaN and inf raise ValueError -- a
    clip that can never act, or that zeroes every step, is a mistake and not a setting."""
    if max_grad_norm is not None:
        if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)):
            raise ValueError("max_grad_norm must be a positive finite number or None, not %r" % (max_grad_norm,))
        max_grad_norm = float(max_grad_norm)
        if not (math.isfinite(max_grad_norm) and max_grad_norm > 0.0):
            raise ValueError("max_grad_norm must be a positive finite number or None, not %r" % (max_grad_norm,))
    return max_grad_norm, bool(skip_nonfinite)


def ema_options(ema_decay=None):
    """The decay of the averaged weights, checked: -> a float in the open interval (0, 1), or None (off).  A bool, 0, 1, a negative
    number, NaN and inf raise ValueError: a decay of 0 is the live weights, a decay of 1 never moves, neither is an average."""
    if ema_decay is None:
        return None
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 < float(ema_decay) < 1.0:
        raise ValueError("ema_decay must be a number in the open interval (0, 1) or None, not %r" % (ema_decay,))
    return float(ema_decay)


def grad_norm(bucket):
    """The L2 norm of the bucket's gradient as a 0-d float64 device tensor: cmf_grad_norm, two launches on the current stream, no
    host read.  The sum of squares is accumulated in double over a partition that depends on the bucket's size alone, in a fixed
    order (relative error <= numel * 2^-53, bit-reproducible); a NaN or +-Inf gradient gives a non-finite norm.  The value a
    guarded FlatAdam step on the same bucket decides by is ``float32(grad_norm(bucket))``."""
    from . import _lib
    flat = bucket.flat
    parts = _lib.lib().cmf_grad_norm_parts(bucket.numel)
    partials = torch.empty(parts, dtype=torch.float64, device=flat.device)
    out = torch.empty(2, dtype=torch.float64, device=flat.device)
    _lib.check(_lib.lib().cmf_grad_norm(bucket.numel, _lib.dev_ptr(flat, torch.float32), partials.data_ptr(), out.data_ptr(),
                                        _lib.stream_ptr()), "cmf_grad_norm")
    return out[1]


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.Adam (L2 weight decay, no amsgrad: the reference's optimizer, main.py:107) over a FlatGradBucket as ONE kernel
    launch (cmf_adam_step): the gradients already lie contiguously in the bucket, the moments are two flat arrays in the same order, and
    the parameters stay where the module holds them (a device table of their addresses).  torch's fused Adam needs six multi-tensor
    launches for the model's 182 tensors at the very end of a step.  A torch Optimizer all the same: lr schedulers act on
    param_groups[0]['lr'] (the reference steps a StepLR per epoch, main.py:108,151).

    The guard (off by default: ``step()`` is then the one cmf_adam_step launch).  ``max_grad_norm`` clips by the L2 norm of the whole
    bucket with torch's ``clip_grad_norm_`` formula, ``skip_nonfinite`` leaves parameters and both moment arrays untouched when that
    norm is NaN or Inf.  With either on, ``step()`` is cmf_grad_sumsq followed by cmf_adam_step_guarded (include/cmflow_hip.h has the
    formula): the decision is taken on the device, the host reads nothing.  The bucket itself is NOT scaled -- it is zeroed before
    the next backward anyway -- so ``p.grad`` read after a clipped step holds the unclipped gradient.  ``steps`` counts calls: a
    skipped call advances the bias corrections like any other.  ``record`` (8 float64 on the device, see ``guard_stats``) counts
    what the guard did.  Not guarded: BatchNorm's running statistics, which a train-mode forward has already updated.

    Averaged weights (off by default: ``ema_decay=None`` launches what it launched before).  With a decay d in (0, 1), ``ema`` is a
    flat fp32 array in bucket order, set to the parameters at construction (so there is no debiasing), and ``step()`` calls
    cmf_adam_step_ema / cmf_adam_step_guarded_ema: the same launch also does ``ema += float32(1 - d) * (p_new - ema)`` in one fma
    (include/cmflow_hip.h has the formula and why this form).  Parameters and moments get the bits they get without it; a step the
    guard skips leaves ``ema`` untouched as well.  ``ema_weights()`` runs the module on the average, ``ema_state_dict(module)`` is
    the state dict to save.  BatchNorm's buffers are not averaged: the averaged parameters run with the live running statistics."""

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False,
                 ema_decay=None):
        self.max_grad_norm, self.skip_nonfinite = guard_options(max_grad_norm, skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self.ema_decay = ema_options(ema_decay)
        if self.ema_decay is not None and not bucket.flat.is_cuda:
            raise ValueError("FlatAdam: ema_decay needs the GPU optimizer; the model is on the CPU")
        super().__init__(bucket.params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) != 1:
            raise ValueError("FlatAdam: one parameter group (the bucket's parameters) -- per-group options are not supported")
        self.bucket = bucket
        self.exp_avg = torch.zeros_like(bucket.flat)
        self.exp_avg_sq = torch.zeros_like(bucket.flat)
        self.steps = 0
        self._ptrs = None
        self._tables()
        if self.guarded:
            from . import _lib
            parts = _lib.lib().cmf_grad_norm_parts(bucket.numel)
            self._partials = torch.zeros(parts, dtype=torch.float64, device=bucket.flat.device)
            self.record = torch.zeros(8, dtype=torch.float64, device=bucket.flat.device)
        self._exchanged = False
        if self.ema_decay is not None:
            self.ema = torch.empty_like(bucket.flat)
            self._ema_from_params()

    def _ema_from_params(self):
        """ema <- the parameters as they are now, slice by slice at the table's offsets."""
        off = 0
        with torch.no_grad():
            for p in self.bucket.params:
                n = p.numel()
                self.ema[off:off + n].copy_(p.detach().reshape(-1))
                off += n

    def _need_ema(self, what):
        if self.ema_decay is None:
            raise RuntimeError("FlatAdam.%s: the averaged weights are off (ema_decay=None)" % what)

    def _exchange(self):
        from . import _lib
        b = self.bucket
        self._tables()
        _lib.check(_lib.lib().cmf_param_exchange(len(b.params), self._offs.data_ptr(), self._pt.data_ptr(), b.numel, self.ema.data_ptr(),
                                                 _lib.stream_ptr()), "cmf_param_exchange")
        bump = getattr(torch.autograd.graph, "increment_version", None)      # a raw-pointer write to the parameters, as in step()
        if bump is not None:
            bump(b.params)

    @contextlib.contextmanager
    def ema_weights(self):
        """Context manager: inside it the module computes with the averaged parameters.  One cmf_param_exchange launch on entry swaps
        every parameter element with its ``ema`` element (``self.ema`` then holds the live parameters), one on exit -- in a
        ``finally``, so also when the body raises -- swaps them back; pure copies, so everything is restored bit for bit.  Both
        exchanges bump the parameters' autograd version counters as ``step()`` does.  Nested use and ``step()`` inside raise
        RuntimeError.  BatchNorm's buffers are NOT averaged: the averaged parameters run with the live running statistics."""
        self._need_ema("ema_weights")
        if self._exchanged:
            raise RuntimeError("FlatAdam.ema_weights: already inside ema_weights() (the parameters hold the averaged weights)")
        self._exchange()
        self._exchanged = True
        try:
            yield self
        finally:
            self._exchange()
            self._exchanged = False

    def ema_state_dict(self, module):
        """``module.state_dict()`` with every bucket parameter replaced by a clone of its slice of ``ema``: the averaged model in the
        module's own format (buffers and parameters outside the bucket are the live ones).  Slicing only: no exchange, no launch of
        the library.  Raises inside ``ema_weights()``, where ``ema`` holds the live parameters."""
        self._need_ema("ema_state_dict")
        if self._exchanged:
            raise RuntimeError("FlatAdam.ema_state_dict: inside ema_weights() self.ema holds the live parameters")
        sd = module.state_dict()
        slot = {}
        off = 0
        for p in self.bucket.params:
            slot[id(p)] = (off, p)
            off += p.numel()
        found = 0
        for name, p in module.named_parameters(remove_duplicate=False):
            if id(p) in slot and name in sd:
                o, q = slot[id(p)]
                sd[name] = self.ema[o:o + q.numel()].view_as(q).clone()
                found += 1
        if found < len(slot):
            raise ValueError("FlatAdam.ema_state_dict: the module's state dict holds %d of the bucket's %d parameters" % (found, len(slot)))
        return sd

    def guard_stats(self, reset=False):
        """A copy of the guard's record, a float64 device tensor (no host read): [0] step() calls, [1] calls with a non-finite norm,
        [2] clipped calls, [3] the sum and [4] the maximum of the float32 norm over the finite calls, [5] the last sum of squares,
        [6] the last norm, [7] the last scale.  ``reset=True`` zeroes the record on the device behind the copy."""
        if not self.guarded:
            raise RuntimeError("FlatAdam.guard_stats: the guard is off (max_grad_norm=None, skip_nonfinite=False)")
        out = self.record.clone()
        if reset:
            self.record.zero_()
        return out

    def _tables(self):
        ps = self.bucket.params
        ptrs = tuple(p.data_ptr() for p in ps)
        if ptrs == self._ptrs:
            return
        for p in ps:
            if not (p.is_contiguous() and p.dtype == torch.float32 and p.is_cuda):
                raise RuntimeError("FlatAdam: parameters must be contiguous fp32 device tensors")
        offs, o = [], 0
        for p in ps:
            offs.append(o)
            o += p.numel()
        offs.append(o)
        dev = self.bucket.flat.device
        self._offs = torch.tensor(offs, dtype=torch.int64, device=dev)
        self._pt = torch.tensor(ptrs, dtype=torch.int64, device=dev)
        self._ptrs = ptrs

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib
        if self._exchanged:
            raise RuntimeError("FlatAdam.step: inside ema_weights() the parameters hold the averaged weights")
        loss = closure() if closure is not None else None
        b = self.bucket
        for p, v in zip(b.params, b.views):
            if p.grad is not v:
                raise RuntimeError("a gradient left the flat bucket (zero_grad(set_to_none=True)?)")
        self._tables()                                       # a parameter whose storage was replaced gets its new address
        if len(self.param_groups) != 1:
            raise RuntimeError("FlatAdam: add_param_group is not supported (one group: the bucket's parameters)")
        g = self.param_groups[0]
        self.steps += 1
        hyper = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), self.steps)
        averaged = self.ema_decay is not None
        if self.guarded:
            stream = _lib.stream_ptr()
            _lib.check(_lib.lib().cmf_grad_sumsq(b.numel, b.flat.data_ptr(), self._partials.data_ptr(), stream), "cmf_grad_sumsq")
            args = (len(b.params), self._offs.data_ptr(), self._pt.data_ptr(), b.numel, b.flat.data_ptr(), self.exp_avg.data_ptr(),
                    self.exp_avg_sq.data_ptr(), *hyper, self.max_grad_norm or 0.0, int(self.skip_nonfinite), self._partials.data_ptr(),
                    self.record.data_ptr())
            if averaged:
                _lib.check(_lib.lib().cmf_adam_step_guarded_ema(*args, self.ema.data_ptr(), self.ema_decay, stream),
                           "cmf_adam_step_guarded_ema")
            else:
                _lib.check(_lib.lib().cmf_adam_step_guarded(*args, stream), "cmf_adam_step_guarded")
        elif averaged:
            _lib.check(_lib.lib().cmf_adam_step_ema(len(b.params), self._offs.data_ptr(), self._pt.data_ptr(), b.numel, b.flat.data_ptr(),
                                                    self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), *hyper, self.ema.data_ptr(),
                                                    self.ema_decay, _lib.stream_ptr()), "cmf_adam_step_ema")
        else:
            _lib.check(_lib.lib().cmf_adam_step(len(b.params), self._offs.data_ptr(), self._pt.data_ptr(), b.numel, b.flat.data_ptr(),
                                                self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), *hyper, _lib.stream_ptr()),
                       "cmf_adam_step")
        # the kernel writes the parameters through raw pointers: bump their autograd version counters like an in-place torch op would,
        # so that a backward pass through a graph recorded BEFORE this step raises instead of silently using the updated weights
        bump = getattr(torch.autograd.graph, "increment_version", None)
        if bump is not None:
            bump(b.params)
        return loss

    def zero_grad(self, set_to_none=False):
        self.bucket.zero()

    def state_dict(self):
        d = super().state_dict()
        d["flat"] = dict(exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, steps=self.steps)
        if self.guarded:
            d["flat"]["guard"] = self.record
        if self.ema_decay is not None:
            if self._exchanged:
                raise RuntimeError("FlatAdam.state_dict: inside ema_weights() self.ema holds the live parameters")
            d["flat"]["ema"] = self.ema
        return d

    def load_state_dict(self, d):
        """Accepts this class's own format (`flat`) and a torch.optim.Adam checkpoint -- per-parameter `state` with exp_avg /
        exp_avg_sq / step -- saved over the bucket's parameters in bucket order (what the previous TrainStep saved) OR over all of
        the module's parameters (the reference's `torch.optim.Adam(net.parameters())`, main.py:107, or an oracle / CPU run): its
        indices are then positions in module.parameters(); the parameters outside the bucket (never used, frozen) have no state in
        such a checkpoint either and are skipped.  The moments are scattered into the flat arrays.  Anything else raises:
        restarting the moments silently would change the training run.  A guarded optimizer restores its record from
        ``flat["guard"]`` and zeroes it for a checkpoint without one (the counters are diagnostics, not state of the run).
        Averaged weights: with ``ema_decay`` set, ``flat["ema"]`` is restored; a checkpoint without it (any of the formats above)
        re-initialises ``ema`` from the parameters as they are at load time -- load the model first; averaging starts from here (the
        fine-tuning case).  With ``ema_decay=None`` a stored ``ema`` is ignored."""
        if self._exchanged:
            raise RuntimeError("FlatAdam.load_state_dict: inside ema_weights() the parameters hold the averaged weights")
        d = dict(d)
        flat = d.pop("flat", None)
        per_param = d.get("state") or {}
        ps = self.bucket.params
        groups = d.get("param_groups")
        if groups is None or len(groups) != 1:
            raise ValueError("FlatAdam: the checkpoint has %s parameter groups, one is supported" % (len(groups) if groups is not None else "no"))
        saved = list(groups[0]["params"])
        if len(saved) == len(ps):
            key_of = list(saved)                              # bucket order
        elif len(saved) == self.bucket.module_params:
            key_of = [saved[i] for i in self.bucket.module_index]
            extra = set(per_param.keys()) - set(key_of)
            if extra:
                raise ValueError("FlatAdam: the checkpoint holds optimizer state for %d parameters outside the gradient bucket" % len(extra))
        else:
            raise ValueError("FlatAdam: the checkpoint covers %d parameters; the bucket holds %d of the module's %d"
                             % (len(saved), len(ps), self.bucket.module_params))
        group = dict(groups[0], params=list(range(len(ps))))
        super().load_state_dict(dict(d, state={}, param_groups=[group]))
        if self.ema_decay is not None:
            if flat is not None and "ema" in flat:
                self.ema.copy_(flat["ema"])
            else:
                self._ema_from_params()
        if flat is not None:
            self.exp_avg.copy_(flat["exp_avg"]); self.exp_avg_sq.copy_(flat["exp_avg_sq"]); self.steps = int(flat["steps"])
            if self.guarded and "guard" in flat:
                self.record.copy_(flat["guard"])
            elif self.guarded:
                self.record.zero_()
            return
        if not per_param:
            return                                           # a fresh optimizer's checkpoint: nothing to restore
        if not all(k in per_param for k in key_of):
            raise ValueError("FlatAdam: the checkpoint's per-parameter state does not cover the bucket's %d parameters" % len(ps))
        steps = set()
        off = 0
        for i, p in enumerate(ps):
            st = per_param[key_of[i]]
            n = p.numel()
            if st["exp_avg"].numel() != n:
                raise ValueError("FlatAdam: state %d has %d elements, the parameter %d" % (i, st["exp_avg"].numel(), n))
            self.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1)); self.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(st["step"]))
            off += n
        if len(steps) != 1:
            raise ValueError("FlatAdam: the checkpoint's parameters are at different step counts %s" % sorted(steps))
        self.steps = steps.pop()


class SegmentedReducer:
    """The gradient all-reduce of a step, cut into segments that are launched as soon as their part of the backward pass
    has been enqueued -- the counterpart of nn.DataParallel's reduction running inside backward (models/model.py:40-42).

    segments: [(offset, length)] in the order their gradients become complete.  launch(i) is called from a tensor hook on
    the autograd thread (after the chains that write the segment have been joined into the current stream); the
    collective runs on the backend's own stream behind an event of the current stream, so it overlaps the rest of the
    backward pass.  finish() makes the current stream wait for every launched segment, reduces the ones that were never
    launched (hooks that did not fire) and applies the 1/world mean.  RCCL: one ncclAvg all-reduce per segment (no scaling
    kernel); gloo (CPU tests, the 1-GPU two-rank tests): SUM followed by a multiply."""

    def __init__(self, bucket, segments, group=None):
        self.bucket, self.segments, self.group = bucket, list(segments), group
        covered = sorted(self.segments)
        pos = 0
        for off, n in covered:
            if off != pos:
                raise ValueError("segments must tile the bucket")
            pos = off + n
        if pos != bucket.numel:
            raise ValueError("segments must tile the bucket")
        self.views = [bucket.flat[off:off + n] for off, n in self.segments]
        self.work = [None] * len(self.segments)
        self.active = False
        self.early = 0

    def begin(self, force=False):
        """Arm the reducer for one backward pass; False when there is nothing to reduce (single rank, not forced)."""
        self.active = dist.is_available() and dist.is_initialized() and (force or dist.get_world_size(self.group) > 1)
        self.work = [None] * len(self.segments)
        if self.active:
            self.avg = dist.get_backend(self.group) == "nccl"
        return self.active

    def launch(self, i):
        if not self.active or self.work[i] is not None:
            return
        op = dist.ReduceOp.AVG if self.avg else dist.ReduceOp.SUM
        self.work[i] = dist.all_reduce(self.views[i], op=op, group=self.group, async_op=True)

    def finish(self):
        if not self.active:
            return
        self.early = sum(w is not None for w in self.work)      # segments launched from inside backward (diagnostics / tests)
        for i in range(len(self.segments)):
            self.launch(i)
        for w in self.work:
            w.wait()                                    # the current stream waits; the host does not block (NCCL semantics)
        if not self.avg:
            self.bucket.flat.mul_(1.0 / dist.get_world_size(self.group))
        self.active = False


def _gpu_local_cpus(index):
    """Host CPUs local to GPU `index` (its PCI device's NUMA node): /sys/bus/pci/devices/<domain:bus:device.0>/local_cpulist,
    or None when the property or the file is missing."""
    import os
    try:
        pr = torch.cuda.get_device_properties(index)
        bdf = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
        with open(os.path.join("/sys/bus/pci/devices", bdf, "local_cpulist")) as f:
            text = f.read().strip()
    except Exception:
        return None
    cpus = []
    for part in text.split(","):
        if part:
            lo, _, hi = part.partition("-")
            cpus.extend(range(int(lo), int(hi or lo) + 1))
    return cpus or None


def pin_rank_to_cores(local_rank=None, local_world=None):
    """OPT-IN (CMF_PIN_CORES=1; unmeasured -- no multi-GPU box so far): restrict this rank (and every thread it creates later:
    the library's chain workers, the autograd thread) to host cores of ITS GPU's NUMA node.  The cores local to the GPU come
    from sysfs (logical CPU ids are not laid out socket by socket: on SMT hosts the second half of the ids are the siblings of
    the first); the ranks whose GPUs share a node split that node's cores evenly, in local-rank order.  local_world is the
    number of ranks on THIS host (LOCAL_WORLD_SIZE), not the job's world size.  Returns the core list or None (not enabled,
    no locality information, or fewer than two cores per rank: the scheduler is left alone)."""
    import os
    if os.environ.get("CMF_PIN_CORES") != "1" or not hasattr(os, "sched_setaffinity"):
        return None
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if local_rank is None else local_rank
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "1")) if local_world is None else local_world
    if local_world <= 1:
        return None
    avail = set(os.sched_getaffinity(0))
    mine = _gpu_local_cpus(local_rank)
    if not mine:
        return None
    key = tuple(mine)
    sharing = [r for r in range(local_world) if tuple(_gpu_local_cpus(r) or ()) == key]     # ranks whose GPUs hang off the same node
    cores = sorted(c for c in mine if c in avail)
    per = len(cores) // max(len(sharing), 1)
    if per < 2 or local_rank not in sharing:
        return None
    i = sharing.index(local_rank)
    cores = cores[i * per:(i + 1) * per]
    os.sched_setaffinity(0, cores)
    return cores


def broadcast_module(module: torch.nn.Module, src=0, group=None):
    """One-time parameter/buffer broadcast from rank `src` (replicas start identical)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    for t in list(module.parameters()) + list(module.buffers()):
        dist.broadcast(t.data, src=src, group=group)


def shard_batch(batch: dict, rank: int, world: int) -> dict:
    """Rank r's contiguous slice of a global batch (dim 0), as DataParallel's scatter does."""
    out = {}
    for k, v in batch.items():
        B = v.shape[0]
        assert B % world == 0, "global batch must divide evenly over ranks"
        per = B // world
        out[k] = v[rank * per:(rank + 1) * per].contiguous()
    return out
