"""CPU: the host side of training on ragged batches (CMFlow.forward_ragged_train, TrainStep.step_ragged, cmf_ego_refine_grad_counted,
cmf_global_max_cat_grad_counted) -- signatures, the refusals that need no GPU, the C-ABI mirrors, and the ORACLE side of
tests/test_gpu_ragged_train.py: the per-sample eval-mode gradients whose mean that test compares against are finite and non-zero
wherever the dense golden reports a gradient."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ragged_loss_case as RC
import ragged_train_case as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cmf_ego_refine_grad_counted": 16, "cmf_global_max_cat_grad_counted": 10}


def test_header_and_ctypes_agree_on_the_new_entry_points():
    from cmflow_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "cmflow_hip.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert getattr(ctypes.CDLL(_lib.build()), name)
    # the counted forms take the dense argument lists plus the count pointer
    S, vp = _lib.SIGNATURES, ctypes.c_void_p
    assert S["cmf_ego_refine_grad_counted"] == S["cmf_ego_refine_grad"][:5] + [vp] + S["cmf_ego_refine_grad"][5:]
    assert S["cmf_global_max_cat_grad_counted"] == S["cmf_global_max_cat_grad"][:-1] + [vp, vp]


def test_signatures():
    from cmflow_amd.cmflow import CMFlow, CMFlow_T
    from cmflow_amd.raflow import RaFlow
    from cmflow_amd.train import TrainStep
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(CMFlow.forward_ragged_train) == ["self", "pc1", "pc2", "feature1", "feature2", "npoints1", "npoints2", "label_m", "validate"]
    assert names(CMFlow_T.forward_ragged_train) == ["self", "pc1", "pc2", "feature1", "feature2", "npoints1", "npoints2", "label_m", "gfeat",
                                                    "validate"]
    for f in (CMFlow.forward_ragged_train, CMFlow_T.forward_ragged_train):
        assert inspect.signature(f).parameters["validate"].default is False
    assert names(TrainStep.forward_loss_ragged)[:2] == ["self", "batch"] and names(TrainStep.step_ragged)[:2] == ["self", "batch"]
    assert names(CMFlow.forward_ragged) == ["self", "pc1", "pc2", "feature1", "feature2", "npoints1", "npoints2", "validate"]
    with pytest.raises(NotImplementedError):
        RaFlow.forward_ragged_train(None)


def test_refusals_that_need_no_gpu(args):
    from cmflow_amd.cmflow import CMFlow, CMFlow_T
    from cmflow_amd.train import TrainStep
    x = torch.zeros(2, 3, 16)
    n = torch.tensor([16, 16], dtype=torch.int32)
    for cls, extra in ((CMFlow, ()), (CMFlow_T, (None,))):
        net = cls(args)
        net.train()
        with pytest.raises(RuntimeError, match="eval"):
            net.forward_ragged_train(x, x, x, x, n, n, None, *extra)
        net.eval()
        with pytest.raises(ValueError):
            net.forward_ragged_train(x, x, x, x, n.long(), n, None, *extra)
        with pytest.raises(ValueError, match="npoints2"):
            net.forward_ragged_train(x, x, x, x, n, torch.tensor([16, 7], dtype=torch.int32), None, *extra, validate=True)
        with pytest.raises(ValueError, match="label_m"):
            net.forward_ragged_train(x, x, x, x, n, n, torch.zeros(2, 15), *extra)
        with pytest.raises(RuntimeError):                                 # autograd on, CPU tensors: no fallback behind the checks
            net.forward_ragged_train(x, x, x, x, n, n, None, *extra, validate=True)
        with pytest.raises(RuntimeError, match="no_grad"):                # forward_ragged keeps its own mode checks
            net.forward_ragged(x, x, x, x, n, n, *extra)
    net = CMFlow(args).train()
    with pytest.raises(RuntimeError, match="eval"):
        TrainStep(net).forward_loss_ragged({"pc1": x, "pc2": x, "ft1": x, "ft2": x, "n1": n, "n2": n})


@pytest.mark.parametrize("case", list(TC.CASES))
def test_oracle_per_sample_eval_mode_gradients_are_usable(case, golden_dir):
    """The precondition of the GPU comparison: on every truncated sample the oracle's eval-mode step is finite and gives a non-zero
    gradient in every tensor the dense eval-BN golden reports one for (and none where it reports none)."""
    counts, seed = TC.CASES[case]
    g = np.load(os.path.join(golden_dir, "cmflow_train_evalbn_synth_b4.npz"))
    has_grad = {str(k): float(v) >= 0 for k, v in zip(g["grad_names"], g["grad_norms"])}
    batch = RC.make_case(counts, seed)[0]
    sd = TC.weights()
    for i in range(len(counts)):
        grads, totals, items, outs = TC.oracle_mean_gradient(sd, {k: v[i:i + 1] for k, v in batch.items()}, counts[i:i + 1], torch.float32)
        assert np.isfinite(totals[0]) and all(np.isfinite(v) for v in items[0].values()), (i, totals, items)
        assert set(grads) == set(has_grad)
        for k, v in grads.items():
            if not has_grad[k]:
                assert v is None, (i, k)
                continue
            assert v is not None and torch.isfinite(v).all() and v.any(), (i, k)
    assert TC.bounds_for(case)[0][0] >= TC.DEFAULT_BOUNDS[0] and TC.bounds_for(case)[1][0] >= TC.WHOLE_GRADIENT_BOUND[0]
