"""References and fixtures of tests/test_gpu_grad_guard.py and tests/test_grad_guard_host.py (not a test): the exact sum of squares of
an fp32 vector, the clip coefficient of torch's ``clip_grad_norm_`` evaluated in fp32 from a float32 norm, the small module of
tests/test_gpu_model.py::test_flat_adam_matches_torch_adam (tensors that straddle the optimizer kernel's 1024-element chunks), and
the two-frame ragged batch of the whole-frame test."""
import math

import torch

SUMSQ_TOTALS = (1, 3, 255, 1024, 1025, 4 * 1024 + 3, 300001)      # below one float4 | one slab | past a vector / slab boundary | P > 1 and a tail
RANGE_TOTAL = 4099
RAGGED_COUNTS = ((256, 256), (33, 9))                              # (n1, n2) per frame; tests/ragged_loss_case.py's largest and smallest
RAGGED_SEED = 3                                                    # both motion-seg classes and a dynamic point in either frame (host test)
LAST_PT_KEYS = {"format", "version", "settings", "epoch", "model", "optimizer", "scheduler", "training", "history"}
SETTINGS_KEYS = {"model", "batch_size", "val_batch_size", "num_points", "seed", "lr", "decay_epochs", "decay_rate", "mini_clip_len",
                 "vr_thres", "world", "train_frames", "val_frames"}
HISTORY_KEYS = {"train_loss", "loss_items", "val_score", "lr", "best"}
GUARD_KEYS = ("grad_norm_mean", "grad_norm_max", "clipped_steps", "skipped_steps")


def exact_sumsq(x):
    """sum x_i^2 of a float32 CPU tensor, correctly rounded to double: the square of an fp32 value is exact in float64, and
    math.fsum adds without intermediate rounding."""
    assert x.dtype == torch.float32 and not x.is_cuda
    return math.fsum((x.double() * x.double()).tolist())


def sumsq_bound(total):
    """Relative error allowed to a double accumulation of `total` exact non-negative terms in ANY order: gamma_(n-1) =
    (n-1) u / (1 - (n-1) u) with u = 2^-53 -- taken with a factor 2 of margin as total * 2^-52."""
    return total * 2.0 ** -52


def wide_range_values(total, seed):
    """Seeded normals scaled by 10^U(-15, 15): 30 decades, squares from 1e-30 to 1e30 and beyond."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(total, generator=g, dtype=torch.float64)
            * 10.0 ** (torch.rand(total, generator=g, dtype=torch.float64) * 30.0 - 15.0)).float()


def clip_scale(normf, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient, clamped to 1, in fp32 from a float32 norm -> a Python float (exactly an fp32)."""
    coef = torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(normf, dtype=torch.float32) + torch.tensor(1e-6, dtype=torch.float32))
    return float(torch.clamp(coef, max=1.0))


def small_module(dev):
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(37, 129, bias=False), torch.nn.BatchNorm1d(129), torch.nn.ReLU(),
                               torch.nn.Linear(129, 5)).to(dev)


def ragged_batch():
    """The padded two-frame batch (CPU) with its n1 / n2."""
    import ragged_loss_case as RC
    import ragged_train_case as TC
    return TC.padded(RC.make_case(RAGGED_COUNTS, RAGGED_SEED)[0], RAGGED_COUNTS, 300, 256)
