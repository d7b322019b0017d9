"""Mixup, CutMix and label smoothing for fine-tuning on the HIP path (TRAIN.MIXUP / CUTMIX / LABEL_SMOOTHING; additions of this
build -- the reference trains on plain batches with nn.CrossEntropyLoss).

  mix_volumes            every sample of a [B, C, S, S, S] fp32 batch mixed with its partner B - 1 - b in place, one launch
                         (hct_mix_volumes: one read and one write per voxel, only the boxes' voxels for CutMix)
  rand_box3d             timm's rand_bbox in three dimensions
  Mixup                  timm's Mixup (modes 'batch' and 'elem'): draws on the host from a numpy Generator, mixes on the device
  mix_multilabel_targets the mixed [B, T] label table of multi-label mode (a torch composition on a table of a few hundred entries)
  MixedCriterion         what main_downstream.py hands the engine when the recipe is on: the plain loss for validation and test,
                         `mix` + `train_loss` for training

The loss of the mixed batch is `classifier.soft_cross_entropy` (hct_mix_xent): the soft target is never built.  The draws are not
timm's random stream (as `DeviceAugment` does not reproduce MONAI's): per decision -- one per batch in mode 'batch', one per
sample in index order in mode 'elem' -- the Generator gives, in this order, `random()` against `prob`; if that fired and both
alphas are positive, `random()` against `switch_prob`; `beta(alpha, alpha)`; and for CutMix the three box centres of `rand_box3d`.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .classifier import bce_with_logits, cross_entropy, soft_cross_entropy


def mix_volumes(x: torch.Tensor, lam: torch.Tensor, box: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x fp32 [B, C, S, S, S] on the GPU, mixed in place and returned (hct_mix_volumes): sample b with a box (box[b] = lo0, hi0,
    lo1, hi1, lo2, hi2, half-open, non-empty on every axis) takes its partner's voxels x[B - 1 - b] inside the box; any other
    sample becomes lam[b] * x[b] + (1 - lam[b]) * x[B - 1 - b].  Both members of a pair read the values from before the call.
    lam / box given on the CPU are checked (lam in [0, 1], bounds in [0, S]) and uploaded; on the device they are taken as they
    are and the kernel clamps the bounds."""
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.HctError("mix_volumes runs on the GPU (libheadct_hip); no CPU fallback exists")
    if x.dtype != torch.float32 or x.dim() != 5 or not x.is_contiguous() or not (x.shape[2] == x.shape[3] == x.shape[4]):
        raise ValueError(f"x must be a contiguous fp32 [B, C, S, S, S] tensor, not {x.dtype} {tuple(x.shape)}")
    B, C, S = x.shape[0], x.shape[1], x.shape[2]
    if lam.numel() != B or (box is not None and tuple(box.shape) != (B, 6)):
        raise ValueError(f"lam needs {B} entries and box the shape ({B}, 6)")
    if not lam.is_cuda and B and not bool(((lam >= 0) & (lam <= 1)).all()):
        raise ValueError(f"lam must lie in [0, 1]: {lam.tolist()}")
    if box is not None and not box.is_cuda and B and (int(box.min()) < 0 or int(box.max()) > S):
        raise ValueError(f"box bounds must lie in [0, {S}]: {box.tolist()}")
    on = lambda t, dt: None if t is None else t.to(device=x.device, dtype=dt).contiguous()
    lam, box = on(lam, torch.float32), on(box, torch.int32)
    with torch.cuda.device(x.device):
        _lib.check(lib.hct_mix_volumes(x.data_ptr(), B, C, S, lam.data_ptr(), _lib.ptr(box), _lib.stream_ptr()), "hct_mix_volumes")
    return x


def rand_box3d(S: int, lam: float, rng: np.random.Generator) -> Tuple[Tuple[int, int, int, int, int, int], float]:
    """timm's rand_bbox in three dimensions: a cube of side int(S * (1 - lam) ** (1/3)) around a centre drawn per axis with
    rng.integers(0, S) (axis 0 first), cut off at the volume's faces.  Returns ((lo0, hi0, lo1, hi1, lo2, hi2), lam corrected to
    the share of the volume the box leaves: 1 - volume / S**3)."""
    cut = int(S * (1.0 - lam) ** (1.0 / 3.0))
    box, volume = [], 1
    for _ in range(3):
        c = int(rng.integers(0, S))
        lo, hi = max(c - cut // 2, 0), min(c + cut // 2, S)
        box += [lo, hi]
        volume *= hi - lo
    return tuple(box), 1.0 - volume / float(S) ** 3


class Mixup:
    """timm's Mixup for volumes: mixup when `mixup_alpha` > 0, CutMix when `cutmix_alpha` > 0, one of the two per decision with
    probability `switch_prob` for CutMix when both are; lam ~ Beta(alpha, alpha); with probability 1 - `prob` nothing is mixed
    (lam = 1).  Mode 'batch' takes one decision, one lam and one box for the whole batch, 'elem' one of each per sample.  Sample
    b is mixed with sample B - 1 - b.  The draws come from numpy.random.default_rng(seed) on the host (module docstring).

    `draw(B, S)` returns the CPU tables (lam for the voxels fp32 [B], box int32 [B, 6] or None, lam for the targets fp32 [B]) and
    keeps them in `last_draw`; a CutMix sample has voxel lam 1 (an empty box mixes nothing) and the corrected target lam.
    `__call__(x)` draws, mixes `x` in place (one launch; none when nothing fired) and returns the target lam on x's device."""

    def __init__(self, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0, switch_prob: float = 0.5, mode: str = "batch",
                 seed: int = 0):
        if not (mixup_alpha >= 0.0 and cutmix_alpha >= 0.0):
            raise ValueError(f"mixup_alpha and cutmix_alpha must be >= 0: got {mixup_alpha}, {cutmix_alpha}")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError(f"prob and switch_prob must lie in [0, 1]: got {prob}, {switch_prob}")
        if mode not in ("batch", "elem"):
            raise ValueError(f"mode must be 'batch' or 'elem', not {mode!r}")
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob, self.mode = float(mixup_alpha), float(cutmix_alpha), float(prob), float(switch_prob), mode
        self.rng = np.random.default_rng(seed)
        self.last_draw = None

    def _decide(self, S: int):
        """One decision: (voxel lam, box or None, target lam)."""
        if not (self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0) or not self.rng.random() < self.prob:
            return 1.0, None, 1.0
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cutmix = bool(self.rng.random() < self.switch_prob)
        else:
            cutmix = self.cutmix_alpha > 0.0
        alpha = self.cutmix_alpha if cutmix else self.mixup_alpha
        lam = float(self.rng.beta(alpha, alpha))
        if not cutmix:
            return lam, None, lam
        box, lam = rand_box3d(S, lam, self.rng)
        return 1.0, box, lam

    def draw(self, B: int, S: int):
        decisions = [self._decide(S)] * B if self.mode == "batch" else [self._decide(S) for _ in range(B)]
        lam_x = torch.tensor([d[0] for d in decisions], dtype=torch.float32)
        lam_y = torch.tensor([d[2] for d in decisions], dtype=torch.float32)
        box = None
        if any(d[1] is not None for d in decisions):
            box = torch.tensor([d[1] if d[1] is not None else (0,) * 6 for d in decisions], dtype=torch.int32)
        self.last_draw = (lam_x, box, lam_y)
        return self.last_draw

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise _lib.HctError("Mixup mixes on the GPU (libheadct_hip); no CPU fallback exists")
        lam_x, box, lam_y = self.draw(x.shape[0], x.shape[2])
        if box is not None or bool((lam_x != 1).any()):
            mix_volumes(x, lam_x, box)
        return lam_y.to(x.device)


def mix_multilabel_targets(y: torch.Tensor, lam: torch.Tensor) -> torch.Tensor:
    """The label table [B, T] of a mixed batch in multi-label mode: lam[b] * y[b] + (1 - lam[b]) * y[B - 1 - b] where both entries
    are valid, missing (-1) where either is missing (negative or NaN).  `bce_with_logits` takes the soft entries as they are."""
    y = y.to(torch.float32)
    other = y.flip(0)
    lam = lam.to(device=y.device, dtype=torch.float32).view(-1, 1)
    valid = (y >= 0) & (other >= 0)  # a NaN compares false
    return torch.where(valid, lam * y + (1.0 - lam) * other, torch.full_like(y, -1.0))


class MixedCriterion:
    """The criterion of a fine-tuning run with the recipe on.  Called as `criterion(logits, target)` it is the plain loss of a run
    without it -- `cross_entropy`, or `bce_with_logits` with `pos_weight` in multi-label mode: no mixing, no smoothing; this is
    what validation and test compute.  Training goes through `mix(data, target)`, which mixes the batch in place and returns
    `(data, state)`, and `train_loss(logits, target, state)`: `soft_cross_entropy` with the state's lam and the smoothing, or in
    multi-label mode `bce_with_logits` on `mix_multilabel_targets`.  Smoothing is defined for the softmax mode only."""

    def __init__(self, mixup: Optional[Mixup] = None, smoothing: float = 0.0, multilabel: bool = False, pos_weight: Optional[torch.Tensor] = None):
        smoothing = float(smoothing)
        if not 0.0 <= smoothing < 1.0:
            raise ValueError(f"smoothing must lie in [0, 1): got {smoothing}")
        if multilabel and smoothing > 0.0:
            raise ValueError("label smoothing is defined for the softmax mode only, not for multi-label (sigmoid) outputs")
        self.mixup, self.smoothing, self.multilabel, self.pos_weight = mixup, smoothing, bool(multilabel), pos_weight

    def __call__(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self.multilabel:
            return bce_with_logits(logits, target, self.pos_weight)
        return cross_entropy(logits, target)

    def mix(self, data: torch.Tensor, target: torch.Tensor):
        """(data mixed in place, state); the state is the target-side lam [B] on the device, None without a `Mixup`."""
        return data, (self.mixup(data) if self.mixup is not None else None)

    def train_loss(self, logits: torch.Tensor, target: torch.Tensor, state) -> torch.Tensor:
        if self.multilabel:
            return bce_with_logits(logits, target if state is None else mix_multilabel_targets(target, state), self.pos_weight)
        return soft_cross_entropy(logits, target, state, self.smoothing)
