"""iBOT masked patch-token loss on the HIP path (DINOv2's second objective; DESIGN.md "iBOT").

Built: `IBotMaskGenerator` (block-wise masks in 3-D, drawn on the host like the affine draws), `ibot_rows_and_weights` (the host's
index list of the masked tokens and their 1 / count weights), `IBOTPatchLoss` (DINOv2 `iBOTPatchLoss.forward_masked` over
hct_ibot_loss / hct_ibot_loss_sk, with a centre of its own) and `pad_head_rows`.  The student sees the two global crops with the
masked patches replaced by the backbone's `mask_token` (`ViTBackbone(mask_token=True)`), the teacher sees them whole; the shared
`DINOHead` runs on the masked patch tokens of both (`MultiCropWrapper.forward(..., patch_rows=...)`).  No CPU fallback for the loss.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib
from ._lib import HctError
from .dino import CENTERING_MODES, sinkhorn_knopp_logs

ASPECT_MIN = 0.3      # axis aspect of a cuboid: log-uniform in [0.3, 1 / 0.3]
CUBOID_ATTEMPTS = 10  # tries at placing one cuboid that adds a patch before the mask is filled up patch by patch
HEAD_ROW_MULTIPLE = 16  # the prototype layer's dgrad runs its split-K path on row counts that are multiples of 16


class IBotMaskGenerator:
    """Masks of the two global crops, `__call__(n_g)` -> uint8 `[n_g, L]` (L = grid ** 3 patches, row-major).

    `n_m = int(n_g * sample_prob)` samples are masked (0 of them: ValueError).  Masked sample j draws u uniformly from the j-th of n_m
    equal sub-intervals of `ratio` and masks exactly `max(1, int(L * u))` patches: random cuboids of patches (volume uniform in
    1 .. what is still missing, the two aspect draws log-uniform in [0.3, 1 / 0.3], random corner) are added, each clipped in raster
    order to the count that remains; a cuboid that adds nothing is drawn again, at most 10 times, then the mask is filled up with
    uniformly drawn unmasked patches.  The rows are permuted at the end.  numpy, with a generator of its own (`seed`)."""

    def __init__(self, grid: int, ratio=(0.1, 0.5), sample_prob: float = 0.5, seed: int = 0):
        lo, hi = (float(r) for r in ratio)
        if not (int(grid) >= 1):
            raise ValueError(f"IBotMaskGenerator: grid must be a positive integer, got {grid!r}")
        if not (0.0 < lo <= hi <= 1.0):
            raise ValueError(f"IBotMaskGenerator: ratio must satisfy 0 < lo <= hi <= 1, got {ratio!r}")
        if not (0.0 < float(sample_prob) <= 1.0):
            raise ValueError(f"IBotMaskGenerator: sample_prob must lie in (0, 1], got {sample_prob!r}")
        self.grid, self.num_patches = int(grid), int(grid) ** 3
        self.ratio, self.sample_prob = (lo, hi), float(sample_prob)
        self.rng = np.random.default_rng(seed)

    def targets(self, n_m: int):
        """(u_j, target_j) of the n_m masked samples, in sub-interval order (draws from the generator)."""
        lo, hi = self.ratio
        edges = np.linspace(lo, hi, n_m + 1)
        us = [float(self.rng.uniform(edges[j], edges[j + 1])) for j in range(n_m)]
        return [(u, max(1, int(self.num_patches * u))) for u in us]

    def _one(self, target: int) -> np.ndarray:
        g, rng = self.grid, self.rng
        m = np.zeros((g, g, g), dtype=bool)
        count = 0
        log_lo, log_hi = math.log(ASPECT_MIN), math.log(1.0 / ASPECT_MIN)
        while count < target:
            added = 0
            for _ in range(CUBOID_ATTEMPTS):
                remain = target - count
                vol = float(rng.uniform(1.0, float(remain))) if remain > 1 else 1.0
                a1, a2 = math.exp(rng.uniform(log_lo, log_hi)), math.exp(rng.uniform(log_lo, log_hi))
                dims = (vol * a1 * a2) ** (1.0 / 3.0), (vol / a1) ** (1.0 / 3.0), (vol / a2) ** (1.0 / 3.0)
                d = [min(g, max(1, int(round(x)))) for x in dims]
                o = [int(rng.integers(0, g - d[i] + 1)) for i in range(3)]
                sub = m[o[0]:o[0] + d[0], o[1]:o[1] + d[1], o[2]:o[2] + d[2]]
                free = np.argwhere(~sub)  # raster order
                if len(free) == 0:
                    continue
                free = free[:remain]  # clipped to the count that remains
                sub[free[:, 0], free[:, 1], free[:, 2]] = True
                added = len(free)
                break
            if added == 0:
                break
            count += added
        flat = m.reshape(-1)
        if count < target:  # fill with uniformly drawn unmasked patches
            free = np.flatnonzero(~flat)
            flat[rng.choice(free, size=target - count, replace=False)] = True
        return flat

    def __call__(self, n_g: int) -> np.ndarray:
        n_m = int(n_g * self.sample_prob)
        if n_m < 1:
            raise ValueError(f"IBotMaskGenerator: int({n_g} * {self.sample_prob}) = 0 samples to mask; raise DINO.IBOT_MASK_PROB or the batch size")
        masks = np.zeros((n_g, self.num_patches), dtype=np.uint8)
        for j, (_, target) in enumerate(self.targets(n_m)):
            masks[j] = self._one(target)
        return masks[self.rng.permutation(n_g)]


def ibot_rows_and_weights(masks: np.ndarray, num_register_tokens: int = 0):
    """From host masks `[n_g, L]`: (rows int32 [M], weights fp32 [M], M).  rows[i] = b * (1 + R + L) + 1 + R + l is the row of masked
    token i inside the `[n_g * (1 + R + L), D]` token matrix, (b, l) in row-major order; weights[i] = 1 / (masked patches of sample
    b).  Host arithmetic only: nothing is read back from the device."""
    masks = np.asarray(masks)
    n_g, L = masks.shape
    T1 = 1 + int(num_register_tokens) + L
    b, l = np.nonzero(masks)
    rows = (b * T1 + 1 + int(num_register_tokens) + l).astype(np.int32)
    counts = masks.astype(bool).sum(axis=1)
    weights = (1.0 / counts[b]).astype(np.float32)
    return rows, weights, int(rows.shape[0])


def pad_head_rows(n_rows: int, multiple: int = HEAD_ROW_MULTIPLE) -> int:
    """Rows the head runs on: `n_rows` rounded up to a multiple of 16."""
    return (int(n_rows) + multiple - 1) // multiple * multiple


class _IbotLossFn(torch.autograd.Function):
    """hct_ibot_loss (sk None) / hct_ibot_loss_sk (sk = (lc, lr, log N)) on M paired rows, in the logits' own dtype."""

    @staticmethod
    def forward(ctx, student, teacher, weight, inv_images, student_temp, teacher_temp, center, center_sum, sk):
        lib = _lib.load()
        if not (student.is_cuda and teacher.is_cuda and weight.is_cuda):
            raise HctError("IBOTPatchLoss (HIP) needs GPU tensors; there is no CPU fallback")
        if student.dtype not in (torch.float32, torch.bfloat16) or teacher.dtype != student.dtype:
            raise HctError("IBOTPatchLoss (HIP): student / teacher logits must both be fp32 or both bf16")
        M, K = student.shape
        if tuple(teacher.shape) != (M, K) or weight.dtype != torch.float32 or tuple(weight.shape) != (M,) or M < 1 or K % 4:
            raise HctError(f"IBOTPatchLoss: student {tuple(student.shape)}, teacher {tuple(teacher.shape)}, weight {tuple(weight.shape)} "
                           f"{weight.dtype}: M >= 1 paired rows of K % 4 == 0 logits and one fp32 weight per row")
        # a row slice of a larger [rows, K] buffer is contiguous and is read where it lies
        student, teacher, weight = student.contiguous(), teacher.contiguous(), weight.contiguous()
        ws = torch.empty(max(16, lib.hct_ibot_loss_workspace_bytes(M, K)), dtype=torch.uint8, device=student.device)
        loss = torch.empty(1, dtype=torch.float32, device=student.device)
        dstudent = torch.empty_like(student) if ctx.needs_input_grad[0] else None
        st = _lib.stream_ptr()
        if sk is None:
            _lib.check(lib.hct_ibot_loss(student.data_ptr(), teacher.data_ptr(), _lib.dtype_code(student), M, K, weight.data_ptr(), center.data_ptr(),
                                         float(student_temp), float(teacher_temp), float(inv_images), loss.data_ptr(), _lib.ptr(dstudent), None,
                                         _lib.ptr(center_sum), ws.data_ptr(), ws.numel(), st), "hct_ibot_loss")
        else:
            lc, lr, log_n = sk
            _lib.check(lib.hct_ibot_loss_sk(student.data_ptr(), teacher.data_ptr(), _lib.dtype_code(student), M, K, weight.data_ptr(), lc.data_ptr(),
                                            lr.data_ptr(), float(log_n), float(student_temp), float(teacher_temp), float(inv_images),
                                            loss.data_ptr(), _lib.ptr(dstudent), None, ws.data_ptr(), ws.numel(), st), "hct_ibot_loss_sk")
        ctx.dstudent = dstudent
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        if ctx.dstudent is None:
            raise HctError("IBOTPatchLoss: the forward ran without gradient storage")
        return (ctx.dstudent * g.to(ctx.dstudent.dtype),) + (None,) * 8


def _world() -> int:
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class IBOTPatchLoss(nn.Module):
    """DINOv2's `iBOTPatchLoss.forward_masked`: `forward(student_rows, teacher_rows, weights, n_images, epoch)` with the M masked patch
    tokens' logits of student and teacher `[M, K]` (fp32 or bf16, read as they are), `weights [M]` = 1 / masked patches of the token's
    image and `n_images` = the global crops of this rank:  loss = -(1 / n_images) sum_i w_i sum_k q_ik log_softmax(s_i / T_s)_k.
    The teacher temperature follows `DINOLoss`'s schedule.  `centering='centering'`: q = softmax((t - center) / T_t) with this
    module's own `center` buffer, moved by the mean of the masked teacher rows of all ranks (momentum `center_momentum`);
    'sinkhorn_knopp': `sk_iters` Sinkhorn-Knopp iterations over the masked rows of all ranks, `center` left alone."""

    def __init__(self, out_dim, warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs, nepochs, student_temp=0.1, center_momentum=0.9,
                 centering="centering", sk_iters=3):
        super().__init__()
        if centering not in CENTERING_MODES:
            raise ValueError(f"IBOTPatchLoss: centering must be one of {CENTERING_MODES}, got {centering!r}")
        if centering == "sinkhorn_knopp" and int(sk_iters) < 1:
            raise ValueError(f"IBOTPatchLoss: sk_iters must be at least 1, got {sk_iters}")
        self.centering, self.sk_iters = centering, int(sk_iters)
        self.student_temp, self.center_momentum = student_temp, center_momentum
        self.register_buffer("center", torch.zeros(1, out_dim))
        self.teacher_temp_schedule = np.concatenate((np.linspace(warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs),
                                                     np.ones(nepochs - warmup_teacher_temp_epochs) * teacher_temp))

    def total_rows(self, M: int, device) -> int:
        """Masked rows of all ranks (M itself without a process group; one small all-reduce and its read-back with one)."""
        if _world() == 1:
            return int(M)
        n = torch.tensor([int(M)], dtype=torch.int64, device=device)
        dist.all_reduce(n)
        return int(n.item())

    def forward(self, student_rows, teacher_rows, weights, n_images, epoch, n_total=None):
        """`n_total`: the masked rows of all ranks where the caller knows them (tests that stand for several ranks); default: asked."""
        temp = float(self.teacher_temp_schedule[epoch])
        M = int(student_rows.shape[0])
        teacher = teacher_rows.detach()
        n_total = self.total_rows(M, student_rows.device) if n_total is None else int(n_total)
        inv_images = 1.0 / float(n_images)
        if self.centering == "sinkhorn_knopp":
            sk = sinkhorn_knopp_logs(teacher, temp, self.sk_iters, n_total=n_total)
            return _IbotLossFn.apply(student_rows, teacher, weights, inv_images, self.student_temp, temp, None, None, sk)
        csum = torch.empty(self.center.shape[1], dtype=torch.float32, device=self.center.device)
        loss = _IbotLossFn.apply(student_rows, teacher, weights, inv_images, self.student_temp, temp, self.center, csum, None)
        self._apply_center(csum, n_total)
        return loss

    @torch.no_grad()
    def _apply_center(self, csum, n_total):
        if _world() > 1:
            dist.all_reduce(csum)
        _lib.check(_lib.load().hct_dino_center_update(self.center.data_ptr(), csum.data_ptr(), csum.numel(), float(self.center_momentum),
                                                      float(n_total), _lib.stream_ptr()), "hct_dino_center_update")


class IBotObjective:
    """What the DINO engine needs for the iBOT term: its weight, the mask generator and the patch loss.  `draw(n_g, device)` makes one
    step's masks and returns (masks uint8 [n_g, L] on the device, rows: host int32 [M], weights fp32 [M] on the device); everything
    is built on the host and uploaded, nothing is read back."""

    def __init__(self, weight: float, generator: IBotMaskGenerator, loss: IBOTPatchLoss, num_register_tokens: int = 0):
        self.weight, self.generator, self.loss = float(weight), generator, loss
        self.num_register_tokens = int(num_register_tokens)

    def draw(self, n_g: int, device):
        masks = self.generator(n_g)
        rows, weights, _ = ibot_rows_and_weights(masks, self.num_register_tokens)
        return (torch.from_numpy(masks).to(device, non_blocking=True), rows, torch.from_numpy(weights).to(device, non_blocking=True))
