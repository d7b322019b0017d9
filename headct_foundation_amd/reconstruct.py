"""Inference side of a trained MaskedAutoencoderViT: reconstructions and per-patch error maps.

One random mask predicts only the masked share of a scan.  An error map needs every patch predicted from context at least once,
so `reconstruct` runs a SCHEDULE of masks and accumulates: per volume a seeded random permutation puts the L patches on a ring of
slots, and pass p of n masks the window of M = L - K consecutive slots that starts at (p L) // n.  The windows cover the ring iff
n >= ceil(L / M) (`cover_passes`).  The mask is injected through `forward(x, noise=)`: the noise is the slot's distance past the
window's end, integer-valued and distinct, so the model's own rank kernel keeps exactly the K slots outside the window and
nothing in the model changes.

After every forward (under `torch.no_grad()`, which predicts every patch) `hct_mae_recon_accum` reads the plan's prediction and mask
activations in place -- no copy, no `.float()` -- and adds, for the masked patches only, the de-normalised prediction into a
volume-layout sum (unpatchify fused) and the patch's loss term into an error sum; `hct_mae_recon_finish` divides by the counts and
pastes the scan itself where a patch was never masked.  The kernels run on the GPU only (no CPU fallback exists); the schedule is
plain torch.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib


def cover_passes(L: int, K: int) -> int:
    """The least number of passes whose ring windows of M = L - K masked slots cover all L slots: ceil(L / M)."""
    M = L - K
    if not 0 < M <= L:
        raise ValueError(f"no patch is masked: L = {L} patches, K = {K} kept (mask_ratio too small)")
    return -(-L // M)


def window_start(p: int, n: int, L: int) -> int:
    return (p * L) // n


def cover_slots(B: int, L: int, seed: int = 0, device=None) -> torch.Tensor:
    """slot [B, L] int64: the position of patch l in its volume's seeded random permutation (argsort of torch.rand(B, L); drawn on the
    CPU so that a seed means the same schedule everywhere)."""
    g = torch.Generator().manual_seed(int(seed))
    slot = torch.argsort(torch.rand(B, L, generator=g), dim=1)
    return slot if device is None else slot.to(device)


def cover_noise(slot: torch.Tensor, p: int, n: int, K: int) -> torch.Tensor:
    """Masking noise [B, L] fp32 of pass p of n: float((slot - start_p - M) mod L).  The K smallest values are the slots outside
    the window {(start_p + j) mod L : j < M}; values are distinct integers, exact in fp32 (L < 2^24)."""
    L = slot.shape[1]
    M = L - K
    if not 0 <= p < n:
        raise ValueError(f"pass {p} outside [0, {n})")
    if not 0 < M <= L:
        raise ValueError(f"no patch is masked: L = {L} patches, K = {K} kept (mask_ratio too small)")
    return torch.remainder(slot - window_start(p, n, L) - M, L).to(torch.float32)


def cover_masks(slot: torch.Tensor, n: int, K: int) -> torch.Tensor:
    """masks [n, B, L] uint8 of the schedule, from the ring windows directly (1 = masked)."""
    L = slot.shape[1]
    M = L - K
    return torch.stack([(torch.remainder(slot - window_start(p, n, L), L) < M).to(torch.uint8) for p in range(n)])


def resolve_passes(L: int, K: int, passes: Optional[int]) -> int:
    need = cover_passes(L, K)
    if passes is None:
        return need
    passes = int(passes)
    if passes < 1:
        raise ValueError(f"passes must be at least 1, got {passes}")
    if 2 <= passes < need:
        raise ValueError(f"passes = {passes} leaves patches that are never masked: covering L = {L} patches with M = {L - K} masked per pass "
                         f"takes cover_passes = {need} (use passes=1 for a single random mask)")
    return passes


@dataclass
class Reconstruction:
    recon: torch.Tensor                    # [B, C, S, S, S] fp32: mean prediction where a patch was masked, the scan elsewhere
    error: torch.Tensor                    # [B, g, g, g] fp32: mean over its masked passes of the patch's loss term (0 if never masked)
    count: torch.Tensor                    # [B, g, g, g] int32: passes that masked the patch
    loss: torch.Tensor                     # [n] fp32: the forward's own loss per pass
    masks: torch.Tensor                    # [n, B, L] uint8
    error_volume: Optional[torch.Tensor] = None  # [B, S, S, S] fp32: `error` of the voxel's patch


def recon_accum(pred: torch.Tensor, has_cls_row: bool, x: torch.Tensor, mask: torch.Tensor, P: int, norm_pix: bool, recon_sum: torch.Tensor,
                err_sum: torch.Tensor, cnt: torch.Tensor) -> None:
    """`hct_mae_recon_accum` on tensors: pred [B (L + 1), pd] / [B, L, pd] (bf16 or fp32), x [B, C, S, S, S] (fp32 or fp16), mask [B, L]
    fp32; recon_sum (fp32, like x), err_sum [B, L] fp32 and cnt [B, L] int32 are updated in place."""
    if not (pred.is_cuda and x.is_cuda):
        raise _lib.HctError("recon_accum runs on the GPU (no CPU fallback exists)")
    B, C, S = x.shape[0], x.shape[1], x.shape[2]
    for t, dt in ((mask, torch.float32), (recon_sum, torch.float32), (err_sum, torch.float32), (cnt, torch.int32)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"expected a contiguous {dt} tensor, got {t.dtype}")
    if not (pred.is_contiguous() and x.is_contiguous()) or pred.dtype not in (torch.float32, torch.bfloat16) or x.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"pred {pred.dtype} must be contiguous fp32 / bf16 and x {x.dtype} contiguous fp32 / fp16")
    if P > 0 and S % P == 0:  # (other geometries are refused by the library, by name)
        L = (S // P) ** 3
        if pred.numel() != B * (L + int(has_cls_row)) * P ** 3 * C or mask.numel() != B * L or cnt.numel() != B * L or err_sum.numel() != B * L \
                or recon_sum.numel() != x.numel():
            raise ValueError(f"shapes do not fit B = {B}, C = {C}, S = {S}, P = {P}: pred {tuple(pred.shape)}, mask {tuple(mask.shape)}")
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().hct_mae_recon_accum(pred.data_ptr(), _lib.dtype_code(pred), int(has_cls_row), x.data_ptr(), _lib.dtype_code(x),
                                                   mask.data_ptr(), B, C, S, P, int(norm_pix), recon_sum.data_ptr(), err_sum.data_ptr(),
                                                   cnt.data_ptr(), _lib.stream_ptr()), "hct_mae_recon_accum")


def recon_finish(recon_sum: torch.Tensor, err_sum: torch.Tensor, cnt: torch.Tensor, x: torch.Tensor, P: int, error_volume: bool = False,
                 inplace: bool = True):
    """`hct_mae_recon_finish`: (recon, err [B, L], err_vol or None).  `inplace` writes recon over recon_sum."""
    if not x.is_cuda:
        raise _lib.HctError("recon_finish runs on the GPU (no CPU fallback exists)")
    B, C, S = x.shape[0], x.shape[1], x.shape[2]
    with torch.cuda.device(x.device):
        recon = recon_sum if inplace else torch.empty_like(recon_sum)
        err = torch.empty_like(err_sum)
        vol = torch.empty(B, S, S, S, dtype=torch.float32, device=x.device) if error_volume else None
        _lib.check(_lib.load().hct_mae_recon_finish(recon_sum.data_ptr(), err_sum.data_ptr(), cnt.data_ptr(), x.data_ptr(), _lib.dtype_code(x), B, C,
                                                    S, P, recon.data_ptr(), err.data_ptr(), _lib.ptr(vol), _lib.stream_ptr()), "hct_mae_recon_finish")
    return recon, err, vol


def reconstruct(model, x: torch.Tensor, passes: Optional[int] = None, seed: int = 0, noise: Optional[torch.Tensor] = None,
                error_volume: bool = False) -> Reconstruction:
    """Reconstruction and error map of the volumes x [B, C, S, S, S] (fp32 or fp16) with a MaskedAutoencoderViT.

    passes=None: `cover_passes` passes, the fewest that mask every patch at least once; passes=1: one random mask (an explicit
    `noise` [B, L] may be given); 2 <= passes < cover_passes raises.  `seed` fixes the permutations.  The model's `training` flag,
    gradients, flat buffers and optimizer state are left as they were."""
    if not x.is_cuda:
        raise _lib.HctError("reconstruct (HIP) got a CPU tensor: this path has no CPU fallback")
    L, K = model.num_patches, model.len_keep
    n = resolve_passes(L, K, passes)
    if noise is not None and n != 1:
        raise ValueError(f"an explicit noise is one mask: it needs passes=1, got {n} passes")
    B = x.shape[0]
    expect = (B, model.in_chans) + tuple(model.input_size)
    if tuple(x.shape) != expect:
        raise _lib.HctError(f"input shape {tuple(x.shape)} != {expect}")
    x = x.contiguous() if x.dtype == torch.float16 else x.contiguous().float()  # (as forward takes it)
    S, P = model.input_size[0], model.patch_size[0]
    g = model.grid_size[0]
    dev = x.device
    if noise is not None:
        if tuple(noise.shape) != (B, L):
            raise ValueError(f"noise must be [B, L] = [{B}, {L}], got {tuple(noise.shape)}")
        noises = [noise.to(dev).contiguous().float()]
    else:
        slot = cover_slots(B, L, seed, dev)
        noises = [cover_noise(slot, p, n, K) for p in range(n)]

    with torch.cuda.device(dev):
        recon_sum = torch.empty(expect, dtype=torch.float32, device=dev)
        err_sum = torch.empty(B, L, dtype=torch.float32, device=dev)
        cnt = torch.zeros(B, L, dtype=torch.int32, device=dev)
        losses = torch.empty(n, dtype=torch.float32, device=dev)
        masks = torch.empty(n, B, L, dtype=torch.uint8, device=dev)
    was_training = model.training
    overwrite = getattr(model, "_grad_overwrite", None)
    model.eval()
    try:
        with torch.no_grad():
            for p, nz in enumerate(noises):
                loss, _, _ = model(x, noise=nz)
                losses[p] = loss
                plan = model._plan_for(B)
                mask = plan.activation("mask")
                masks[p] = mask.view(B, L).to(torch.uint8)
                recon_accum(plan.activation("pred_full"), True, x, mask, P, model.norm_pix_loss, recon_sum, err_sum, cnt)
            recon, err, vol = recon_finish(recon_sum, err_sum, cnt, x, P, error_volume=error_volume, inplace=True)
    finally:
        model.train(was_training)
        if overwrite is not None:
            model._grad_overwrite = overwrite
    return Reconstruction(recon=recon, error=err.view(B, g, g, g), count=cnt.view(B, g, g, g), loss=losses, masks=masks, error_volume=vol)


def anomaly_score(error: torch.Tensor, count: torch.Tensor, reduce: str = "mean") -> torch.Tensor:
    """One score [B] per volume from an error map: the mean or the maximum of `error` over the patches with count > 0 (a volume
    without any such patch scores 0)."""
    if reduce not in ("mean", "max"):
        raise ValueError(f"reduce {reduce!r} not supported ('mean' or 'max')")
    B = error.shape[0]
    e = error.reshape(B, -1).to(torch.float32)
    seen = count.reshape(B, -1) > 0
    if reduce == "mean":
        return (e * seen).sum(dim=1) / seen.sum(dim=1).clamp(min=1)
    top = torch.where(seen, e, torch.full_like(e, float("-inf"))).max(dim=1).values
    return torch.where(seen.any(dim=1), top, torch.zeros_like(top))
