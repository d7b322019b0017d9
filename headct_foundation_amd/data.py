"""Input side of the engines.  The reference's MONAI loading pipeline (src/data/*.py: NIfTI -> RAS -> 1 mm -> foreground crop ->
HU window -> resize -> fp16 persistent cache) is rebuilt without MONAI or nibabel: the file is decoded on the host (nifti.py),
everything from the raw voxels to the cache item runs on the device (`load_volume`, csrc/loading.hip), `VolumeCache` keeps the
items on disk and `PretrainVolumes` feeds them to the engines as [B, C, S, S, S] fp16 batches, with the reference's sampler and
placeholder rule.  With DATA.SYNTHETIC the engines are fed synthetic volumes with the value range of windowed CT, U[0,1)
(transforms.py:120-128), generated per rank with seed SEED + rank like the reference seeds its ranks (main_pretrain_mae.py:213).
The per-sample device side: `DeviceAugment` = the train-time transforms of `mae3d_transforms` (cast of the cached fp16 volume,
three axis flips, intensity shift as one HIP kernel; the optional Gaussian smoothing as three 1-D passes) and `window_hu`; for the
DINO engine `DeviceAugmentDINO3D` = `DataAugmentationDINO3D` (every view of a batch resampled in one launch) behind `MultiCropLoader`; and for
fine-tuning `LabelledVolumes` = the reference's labelled datasets and samplers (class-balanced draws, few-shot tables) over a `DevicePool`,
the shard's cache items resident on the device, from which `gather_augment` makes a batch in one launch -- with `RandAffine3D`
(TRAIN.AFFINE_*: random rotation, zoom and translation, an addition of this build) resampled through a per-sample 3 x 4 matrix in that same launch."""
from __future__ import annotations

import csv
import hashlib
import logging
import os
import tempfile
import threading
from collections import OrderedDict, deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import nifti


GAUSS_TAPS = 9  # taps per axis the kernel takes (kGaussTaps): sigma <= 1.06 at MONAI's truncation of 4 sigma


def gaussian_taps(sigma: torch.Tensor) -> torch.Tensor:
    """Centred 1-D kernels for sigmas [...] -> [..., GAUSS_TAPS] fp32, as MONAI's `gaussian_1d(sigma, truncated=4.0, approx="erf")`
    builds them (fp32: tail = int(max(4 sigma, 0.5) + 0.5); w(x) = 0.5 (erf(t (x + 0.5)) - erf(t (x - 0.5))), t = 0.70710678 / |sigma|,
    clamped at 0, NOT renormalised), zero beyond the tail.  Stated from knowledge of MONAI 1.2 / 1.3 (not installed here)."""
    sigma = sigma.to(torch.float32)
    tail = torch.clamp(sigma * 4.0, min=0.5).add(0.5).to(torch.int64)
    if int(tail.max()) > GAUSS_TAPS // 2:
        raise ValueError(f"sigma {float(sigma.max())} needs more than {GAUSS_TAPS} taps")
    x = torch.arange(-(GAUSS_TAPS // 2), GAUSS_TAPS // 2 + 1, dtype=torch.float32)
    t = (0.70710678 / sigma.abs()).unsqueeze(-1)
    w = (0.5 * ((t * (x + 0.5)).erf() - (t * (x - 0.5)).erf())).clamp(min=0)
    return torch.where(x.abs() <= tail.unsqueeze(-1).to(torch.float32), w, torch.zeros_like(w))


def _rows3(v, B: int, what: str) -> np.ndarray:
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    if a.shape != (B, 3):
        raise ValueError(f"{what} must be [{B}, 3], not {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} has a non-finite entry")
    return a


def affine_matrices(angles_deg, scale, translate_vox, flip=None) -> torch.Tensor:
    """The [B, 12] fp32 table `hct_affine_augment` takes: per sample the rows of [A | t], the map from OUTPUT voxel coordinates to
    INPUT voxel coordinates about the volume centre c = (S - 1) / 2:  out[i] = in(A (i - c) + t + c), axis 0 the slowest.

        A = R . diag(scale) . F,   R = R2(angles[2]) . R1(angles[1]) . R0(angles[0]),   t = translate_vox

    R_a(theta) rotates about spatial axis a, right-handed in (axis 0, axis 1, axis 2) coordinates:
        R0 = [[1, 0, 0], [0, c, -s], [0, s, c]],  R1 = [[c, 0, s], [0, 1, 0], [-s, 0, c]],  R2 = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    so R2(90 deg) reads input (-i1, i0, i2) at output (i0, i1, i2) (centred): the content turns by -90 deg, as with every
    output-to-input map.  scale > 1 reads from further out: the content shrinks.  A positive t_a moves the content towards
    lower indices of axis a.  F = diag(+-1), -1 on axis a where bit a of flip[b] is set, acts on the output index first: the result
    is the affine transform applied first and the flips after it (flip(resample(x)), the order of RandAffine followed by RandFlip).
    angles_deg, scale, translate_vox: [B, 3] (tensors, arrays or lists); flip: [B] integers or None.  Computed in float64 and
    rounded to fp32 once; a non-finite input raises ValueError."""
    ang = np.asarray(angles_deg.detach().cpu().numpy() if isinstance(angles_deg, torch.Tensor) else angles_deg, dtype=np.float64)
    B = ang.shape[0] if ang.ndim == 2 else -1
    ang, sc, tr = _rows3(ang, B, "angles_deg"), _rows3(scale, B, "scale"), _rows3(translate_vox, B, "translate_vox")
    bits = np.zeros(B, dtype=np.int64) if flip is None else np.asarray(flip.cpu().numpy() if isinstance(flip, torch.Tensor) else flip, dtype=np.int64).reshape(-1)
    if bits.shape != (B,):
        raise ValueError(f"flip must have {B} entries")
    th = np.deg2rad(ang)
    c, s = np.cos(th), np.sin(th)
    # exact at multiples of 90 degrees, where the float64 cosine of pi / 2 is 6e-17 instead of 0
    quarter = np.round(ang / 90.0)
    exact = quarter * 90.0 == ang
    c = np.where(exact, np.array([1.0, 0.0, -1.0, 0.0])[quarter.astype(np.int64) % 4], c)
    s = np.where(exact, np.array([0.0, 1.0, 0.0, -1.0])[quarter.astype(np.int64) % 4], s)
    one, zero = np.ones(B), np.zeros(B)
    stack = lambda rows: np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)
    R0 = stack([[one, zero, zero], [zero, c[:, 0], -s[:, 0]], [zero, s[:, 0], c[:, 0]]])
    R1 = stack([[c[:, 1], zero, s[:, 1]], [zero, one, zero], [-s[:, 1], zero, c[:, 1]]])
    R2 = stack([[c[:, 2], -s[:, 2], zero], [s[:, 2], c[:, 2], zero], [zero, zero, one]])
    F = np.stack([np.where((bits >> a) & 1, -1.0, 1.0) for a in range(3)], axis=-1)
    A = (R2 @ R1 @ R0) * (sc * F)[:, None, :]  # column k scaled by scale_k * F_k
    return torch.from_numpy(np.concatenate([A, tr[:, :, None]], axis=-1).reshape(B, 12).astype(np.float32))


def _three(v, what: str) -> tuple:
    v = [float(x) for x in (v if isinstance(v, (list, tuple)) else [v])]
    if len(v) == 1:
        v = v * 3
    if len(v) != 3 or not all(np.isfinite(x) and x >= 0 for x in v):
        raise ValueError(f"{what} must be one or three finite numbers >= 0: got {v}")
    return tuple(v)


class RandAffine3D:
    """MONAI's RandAffine for cubic volumes, as draws for `hct_affine_augment` (an addition of this build: the reference's
    vit_transforms has no affine).  Per sample: fire ~ Bernoulli(prob); angles ~ U(-r_a, r_a) degrees about axis a (`rotate_deg`: a
    number or three); a scale factor ~ U(1 - s, 1 + s) (`scale` = s in [0, 1): one factor for the three axes, or one per axis when
    `isotropic_scale` is False); a translation ~ U(-tau_a, tau_a) * S voxels per axis (`translate`: fractions of S, a number or
    three).  The conventions are `affine_matrices`'.  Every number is drawn whether or not the sample fires, from a generator of
    this object's OWN: the flip / shift stream of the DeviceAugment it is attached to is the same with and without it.
    `last_draw` keeps {fire bool [B], angles_deg, scale, translate_vox: float64 [B, 3]} of the last batch."""

    def __init__(self, rotate_deg=10.0, scale=0.1, translate=0.05, prob: float = 0.5, isotropic_scale: bool = True, seed: int = 0):
        self.rotate_deg, self.translate = _three(rotate_deg, "rotate_deg"), _three(translate, "translate")
        self.scale, self.prob, self.isotropic_scale = float(scale), float(prob), bool(isotropic_scale)
        if max(self.rotate_deg) > 180.0 or not 0.0 <= self.scale < 1.0 or max(self.translate) >= 1.0 or not 0.0 <= self.prob <= 1.0:
            raise ValueError(f"RandAffine3D: need angles in [0, 180], 0 <= scale < 1, translate in [0, 1) and prob in [0, 1]: got "
                             f"{self.rotate_deg}, {self.scale}, {self.translate}, {self.prob}")
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(seed)
        self.last_draw = None

    def draw(self, B: int, S: int) -> dict:
        u = torch.rand(B, 10, generator=self.gen, dtype=torch.float64)
        sym = lambda cols, half: (u[:, cols] * 2 - 1) * torch.tensor(half, dtype=torch.float64)
        factor = 1 + sym(slice(4, 7), [self.scale] * 3)
        if self.isotropic_scale:
            factor = factor[:, :1].expand(B, 3).contiguous()
        self.last_draw = {"fire": u[:, 0] < self.prob, "angles_deg": sym(slice(1, 4), self.rotate_deg), "scale": factor,
                          "translate_vox": sym(slice(7, 10), self.translate) * S}
        return self.last_draw

    def matrices(self, d: dict, flip=None) -> torch.Tensor:
        """[B, 12] fp32 of a draw, the flips of the same batch folded in (they act after the affine)."""
        return affine_matrices(d["angles_deg"], d["scale"], d["translate_vox"], flip)


def _checked_mat(mat, fire, B: int):
    """`mat` [B, 12] / `fire` [B] as the kernel wants them; what is given on the CPU is checked here (the kernel cannot refuse a
    table that lives on the device, and is safe against any)."""
    if mat is None:
        if fire is not None:
            raise ValueError("fire without mat")
        return None, None
    if mat.numel() != B * 12 or (fire is not None and fire.numel() != B):
        raise ValueError(f"mat must be [{B}, 12] and fire [{B}]")
    if not mat.is_cuda and not bool(torch.isfinite(mat).all()):
        raise ValueError("mat has a non-finite entry")
    return mat, fire


def affine_augment(x: torch.Tensor, mat: torch.Tensor, fire: torch.Tensor = None, flip: torch.Tensor = None, shift: torch.Tensor = None) -> torch.Tensor:
    """A stacked batch x [B, C, S, S, S] (fp16 / bf16 / fp32, on the GPU) through hct_affine_augment: fp32 [B, C, S, S, S], sample b
    resampled through mat[b] (see `affine_matrices`) where fire[b] (None: everywhere), flipped by flip[b]'s bits where not, plus
    shift[b].  Tables given on the CPU are checked (a non-finite matrix entry raises) and uploaded."""
    from . import _lib
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.HctError("affine_augment runs on the GPU (libheadct_hip); no CPU fallback exists")
    if x.dim() != 5 or not (x.shape[2] == x.shape[3] == x.shape[4]) or x.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"x must be a [B, C, S, S, S] fp16 / bf16 / fp32 tensor, not {x.dtype} {tuple(x.shape)}")
    B, C, S = x.shape[0], x.shape[1], x.shape[2]
    code = {torch.float16: _lib.HCT_F16, torch.bfloat16: _lib.HCT_BF16, torch.float32: _lib.HCT_F32}[x.dtype]
    mat, fire = _checked_mat(mat, fire, B)
    on = lambda t, dt: None if t is None else t.to(device=x.device, dtype=dt).contiguous()
    mat, fire, flip, shift = on(mat, torch.float32), on(fire, torch.uint8), on(flip, torch.uint8), on(shift, torch.float32)
    if any(t is not None and t.numel() != B for t in (flip, shift)):
        raise ValueError("flip and shift need one entry per sample")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.hct_affine_augment(x.data_ptr(), code, None, 0, out.data_ptr(), B, C, S, _lib.ptr(mat), _lib.ptr(fire), _lib.ptr(flip),
                                          _lib.ptr(shift), _lib.stream_ptr()), "hct_affine_augment")
    return out


class DeviceAugment:
    """mae3d_transforms(mode='train') (src/data/transforms.py:193-238) on a device batch: CastToTyped(float32) ->
    RandFlipd(prob, axis 0/1/2) -> RandShiftIntensityd(offsets, prob) [-> RandGaussianSmoothd(sigma per axis ~ U(0.5, 1), prob 0.2),
    which the reference appends when `reshape` is False: `smooth_prob=0.2` here].  Input: [B,C,S,S,S] fp16 (the cache format,
    transforms.py:170-175), bf16 or fp32; output fp32.  Draws come from a torch generator on the host (MONAI's numpy RandomState
    stream is not reproduced); `last_draw` exposes (flip bits, shift[, smooth flags, sigmas]) for tests.
    With `affine` (a RandAffine3D, which draws from a generator of its own) the samples that fire are resampled through their
    matrix -- affine first, flips after, then the shift -- in the same single launch (hct_affine_augment)."""

    def __init__(self, flip_prob: float = 0.1, shift_offsets: float = 0.1, shift_prob: float = 0.5, seed: int = 0,
                 smooth_prob: float = 0.0, smooth_sigma=(0.5, 1.0), affine: RandAffine3D = None):
        self.flip_prob, self.shift_offsets, self.shift_prob = flip_prob, shift_offsets, shift_prob
        self.smooth_prob, self.smooth_sigma, self.affine = smooth_prob, smooth_sigma, affine
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(seed)
        self.last_draw = None

    def draw(self, B: int):
        """The flips and shifts of one batch, on the CPU: (flip uint8 [B], bit a = spatial axis a; shift fp32 [B], 0 = did not fire)."""
        u = torch.rand(B, 5, generator=self.gen)
        flip = ((u[:, 0] < self.flip_prob).to(torch.uint8) | ((u[:, 1] < self.flip_prob).to(torch.uint8) << 1)
                | ((u[:, 2] < self.flip_prob).to(torch.uint8) << 2))
        shift = torch.where(u[:, 3] < self.shift_prob, (u[:, 4] * 2 - 1) * self.shift_offsets, torch.zeros(B))
        self.last_draw = (flip.clone(), shift.clone())
        return flip, shift

    def draw_affine(self, B: int, S: int, flip: torch.Tensor):
        """(mat fp32 [B, 12] with `flip` folded in, fire uint8 [B]) of one batch on the CPU, or (None, None) without an affine."""
        if self.affine is None:
            return None, None
        d = self.affine.draw(B, S)
        return self.affine.matrices(d, flip), d["fire"].to(torch.uint8)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        from . import _lib
        lib = _lib.load()
        if not x.is_cuda:
            raise _lib.HctError("DeviceAugment runs on the GPU (libheadct_hip); no CPU fallback exists")
        B, C, S = x.shape[0], x.shape[1], x.shape[2]
        code = {torch.float16: _lib.HCT_F16, torch.bfloat16: _lib.HCT_BF16, torch.float32: _lib.HCT_F32}[x.dtype]
        flip, shift = self.draw(B)
        if self.affine is not None:
            mat, fire = self.draw_affine(B, S, flip)
            out = affine_augment(x, mat, fire, flip, shift)
        else:
            x = x.contiguous()
            flip_d, shift_d = flip.to(x.device), shift.to(device=x.device, dtype=torch.float32)
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                st = _lib.stream_ptr()
                _lib.check(lib.hct_augment_volume(x.data_ptr(), code, out.data_ptr(), B, C, S, flip_d.data_ptr(), shift_d.data_ptr(), st),
                           "hct_augment_volume")
        if self.smooth_prob > 0:
            v = torch.rand(B, 4, generator=self.gen)
            fire = v[:, 0] < self.smooth_prob
            lo, hi = self.smooth_sigma
            sigma = lo + (hi - lo) * v[:, 1:4]  # one sigma per spatial axis, drawn whether or not the transform fires (as MONAI's randomize does)
            self.last_draw = self.last_draw + (fire.clone(), sigma.clone())
            if bool(fire.any()):
                out = gaussian_smooth(out, sigma, fire)
        return out


def gaussian_smooth(x: torch.Tensor, sigma: torch.Tensor, apply: torch.Tensor = None) -> torch.Tensor:
    """Separable Gaussian smoothing of fp32 volumes [B,C,S,S,S] with per-sample, per-axis sigmas [B,3] (zero padding at the borders):
    MONAI's GaussianSmooth as RandGaussianSmoothd applies it (src/data/transforms.py:230-238).  apply [B] bool: samples left as is."""
    from . import _lib
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.HctError("gaussian_smooth runs on the GPU (libheadct_hip); no CPU fallback exists")
    if x.dtype != torch.float32:
        raise _lib.HctError("gaussian_smooth takes fp32 volumes (the output of DeviceAugment)")
    x = x.contiguous()
    B, C, S = x.shape[0], x.shape[1], x.shape[2]
    taps = gaussian_taps(sigma.reshape(B, 3)).to(x.device).contiguous()
    flags = (torch.ones(B, dtype=torch.uint8) if apply is None else apply.to(torch.uint8)).to(x.device)
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = _lib.stream_ptr()
        _lib.check(lib.hct_gaussian_smooth3d(x.data_ptr(), out.data_ptr(), tmp.data_ptr(), B, C, S, taps.data_ptr(), flags.data_ptr(), st),
                   "hct_gaussian_smooth3d")
    return out


def _cubic(size, what: str) -> int:
    """An int, or a sequence of three equal ints (the yaml's [96, 96, 96]) -> that int."""
    if isinstance(size, int):
        return size
    size = [int(s) for s in size]
    if len(size) != 3 or len(set(size)) != 1:
        raise NotImplementedError(f"{what} {size} is not implemented: only cubic sizes are (the model side is cubic).")
    return size[0]


class DeviceAugmentDINO3D:
    """DataAugmentationDINO3D (src/data/transforms.py:39-105) on a device batch: per cached volume 2 global + `local_crops_number`
    local views.  Per view, in the reference's order: CastToType(float32) -> ResizeWithPadOrCrop(field) [-> CenterSpatialCrop(
    local_field), local views] -> RandSpatialCrop(random_size, random_center: per axis size = randint(r, m + 1), start =
    randint(0, extent - size + 1); global r = global_crops_size, m = field; local r = local_crops_size, m = global_crops_size)
    -> Resize(final_size, mode "area") [-> RandFlip(0.2) x 3 -> RandShiftIntensity(0.2, prob 0.5), global views]
    [-> RandGaussianSmooth(sigma ~ U(0.5, 1) per axis, prob 0.2), view 0] [-> RandAdjustContrast(gamma ~ U(0.2, 1), prob 0.2), view 1].

    Everything up to the shift is ONE launch for all views of the batch (hct_crop_resize_area): the padded field is never built,
    boxes go to the kernel in input-volume coordinates and what lies outside the volume reads as zero.  Input [B, C, S, S, S]
    fp16 (the cache format), bf16 or fp32; output a list of 2 + n contiguous fp32 tensors [B, C, F, F, F]: views of one
    [V, B, C, F, F, F] buffer, except view 0 when the smoothing fired for some sample (hct_gaussian_smooth3d works out of place).

    The padding / centre-crop offsets, the crop-size and crop-start distributions, Resize's default mode and AdjustContrast's
    formula are stated from knowledge of MONAI 1.2 / 1.3 (not installed here): parity with MONAI itself is unpinned.  Draws come
    from a torch generator on the host (MONAI's numpy RandomState stream is not reproduced); `last_draw` keeps the one used."""

    FLIP_PROB, SHIFT_OFFSETS, SHIFT_PROB = 0.2, 0.2, 0.5
    SMOOTH_PROB, SMOOTH_SIGMA, GAMMA_PROB, GAMMA = 0.2, (0.5, 1.0), 0.2, (0.2, 1.0)

    def __init__(self, final_size, global_crops_size, local_crops_size, local_crops_number: int, seed: int = 0, field: int = 224,
                 local_field: int = 192):
        self.final_size = _cubic(final_size, "final_size")
        self.global_crops_size = _cubic(global_crops_size, "global_crops_size")
        self.local_crops_size = _cubic(local_crops_size, "local_crops_size")
        self.local_crops_number, self.field, self.local_field = int(local_crops_number), int(field), int(local_field)
        if self.final_size % 4:
            raise NotImplementedError(f"final_size {self.final_size} is not implemented: a multiple of 4 is needed (16-byte stores).")
        if not (1 <= self.local_crops_size <= self.global_crops_size <= self.local_field <= self.field):
            raise ValueError(f"need 1 <= local_crops_size ({self.local_crops_size}) <= global_crops_size ({self.global_crops_size}) <= "
                             f"local_field ({self.local_field}) <= field ({self.field})")
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(seed)
        self.last_draw = None
        self._workspace = None

    @property
    def n_views(self) -> int:
        return 2 + self.local_crops_number

    def origins(self, S: int):
        """Input-volume coordinate of voxel 0 of the global field and of the local field (the same on every axis):
        ResizeWithPadOrCrop pads (field - S) // 2 in front where S < field and crops from S // 2 - field // 2 where larger;
        CenterSpatialCrop(local_field) starts at field // 2 - local_field // 2 of that."""
        g = -((self.field - S) // 2) if S <= self.field else S // 2 - self.field // 2
        return g, g + self.field // 2 - self.local_field // 2

    def draw(self, B: int, S: int) -> dict:
        """The random numbers of one batch, on the CPU: boxes int32 [V, B, 6] (start[3], size[3], in INPUT coordinates), flip uint8
        [V, B] (bit a = spatial axis a), shift fp32 [V, B] (0 = did not fire; both zero for local views), smooth_fire bool [B],
        sigma fp32 [B, 3], gamma_fire bool [B], gamma fp32 [B]."""
        V, g = self.n_views, self.gen
        og, ol = self.origins(S)
        lo = torch.tensor([self.global_crops_size] * 2 + [self.local_crops_size] * (V - 2)).view(V, 1, 1)
        hi = torch.tensor([self.field] * 2 + [self.global_crops_size] * (V - 2)).view(V, 1, 1)
        extent = torch.tensor([self.field] * 2 + [self.local_field] * (V - 2)).view(V, 1, 1)
        origin = torch.tensor([og] * 2 + [ol] * (V - 2)).view(V, 1, 1)
        u = torch.rand(2, V, B, 3, generator=g, dtype=torch.float64)
        size = torch.minimum(lo + (u[0] * (hi - lo + 1)).floor().long(), hi)             # randint(r, m + 1), per axis
        start = torch.minimum((u[1] * (extent - size + 1)).floor().long(), extent - size)  # randint(0, extent - size + 1)
        boxes = torch.cat([start + origin, size], dim=-1).to(torch.int32)
        w = torch.rand(2, B, 5, generator=g)
        bit = (w[:, :, :3] < self.FLIP_PROB).to(torch.uint8)
        flip = torch.zeros(V, B, dtype=torch.uint8)
        flip[:2] = bit[..., 0] | (bit[..., 1] << 1) | (bit[..., 2] << 2)
        shift = torch.zeros(V, B)
        shift[:2] = torch.where(w[:, :, 3] < self.SHIFT_PROB, (w[:, :, 4] * 2 - 1) * self.SHIFT_OFFSETS, torch.zeros(2, B))
        v = torch.rand(B, 6, generator=g)  # drawn whether or not the transform fires, as MONAI's randomize does
        sigma = self.SMOOTH_SIGMA[0] + (self.SMOOTH_SIGMA[1] - self.SMOOTH_SIGMA[0]) * v[:, 1:4]
        gamma = self.GAMMA[0] + (self.GAMMA[1] - self.GAMMA[0]) * v[:, 5]
        return {"boxes": boxes, "flip": flip, "shift": shift, "smooth_fire": v[:, 0] < self.SMOOTH_PROB, "sigma": sigma,
                "gamma_fire": v[:, 4] < self.GAMMA_PROB, "gamma": gamma}

    def _upload(self, d: dict, device):
        """The draw as device tensors through ONE pinned buffer and one asynchronous copy: a pageable copy per table would make
        the host wait for the stream, and with it for the training step in front of this batch."""
        B = d["gamma"].numel()
        parts = [d["boxes"].to(torch.int32).contiguous().view(torch.uint8).reshape(-1),
                 d["shift"].to(torch.float32).contiguous().view(torch.uint8).reshape(-1),
                 d["gamma"].to(torch.float32).contiguous().view(torch.uint8).reshape(-1),
                 gaussian_taps(d["sigma"].reshape(B, 3)).contiguous().view(torch.uint8).reshape(-1),
                 d["flip"].to(torch.uint8).reshape(-1), d["smooth_fire"].to(torch.uint8).reshape(-1), d["gamma_fire"].to(torch.uint8).reshape(-1)]
        offs, total = [], 0
        for p in parts:
            offs.append(total)
            total += (p.numel() + 15) // 16 * 16
        host = torch.zeros(total, dtype=torch.uint8, pin_memory=True)
        for p, o in zip(parts, offs):
            host[o:o + p.numel()] = p
        dev = host.to(device, non_blocking=True)
        cut = lambda i, dt: dev[offs[i]:offs[i] + parts[i].numel()].view(dt)
        return (cut(0, torch.int32), cut(1, torch.float32), cut(2, torch.float32), cut(3, torch.float32), cut(4, torch.uint8),
                cut(5, torch.uint8), cut(6, torch.uint8))

    def __call__(self, x: torch.Tensor, draw: dict = None):
        from . import _lib
        lib = _lib.load()
        if not x.is_cuda:
            raise _lib.HctError("DeviceAugmentDINO3D runs on the GPU (libheadct_hip); no CPU fallback exists")
        if x.dim() != 5 or not (x.shape[2] == x.shape[3] == x.shape[4]):
            raise NotImplementedError(f"Volume shape {tuple(x.shape)} is not implemented: [B, C, S, S, S] is.")
        B, C, S = x.shape[0], x.shape[1], x.shape[2]
        V, F = self.n_views, self.final_size
        code = {torch.float16: _lib.HCT_F16, torch.bfloat16: _lib.HCT_BF16, torch.float32: _lib.HCT_F32}[x.dtype]
        d = self.draw(B, S) if draw is None else draw
        if tuple(d["boxes"].shape) != (V, B, 6) or int(d["boxes"][..., 3:].min()) < 1:
            raise ValueError(f"draw['boxes'] must be [{V}, {B}, 6] with sizes >= 1")
        self.last_draw = d
        x = x.contiguous()
        boxes, shift, gamma, taps, flip, smooth_fire, gamma_fire = self._upload(d, x.device)
        out = torch.empty((V, B, C, F, F, F), dtype=torch.float32, device=x.device)
        views = list(out.unbind(0))
        with torch.cuda.device(x.device):
            st = _lib.stream_ptr()
            _lib.check(lib.hct_crop_resize_area(x.data_ptr(), code, B, C, S, out.data_ptr(), F, V, boxes.data_ptr(), flip.data_ptr(),
                                                shift.data_ptr(), st), "hct_crop_resize_area")
            if bool(d["smooth_fire"].any()):  # out of place: the smoothed view 0 becomes a buffer of its own
                smoothed, tmp = torch.empty_like(views[0]), torch.empty_like(views[0])
                _lib.check(lib.hct_gaussian_smooth3d(views[0].data_ptr(), smoothed.data_ptr(), tmp.data_ptr(), B, C, F, taps.data_ptr(),
                                                     smooth_fire.data_ptr(), st), "hct_gaussian_smooth3d")
                views[0] = smoothed
            if bool(d["gamma_fire"].any()):
                n = C * F * F * F
                need = lib.hct_adjust_contrast_workspace_bytes(B, n)
                if self._workspace is None or self._workspace.numel() < need or self._workspace.device != x.device:
                    self._workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
                _lib.check(lib.hct_adjust_contrast(views[1].data_ptr(), B, n, gamma.data_ptr(), gamma_fire.data_ptr(),
                                                   self._workspace.data_ptr(), self._workspace.numel(), st), "hct_adjust_contrast")
        return views


class TransformedLoader:
    """`transform(batch)` for every batch of `base`."""

    def __init__(self, base, transform):
        self.base, self.transform = base, transform

    def __len__(self):
        return len(self.base)

    def __iter__(self):
        for x in self.base:
            yield self.transform(x)


class MultiCropLoader(TransformedLoader):
    """Volumes in, crop lists out: wraps a loader of [B, C, S, S, S] batches on the device (the cache's fp16, bf16 or fp32) and
    yields what the DINO engine consumes, a list of 2 + n tensors [B, C, F, F, F] made by `augment` (DeviceAugmentDINO3D)."""

    def __init__(self, base, augment):
        super().__init__(base, augment)
        self.augment = augment


# (centre, width) of the reference's three-channel input (transforms.py:130) and its one-channel window 40 +- 150 (:121-122)
HU_WINDOWS = {1: [(-110.0, 190.0)], 3: [(l - w // 2, l + w // 2) for l, w in ((40, 80), (80, 200), (600, 2800))]}


def window_hu(hu: torch.Tensor, in_channels: int = 1, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """HU volumes [B, 1, ...] (fp32 or fp16) -> windowed [B, in_channels, ...] in [0, 1]: the windowing step of
    `loading_transforms` (src/data/transforms.py:108-133) on the device, cast to the cache's fp16 by default."""
    from . import _lib
    lib = _lib.load()
    if not hu.is_cuda:
        raise _lib.HctError("window_hu runs on the GPU (libheadct_hip); no CPU fallback exists")
    if in_channels not in HU_WINDOWS:
        raise NotImplementedError(f"Channel size {in_channels} is not implemented.")
    if hu.dtype not in (torch.float32, torch.float16):
        hu = hu.float()
    hu = hu.contiguous()
    B, vox = hu.shape[0], hu[0].numel()
    lo = torch.tensor([w[0] for w in HU_WINDOWS[in_channels]], dtype=torch.float32, device=hu.device)
    hi = torch.tensor([w[1] for w in HU_WINDOWS[in_channels]], dtype=torch.float32, device=hu.device)
    out = torch.empty((B, in_channels) + tuple(hu.shape[2:]), dtype=out_dtype, device=hu.device)
    code = {torch.float16: _lib.HCT_F16, torch.float32: _lib.HCT_F32}
    with torch.cuda.device(hu.device):
        st = _lib.stream_ptr()
        _lib.check(lib.hct_hu_window(hu.data_ptr(), code[hu.dtype], out.data_ptr(), code[out_dtype], B, vox, in_channels,
                                     lo.data_ptr(), hi.data_ptr(), st), "hct_hu_window")
    return out


class SyntheticVolumes:
    """A fixed pool of `n_batches` pre-generated [B,C,S,S,S] batches on `device`, cycled (len == n_batches); `dtype` fp16 gives
    them in the persistent cache's format (the same fp32 draws, rounded)."""

    def __init__(self, n_batches, batch_size, in_chans, size, device, seed=0, dtype=torch.float32):
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        self.batches = [torch.rand(batch_size, in_chans, size, size, size, device=device, generator=gen).to(dtype) for _ in range(n_batches)]

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


# ---- real volumes: NIfTI -> cache item on the device ---------------------------------------------------------------------------------
PIPELINE_VERSION = 1  # part of every cache key: raise it when the arithmetic of load_volume changes

_NIFTI_CODE = {"uint8": 2, "int16": 4, "int32": 8, "float32": 16, "float64": 64, "int8": 256, "uint16": 512}
_window_tables = {}
_window_lock = threading.Lock()


def _windows_on(device, in_channels: int):
    key = (str(device), in_channels)
    with _window_lock:
        if key not in _window_tables:
            w = torch.tensor(HU_WINDOWS[in_channels], dtype=torch.float32)
            _window_tables[key] = (w[:, 0].contiguous().to(device), w[:, 1].contiguous().to(device))
        return _window_tables[key]


def _roi3(roi):
    roi = [int(r) for r in ([roi] * 3 if isinstance(roi, int) else roi)]
    if len(roi) != 3 or min(roi) < 1:
        raise ValueError(f"roi {roi} is not three positive sizes")
    return tuple(roi)


class DecodedVolume:
    """What the host makes of one file, ready to go up in one copy: `host`, a pinned byte buffer holding the raw voxels and the
    resampling tables at `offsets` (raw, base, weights), and the header-derived geometry (file shape ni, nj, nk; perm / flip to
    RAS; RAS shape d; resampled shape m)."""

    def __init__(self, path):
        self.path = str(path)
        raw, self.slope, self.inter, affine = nifti.read_nifti(path)
        nk, nj, ni = raw.shape
        self.file_shape, self.code = (ni, nj, nk), _NIFTI_CODE[raw.dtype.name]
        self.affine = affine
        self.perm, self.flip, zooms, _ = nifti.ras_axes(affine, self.file_shape)
        self.d = [self.file_shape[self.perm[o]] for o in range(3)]
        geom = [nifti.spacing_geometry(self.d[o], zooms[o]) for o in range(3)]
        self.m = [g[0] for g in geom]
        self.steps = [g[1] for g in geom]
        if max(self.d + self.m) > nifti.MAX_AXIS:
            raise ValueError(f"{path}: shape {tuple(self.d)} -> {tuple(self.m)} at 1 mm has an axis beyond {nifti.MAX_AXIS} voxels")
        tables = [nifti.bspline3_tables(self.d[o], self.m[o], geom[o][1]) for o in range(3)]
        parts = [raw.reshape(-1).view(np.uint8), np.concatenate([t[0] for t in tables]).view(np.uint8),
                 np.concatenate([t[1].reshape(-1) for t in tables]).view(np.uint8)]
        self.offsets, total = [], 0
        for p in parts:
            self.offsets.append(total)
            total += (p.size + 255) // 256 * 256
        self.host = torch.empty(total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        staged = self.host.numpy()
        for p, o in zip(parts, self.offsets):
            staged[o:o + p.size] = p


def run_loading_chain(dec: DecodedVolume, staged: torch.Tensor, roi, in_channels: int):
    """The device side of `load_volume` on the current stream: `staged` is `dec.host` on the device.  Returns (item fp16
    [in_channels, *roi], box int32 [8]: start[3], size[3], status, pad); the status is not looked at here."""
    from . import _lib
    lib = _lib.load()
    device, d, m = staged.device, dec.d, dec.m
    st = _lib.stream_ptr()
    c3 = _lib.c_int * 3
    ras = torch.empty(d, dtype=torch.float32, device=device)
    _lib.check(lib.hct_volume_to_ras(staged.data_ptr() + dec.offsets[0], dec.code, *dec.file_shape, c3(*dec.perm), c3(*[int(f) for f in dec.flip]),
                                     int(dec.slope is not None), float(dec.slope or 0.0), float(dec.inter or 0.0), ras.data_ptr(), st),
               "hct_volume_to_ras")
    iso = torch.empty(m, dtype=torch.float32, device=device)
    ws = torch.empty(max(16, lib.hct_bspline3_resample_workspace_bytes(*d, *m)), dtype=torch.uint8, device=device)
    _lib.check(lib.hct_bspline3_resample(ras.data_ptr(), *d, iso.data_ptr(), *m, staged.data_ptr() + dec.offsets[1],
                                         staged.data_ptr() + dec.offsets[2], ws.data_ptr(), ws.numel(), st), "hct_bspline3_resample")
    box = torch.empty(8, dtype=torch.int32, device=device)
    bws = torch.empty(max(16, lib.hct_foreground_bbox_workspace_bytes(*m)), dtype=torch.uint8, device=device)
    _lib.check(lib.hct_foreground_bbox(iso.data_ptr(), *m, box.data_ptr(), box.data_ptr() + 24, bws.data_ptr(), bws.numel(), st),
               "hct_foreground_bbox")
    lo, hi = _windows_on(device, in_channels)
    item = torch.empty((in_channels,) + tuple(roi), dtype=torch.float16, device=device)
    _lib.check(lib.hct_crop_window_resize_area(iso.data_ptr(), *m, box.data_ptr(), in_channels, lo.data_ptr(), hi.data_ptr(),
                                               item.data_ptr(), *roi, st), "hct_crop_window_resize_area")
    return item, box


def load_volume(path, roi, in_channels: int, device) -> torch.Tensor:
    """One NIfTI file -> the cache item, fp16 [in_channels, *roi] on `device`: `loading_transforms(roi, in_channels)`
    (src/data/transforms.py:108-178).  The host decodes the file and derives every shape from its header (DecodedVolume); raw
    voxels and the resampling tables go up in one pinned buffer by one asynchronous copy, and the launches of run_loading_chain
    (reorient + scale, three resampling passes, foreground box, crop + window + resize) make the item without waiting for the
    host.  The status word comes back with the result.  Raises ValueError on what the reader refuses, on an empty foreground and
    on axes beyond nifti.MAX_AXIS (before or after resampling)."""
    from . import _lib
    if in_channels not in HU_WINDOWS:
        raise NotImplementedError(f"Channel size {in_channels} is not implemented.")
    roi = _roi3(roi)
    dec = DecodedVolume(path)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HctError("load_volume runs on the GPU (libheadct_hip); no CPU fallback exists")
    with torch.cuda.device(device):
        item, box = run_loading_chain(dec, dec.host.to(device, non_blocking=True), roi, in_channels)
        status = torch.empty(8, dtype=torch.int32, pin_memory=True)
        status.copy_(box, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    if int(status[6]) != 0:
        raise ValueError(f"{path}: no voxel above 0 after resampling (empty foreground)")
    return item


class VolumeCache:
    """The persistent cache of the loading chain: one `.pt` per scan holding the plain fp16 tensor [in_channels, *roi], named by a
    hash of the path string, roi, channels and PIPELINE_VERSION, written under a temporary name and renamed, rebuilt when it fails
    to load.  (MONAI's PersistentDataset names its files by a hash of its pickled transforms: those files are neither read nor
    written.)  `loader(path, roi, in_channels, device)` makes a missing item; `load_volume` by default."""

    def __init__(self, cache_dir, roi, in_channels: int, loader=None):
        self.cache_dir, self.roi, self.in_channels = str(cache_dir), _roi3(roi), int(in_channels)
        self.loader = load_volume if loader is None else loader
        os.makedirs(self.cache_dir, exist_ok=True)

    def key(self, path) -> str:
        text = f"v{PIPELINE_VERSION}|{path}|{self.roi}|{self.in_channels}"
        return hashlib.sha256(text.encode()).hexdigest()[:32]

    def file_of(self, path) -> str:
        return os.path.join(self.cache_dir, self.key(path) + ".pt")

    def _read(self, file):
        try:
            t = torch.load(file, map_location="cpu", weights_only=True)
        except Exception:
            return None
        ok = isinstance(t, torch.Tensor) and t.dtype == torch.float16 and tuple(t.shape) == (self.in_channels,) + self.roi
        return t if ok else None

    def get(self, path, device) -> torch.Tensor:
        file = self.file_of(path)
        if os.path.exists(file):
            t = self._read(file)
            if t is not None:
                return t.to(device, non_blocking=True)
        item = self.loader(path, self.roi, self.in_channels, device)
        fd, tmp = tempfile.mkstemp(dir=self.cache_dir, suffix=".tmp")
        try:
            with os.fdopen(fd, "wb") as f:
                torch.save(item.detach().cpu().contiguous(), f)
            os.replace(tmp, file)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise
        return item


def read_image_paths(csv_file) -> list:
    """The `img_path` column of a CSV, in file order (the reference reads it with pandas, datasets.py:39-43)."""
    with open(csv_file, newline="") as f:
        reader = csv.DictReader(f)
        if reader.fieldnames is None or "img_path" not in reader.fieldnames:
            raise ValueError(f"{csv_file}: no img_path column (columns: {reader.fieldnames})")
        return [row["img_path"] for row in reader]


class PretrainVolumes:
    """PretrainDataset + DistributedSampler(shuffle=False) + ThreadDataLoader of the reference (src/data/datasets.py:21-137) for
    the device path: yields [B, C, S, S, S] fp16 batches on `device` from the scans of a CSV's `img_path` column, through
    `cache`.  This rank's indices are the sampler's (padded by wrapping so that every rank has as many), the last batch may be
    short, `num_workers` threads decode ahead of the consumer, and any error while loading prints the index and yields the
    all-zero placeholder (datasets.py:70-96)."""

    def __init__(self, csv_file, cache: VolumeCache, batch_size: int, device, rank: int = 0, world_size: int = 1, num_workers: int = 4):
        from torch.utils.data import DistributedSampler
        self.paths = read_image_paths(csv_file)
        if not self.paths:
            raise ValueError(f"{csv_file}: no rows")
        self.cache, self.batch_size, self.device = cache, int(batch_size), torch.device(device)
        self.size = _cubic(list(cache.roi), "MODEL.ROI")
        self.num_workers = max(1, int(num_workers))
        self.indices = list(DistributedSampler(range(len(self.paths)), num_replicas=world_size, rank=rank, shuffle=False))

    def __len__(self):
        return (len(self.indices) + self.batch_size - 1) // self.batch_size

    def item(self, idx: int) -> torch.Tensor:
        try:
            return self.cache.get(self.paths[idx], self.device)
        except Exception as e:
            print(f"Error loading index {idx}: {e}", flush=True)
            return torch.zeros((self.cache.in_channels,) + self.cache.roi, dtype=torch.float16, device=self.device)

    def __iter__(self):
        ahead = max(self.num_workers, self.batch_size) * 2
        with ThreadPoolExecutor(max_workers=self.num_workers) as pool:
            todo, pending, batch = iter(self.indices), deque(), []
            for idx in todo:
                pending.append(pool.submit(self.item, idx))
                if len(pending) >= ahead:
                    break
            while pending:
                batch.append(pending.popleft().result())
                nxt = next(todo, None)
                if nxt is not None:
                    pending.append(pool.submit(self.item, nxt))
                if len(batch) == self.batch_size or not pending:
                    yield torch.stack(batch)
                    batch = []


def pretrain_volume_loaders(config, device, rank, world_size, input_size: int, in_chans: int):
    """The three PretrainVolumes loaders (DATA.TRAIN / VAL / TEST_CSV_PATH) over one VolumeCache in DATA.CACHE_DIR."""
    csvs = []
    for key in ("TRAIN_CSV_PATH", "VAL_CSV_PATH", "TEST_CSV_PATH"):
        path = getattr(config.DATA, key)
        if not path or not os.path.isfile(path):
            raise FileNotFoundError(f"DATA.{key}: {path!r} is not a file (set it, or DATA.SYNTHETIC True to run without data)")
        csvs.append(path)
    roi = [int(r) for r in config.MODEL.ROI]
    if roi != [input_size] * 3 or config.MODEL.IN_CHANS != in_chans:
        raise ValueError(f"MODEL.ROI {roi} x MODEL.IN_CHANS {config.MODEL.IN_CHANS} is the cache item and must be what the model is "
                         f"built for ({[input_size] * 3} x {in_chans})")
    cache = VolumeCache(config.DATA.CACHE_DIR, roi, in_chans)
    return [PretrainVolumes(c, cache, config.DATA.BATCH_SIZE, device, rank, world_size, config.DATA.NUM_WORKERS) for c in csvs]


def get_pretrain_dataloaders(config, device, rank=0, world_size=1):
    """train / val / test loaders.  DATA.SYNTHETIC: pools of synthetic fp32 batches.  Otherwise the scans of the three CSVs through
    the cache, under `mae3d_transforms` (transforms.py:181-250): flips, shift and smoothing at prob 0.2 for train and val, the
    cast alone for test."""
    if not config.DATA.SYNTHETIC:
        train, val, test = pretrain_volume_loaders(config, device, rank, world_size, config.MAE.INPUT_SIZE, config.MAE.IN_CHANS)
        aug = lambda salt: DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=config.SEED + rank + salt, smooth_prob=0.2)
        cast = DeviceAugment(flip_prob=0.0, shift_offsets=0.0, shift_prob=0.0)
        return TransformedLoader(train, aug(0)), TransformedLoader(val, aug(1000)), TransformedLoader(test, cast)
    bs, n = config.DATA.BATCH_SIZE, config.DATA.SYNTHETIC_SAMPLES
    per_rank = max(1, n // max(1, world_size))
    nb = max(1, per_rank // bs)
    mk = lambda k, salt: SyntheticVolumes(k, bs, config.MAE.IN_CHANS, config.MAE.INPUT_SIZE, device, config.SEED + rank + salt)
    return mk(nb, 0), mk(max(1, nb // 4), 1000), mk(max(1, nb // 4), 2000)


class SyntheticLabelled:
    """`n_batches` labelled batches `(volume [B, C, S, S, S], target [B], names)` on the device for the downstream loop
    (DATA.SYNTHETIC): uniform noise in [0, 1), and for class c > 0 a brighter sub-cube (+0.5 * c) at a fixed corner, so the
    label can be learnt from the volume.  Labels alternate over the batch, so every class has samples in every batch."""

    reuses_batches = True  # the same tensors every epoch: a pass that works in place (mixup) takes a copy

    def __init__(self, n_batches, batch_size, in_chans, size, num_classes, device, seed=0):
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        e = max(1, size // 3)
        self.batches = []
        for i in range(n_batches):
            t = (torch.arange(batch_size, device=device) + i) % num_classes
            v = torch.rand(batch_size, in_chans, size, size, size, device=device, generator=gen)
            v[:, :, :e, :e, :e] += 0.5 * t.view(-1, 1, 1, 1, 1).float()
            self.batches.append((v, t, [f"synthetic_{i}_{b}" for b in range(batch_size)]))

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


class SyntheticMultiLabelled:
    """`n_batches` multi-label batches `(volume [B, C, S, S, S], target fp32 [B, T], names)` on the device for the downstream
    loop (DATA.SYNTHETIC with TRAIN.LABEL_NAMES): uniform noise in [0, 1), and for every label t that is set a brighter sub-cube
    (+0.5) of its own -- the eight corners in binary order of t (bit a of t = the far end of axis a), then the middles of six
    edges -- so each label can be learnt from the volume.  Sample b of batch i carries bit (b + i) % 4 of the four-bit pattern
    t + 1: the 14 patterns that are neither empty nor full, so every label has both values in any four consecutive samples and no
    two labels agree everywhere.  One entry in every 7 is marked missing (-1) -- entry t of the pool's row r where (3 r + t) % 7 == 3,
    so the gaps move from row to row at every T; the sub-cube follows the true label, the target hides it."""

    MAX_LABELS = 14
    reuses_batches = True  # as SyntheticLabelled

    def __init__(self, n_batches, batch_size, in_chans, size, num_labels, device, seed=0):
        if not 1 <= num_labels <= self.MAX_LABELS:
            raise ValueError(f"SyntheticMultiLabelled has {self.MAX_LABELS} sub-cubes and label patterns: {num_labels} labels are not supported")
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        e = max(1, size // 3)
        far, mid = size - e, (size - e) // 2
        self.boxes = []
        for t in range(num_labels):
            if t < 8:
                self.boxes.append(tuple(far if (t >> a) & 1 else 0 for a in range(3)))
            else:  # the middle of an edge along axis (t - 8) % 3, at the near (t < 11) or far corner of the other two axes
                k, side = (t - 8) % 3, far if t >= 11 else 0
                self.boxes.append(tuple(mid if a == k else side for a in range(3)))
        pattern = torch.arange(1, num_labels + 1, device=device)
        self.batches = []
        for i in range(n_batches):
            n = (torch.arange(batch_size, device=device) + i) % 4
            y = ((pattern.view(1, -1) >> n.view(-1, 1)) & 1).to(torch.float32)
            v = torch.rand(batch_size, in_chans, size, size, size, device=device, generator=gen)
            for t, (z0, y0, x0) in enumerate(self.boxes):
                v[:, :, z0:z0 + e, y0:y0 + e, x0:x0 + e] += 0.5 * y[:, t].view(-1, 1, 1, 1, 1)
            row = torch.arange(batch_size, device=device).view(-1, 1) + i * batch_size
            target = torch.where((3 * row + torch.arange(num_labels, device=device).view(1, -1)) % 7 == 3, torch.full_like(y, -1.0), y)
            self.batches.append((v, target, [f"synthetic_{i}_{b}" for b in range(batch_size)]))

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


class SyntheticSegmented:
    """`n_batches` segmentation batches `(volume [B, C, S, S, S], labels uint8 [B, S, S, S], names)` on the device for
    main_segmentation.py (DATA.SYNTHETIC): uniform noise in [0, 1) and, per sample, one axis-aligned box per foreground class c with
    intensity +0.5 * c and label c (a later class paints over an earlier one).  Position and extent come from the seeded generator:
    an extent between 2 voxels and half the side, anywhere in the volume, so some boxes straddle patch borders and some lie inside
    one patch.  With r the running index of the sample, class K - 1 is absent where r % 3 == 2, and where r % 4 == 3 a shell of
    ignore voxels (255), one voxel thick, surrounds each box.  `boxes[i][b]` lists (class, z0, z1, y0, y1, x0, x1) of sample b of
    batch i."""

    reuses_batches = True  # as SyntheticLabelled

    def __init__(self, n_batches, batch_size, in_chans, size, num_classes, device, seed=0):
        if not 2 <= num_classes <= 255:
            raise ValueError(f"SyntheticSegmented needs 2 .. 255 classes, not {num_classes}")
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        vgen = torch.Generator(device=device)
        vgen.manual_seed(seed)
        S, hi = size, max(2, size // 2)
        self.batches, self.boxes = [], []
        for i in range(n_batches):
            v = torch.rand(batch_size, in_chans, S, S, S, device=device, generator=vgen)
            y = torch.zeros(batch_size, S, S, S, dtype=torch.uint8)
            add = torch.zeros(batch_size, S, S, S)
            per_batch = []
            for b in range(batch_size):
                r = i * batch_size + b
                boxes = []
                for c in range(1, num_classes):
                    if c == num_classes - 1 and r % 3 == 2:
                        continue
                    ext = torch.randint(2, hi + 1, (3,), generator=gen)
                    lo = [int(torch.randint(0, S - int(e) + 1, (1,), generator=gen)) for e in ext]
                    z0, y0, x0 = lo
                    z1, y1, x1 = (l + int(e) for l, e in zip(lo, ext))
                    if r % 4 == 3:
                        y[b, max(z0 - 1, 0):z1 + 1, max(y0 - 1, 0):y1 + 1, max(x0 - 1, 0):x1 + 1] = 255
                    y[b, z0:z1, y0:y1, x0:x1] = c
                    add[b, z0:z1, y0:y1, x0:x1] = 0.5 * c
                    boxes.append((c, z0, z1, y0, y1, x0, x1))
                per_batch.append(boxes)
            v += add.to(device).unsqueeze(1)
            self.batches.append((v, y.to(device), [f"synthetic_{i}_{b}" for b in range(batch_size)]))
            self.boxes.append(per_batch)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


# ---- labelled volumes: fine-tuning on real scans ------------------------------------------------------------------------------------
# label name -> column position in the dataset's CSV (src/data/datasets.py:248-253; position 0 is img_path)
CLASS_MAPPINGS = {
    "nyu": ["cancer", "hydrocephalus", "edema", "dementia", "IPH", "IVH", "SDH", "EDH", "SAH", "ICH", "fracture"],
    "rsna": ["epidural", "intraparenchymal", "intraventricular", "subarachnoid", "subdural", "any"],
    "cq500": ["ICH", "IPH", "IVH", "SDH", "EDH", "SAH", "BleedLocation-Left", "BleedLocation-Right", "ChronicBleed", "Fracture",
              "CalvarialFracture", "OtherFracture", "MassEffect", "MidlineShift"],
}
CLASS_MAPPINGS["longisland"] = CLASS_MAPPINGS["nyu"]
TRAIN_SAMPLES_PER_RANK = 500  # the reference's hard-coded sample_size (datasets.py:298)

_log = logging.getLogger(__name__)


def label_column(dataset: str, label_name: str) -> int:
    """Column position of `label_name` in the CSVs of `dataset` (the reference's class_mapping, datasets.py:248-258)."""
    if dataset not in CLASS_MAPPINGS:
        raise ValueError(f"Unrecognized dataset: {dataset}")
    names = CLASS_MAPPINGS[dataset]
    if label_name not in names:  # the reference goes on with class_idx None and dies on an unbound name
        raise ValueError(f"label {label_name!r} is not one of dataset {dataset}'s: {names}")
    return names.index(label_name) + 1


def _as_label(text: str, csv_file, row: int) -> int:
    try:
        value = float(text)
        if value == int(value):
            return int(value)
    except (ValueError, OverflowError):
        pass
    raise ValueError(f"{csv_file}: row {row}: label {text!r} is not an integer")


def read_labels(csv_file, class_idx: int, label_name: str = None):
    """(paths, labels int64 [rows], label_of): the img_path column in file order, the label of every row taken from column
    POSITION class_idx as the reference's `iloc` takes it (datasets.py:276, 283), and the path -> label dictionary the dataset
    looks its targets up in, where the last of several rows with one path wins (`to_dict()`).  A header at that position that
    is not `label_name` is reported and accepted."""
    with open(csv_file, newline="") as f:
        rows = list(csv.reader(f))
    if not rows or "img_path" not in rows[0]:
        raise ValueError(f"{csv_file}: no img_path column (columns: {rows[0] if rows else None})")
    header, p = rows[0], rows[0].index("img_path")
    if not 0 <= class_idx < len(header):
        raise ValueError(f"{csv_file}: no column {class_idx} (columns: {header})")
    if label_name is not None and header[class_idx] != label_name:
        _log.warning(f"{csv_file}: column {class_idx} is {header[class_idx]!r}, not {label_name!r}; read by position, as the reference does")
    body = [r for r in rows[1:] if r]
    paths = [r[p] for r in body]
    labels = np.array([_as_label(r[class_idx], csv_file, i) for i, r in enumerate(body)], dtype=np.int64).reshape(-1)
    return paths, labels, dict(zip(paths, labels.tolist()))


def class_weights(labels, num_classes: int) -> torch.Tensor:
    """total / count_c per class, fp32 (datasets.py:278-281).  A class without a sample is refused (the reference makes inf of it)."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    if labels.size == 0 or labels.min() < 0 or labels.max() >= num_classes:
        raise ValueError(f"labels must be a non-empty set of values in [0, {num_classes})")
    counts = np.bincount(labels, minlength=num_classes)
    if (counts == 0).any():
        raise ValueError(f"class(es) {np.flatnonzero(counts == 0).tolist()} have no sample: counts {counts.tolist()}")
    return torch.tensor([1 / (c / labels.size) for c in counts], dtype=torch.float)


def expand_label_names(dataset: str, names) -> list:
    """TRAIN.LABEL_NAMES as a list of label names: ['all'] is every label of `dataset`, in CLASS_MAPPINGS order."""
    names = list(names)
    if names == ["all"]:
        if dataset not in CLASS_MAPPINGS:
            raise ValueError(f"Unrecognized dataset: {dataset}")
        return list(CLASS_MAPPINGS[dataset])
    return names


def _as_multilabel(text: str, csv_file, row: int, column: str) -> float:
    cell = text.strip()
    if cell == "" or cell.lower() == "nan":
        return -1.0
    try:
        value = float(cell)
    except ValueError:
        value = None
    if value is None or value not in (0.0, 1.0, -1.0):
        raise ValueError(f"{csv_file}: row {row}: column {column!r}: label {text!r} is not 0, 1 or missing (empty, nan, -1)")
    return value


def read_multilabels(csv_file, dataset: str, names):
    """(paths, labels fp32 [rows, T], label_of) for multi-label fine-tuning: the img_path column in file order and, per name of
    `names` (['all']: every label of the dataset), the column at the POSITION `label_column` gives, as `read_labels` takes its
    one.  A cell is 0, 1 or missing -- empty, `nan` in any case, or -1 -- and a missing one is stored as -1.0; anything else
    raises.  label_of maps a path to its row of labels; the last of several rows with one path wins."""
    names = expand_label_names(dataset, names)
    if not names:
        raise ValueError("read_multilabels: no label names")
    cols = [label_column(dataset, n) for n in names]
    with open(csv_file, newline="") as f:
        rows = list(csv.reader(f))
    if not rows or "img_path" not in rows[0]:
        raise ValueError(f"{csv_file}: no img_path column (columns: {rows[0] if rows else None})")
    header, p = rows[0], rows[0].index("img_path")
    for n, c in zip(names, cols):
        if c >= len(header):
            raise ValueError(f"{csv_file}: no column {c} for label {n!r} (columns: {header})")
        if header[c] != n:
            _log.warning(f"{csv_file}: column {c} is {header[c]!r}, not {n!r}; read by position, as the reference does")
    body = [r for r in rows[1:] if r]
    paths = [r[p] for r in body]
    labels = np.array([[_as_multilabel(r[c] if c < len(r) else "", csv_file, i, n) for n, c in zip(names, cols)] for i, r in enumerate(body)],
                      dtype=np.float32).reshape(len(body), len(names))
    return paths, labels, {path: labels[i] for i, path in enumerate(paths)}


def _label_counts(labels, names=None):
    """(valid rows, zeros, ones) per column of a [rows, T] label table whose negative entries are missing; a column without a 0
    or without a 1 among its valid entries is refused by name."""
    y = np.asarray(labels, dtype=np.float32)
    if y.ndim != 2 or y.shape[0] == 0 or y.shape[1] == 0:
        raise ValueError(f"labels must be a non-empty [rows, T] table, not {y.shape}")
    zeros, ones = (y == 0).sum(axis=0), (y == 1).sum(axis=0)
    for t in range(y.shape[1]):
        for value, count in ((0, zeros[t]), (1, ones[t])):
            if count == 0:
                what = f"label {names[t]!r} (column {t})" if names is not None else f"column {t}"
                raise ValueError(f"{what} has no entry with value {value} among its {int(zeros[t] + ones[t])} valid ones")
    return zeros + ones, zeros, ones


def multilabel_sample_weights(labels, names=None) -> np.ndarray:
    """Per-row sampling weights of a [rows, T] label table: weight_i = the mean, over the valid labels t of row i, of
    total_t / count_t(y_it), with total_t the valid rows of column t and count_t(v) those of value v; a row without a valid label
    gets 0.  Each ratio is `class_weights`' fp32 value, so that at T = 1 without gaps the weights are class_weights(y, 2)[y] value
    for value, and WeightedShardSampler draws the rows the single-label path draws under the same seed."""
    y = np.asarray(labels, dtype=np.float32)
    total, zeros, ones = _label_counts(y, names)
    ratio = np.stack([np.array([1 / (c / n) for c, n in zip(cnt.tolist(), total.tolist())], dtype=np.float32) for cnt in (zeros, ones)])
    per = np.where(y == 1, ratio[1][None, :], ratio[0][None, :]).astype(np.float64)
    valid = y >= 0
    k = valid.sum(axis=1)
    return np.where(k > 0, (per * valid).sum(axis=1) / np.maximum(k, 1), 0.0)


def multilabel_pos_weight(labels, sample_weights, names=None) -> torch.Tensor:
    """pos_weight_t = sum_i w_i [y_it = 0] / sum_i w_i [y_it = 1], fp32 [T]: the imbalance of label t that remains under draws
    with weights w (one sampler cannot balance several labels at once).  TRAIN.POS_WEIGHT 'balanced' passes it to the loss."""
    y = np.asarray(labels, dtype=np.float32)
    _label_counts(y, names)
    w = np.asarray(sample_weights, dtype=np.float64).reshape(-1, 1)
    if w.shape[0] != y.shape[0]:
        raise ValueError(f"{w.shape[0]} sample weights for {y.shape[0]} rows")
    neg, pos = (w * (y == 0)).sum(axis=0), (w * (y == 1)).sum(axis=0)
    if (pos <= 0).any() or (neg <= 0).any():
        raise ValueError(f"column(s) {np.flatnonzero((pos <= 0) | (neg <= 0)).tolist()} have no weight on one of the two values")
    return torch.tensor(neg / pos, dtype=torch.float32)


class WeightedShardSampler:
    """MONAI's DistributedWeightedRandomSampler as the reference uses it (datasets.py:298-305): this rank's shard is what
    DistributedSampler(shuffle=True, seed=0) gives at epoch 0 (padded by wrapping; `set_epoch` is never called, so it is the same
    every epoch), and every iteration draws `torch.multinomial(weights[shard], num_samples_per_rank, replacement=True)` and
    yields shard[draw].  MONAI is not installed here: this restates its documented behaviour.  The draws come from a generator
    of this sampler's own, seeded with `seed` (the loaders pass SEED + rank), not from the global one."""

    def __init__(self, weights, num_samples_per_rank: int = TRAIN_SAMPLES_PER_RANK, rank: int = 0, world_size: int = 1, seed: int = 0):
        from torch.utils.data import DistributedSampler
        self.weights = torch.as_tensor(np.asarray(weights), dtype=torch.double).reshape(-1)
        if self.weights.numel() == 0 or num_samples_per_rank < 1:
            raise ValueError("WeightedShardSampler needs weights and at least one sample per rank")
        self.num_samples_per_rank = int(num_samples_per_rank)
        self.shard = list(DistributedSampler(range(self.weights.numel()), num_replicas=world_size, rank=rank, shuffle=True, seed=0))
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(seed)

    def __len__(self):
        return self.num_samples_per_rank

    def __iter__(self):
        draw = torch.multinomial(self.weights[self.shard], self.num_samples_per_rank, True, generator=self.gen)
        return iter([self.shard[i] for i in draw.tolist()])


def fewshot_rows(csv_file, label_name: str, n: int, seed: int) -> list:
    """Row numbers of `df.groupby(label_name).sample(n, replace=True)` (datasets.py:394): n rows per value of the column NAMED
    label_name, drawn with replacement from the rows of that value, groups in ascending label order.  The draws come from numpy's
    Generator(seed); pandas' own order of draws is not reproduced."""
    with open(csv_file, newline="") as f:
        rows = list(csv.reader(f))
    if not rows or label_name not in rows[0]:
        raise ValueError(f"{csv_file}: no {label_name} column (columns: {rows[0] if rows else None})")
    if n < 1:
        raise ValueError(f"DATA.FEW_SHOTS {n}: at least one row per class is needed")
    c = rows[0].index(label_name)
    groups = {}
    for i, r in enumerate(r for r in rows[1:] if r):
        groups.setdefault(_as_label(r[c], csv_file, i), []).append(i)
    rng = np.random.default_rng(seed)
    return [groups[g][k] for g in sorted(groups) for k in rng.integers(0, len(groups[g]), n).tolist()]


def gather_augment(pool: torch.Tensor, slots: torch.Tensor, flip: torch.Tensor = None, shift: torch.Tensor = None, mat: torch.Tensor = None,
                   fire: torch.Tensor = None) -> torch.Tensor:
    """out[b] = shift[b] + flips(pool[slots[b]]) as fp32 [B, C, S, S, S], one launch (hct_gather_augment): what `DeviceAugment`
    makes of `pool.index_select(0, slots)`, bit for bit, without writing the gathered batch.  pool fp16 [n, C, S, S, S] on the
    GPU; slot -1 is the all-zero volume.  slots / flip / shift given on the CPU are checked (a slot outside [-1, n) raises) and
    uploaded; on the device they are taken as they are and the kernel reads nothing for a slot out of range.
    With `mat` [B, 12] (see `affine_matrices`; `fire` [B]: which samples take it, None = all) the launch is hct_affine_augment:
    what `DeviceAugment` with a RandAffine3D makes of the gathered batch, bit for bit.  A matrix given on the CPU with a
    non-finite entry raises."""
    from . import _lib
    lib = _lib.load()
    if not pool.is_cuda:
        raise _lib.HctError("gather_augment runs on the GPU (libheadct_hip); no CPU fallback exists")
    if pool.dtype != torch.float16 or pool.dim() != 5 or not pool.is_contiguous() or not (pool.shape[2] == pool.shape[3] == pool.shape[4]):
        raise ValueError(f"pool must be a contiguous fp16 [n, C, S, S, S] tensor, not {pool.dtype} {tuple(pool.shape)}")
    n, C, S = pool.shape[0], pool.shape[1], pool.shape[2]
    if not slots.is_cuda:
        if slots.numel() and (int(slots.min()) < -1 or int(slots.max()) >= n):
            raise ValueError(f"slots must lie in [-1, {n}): {slots.tolist()}")
    B = slots.numel()
    mat, fire = _checked_mat(mat, fire, B)
    on = lambda t, dt: None if t is None else t.to(device=pool.device, dtype=dt).contiguous()
    slots, flip, shift = on(slots, torch.int32), on(flip, torch.uint8), on(shift, torch.float32)
    if any(t is not None and t.numel() != B for t in (flip, shift)):
        raise ValueError("flip and shift need one entry per slot")
    out = torch.empty((B, C, S, S, S), dtype=torch.float32, device=pool.device)
    with torch.cuda.device(pool.device):
        if mat is None:
            _lib.check(lib.hct_gather_augment(pool.data_ptr(), slots.data_ptr(), out.data_ptr(), B, C, S, n, _lib.ptr(flip), _lib.ptr(shift),
                                              _lib.stream_ptr()), "hct_gather_augment")
        else:
            mat, fire = on(mat, torch.float32), on(fire, torch.uint8)
            _lib.check(lib.hct_affine_augment(pool.data_ptr(), _lib.HCT_F16, slots.data_ptr(), n, out.data_ptr(), B, C, S, mat.data_ptr(),
                                              _lib.ptr(fire), _lib.ptr(flip), _lib.ptr(shift), _lib.stream_ptr()), "hct_affine_augment")
    return out


class DevicePool:
    """The cache items of a loader's shard kept on the device: one fp16 tensor [capacity, C, S, S, S] and a path -> slot map with
    least-recently-used eviction.  `slots(paths)` returns the slot of every path as int32 [B] on the device (-1 = the placeholder:
    the item could not be loaded); what is not resident is fetched through `cache.get` on `num_workers` threads and copied into
    its slot on the current stream, so a batch gathered earlier on that stream has read its slots before they are overwritten.
    The slots of the batch being assembled are pinned against eviction, hence capacity >= batch_size."""

    def __init__(self, cache: VolumeCache, capacity: int, device, batch_size: int, num_workers: int = 4):
        if capacity < batch_size:
            raise ValueError(f"DevicePool capacity {capacity} is below the batch size {batch_size}: a batch could not be resident at once")
        self.cache, self.capacity, self.device = cache, int(capacity), torch.device(device)
        self.num_workers = max(1, int(num_workers))
        self.buf = torch.zeros((self.capacity, cache.in_channels) + cache.roi, dtype=torch.float16, device=self.device)
        self.slot_of = OrderedDict()  # path -> slot, least recently used first
        self.free = list(range(self.capacity - 1, -1, -1))
        self.hits = self.misses = self.evictions = 0

    @staticmethod
    def capacity_for(n: int, cache_num: int, cache_rate: float, budget_bytes: int, item_bytes: int) -> int:
        """min(n, CACHE_NUM if CACHE_NUM >= 0 else n, int(n * CACHE_RATE), budget_bytes // item_bytes): MONAI CacheDataset's rule
        (cache_num / cache_rate) and a byte budget."""
        return max(0, min(n, cache_num if cache_num >= 0 else n, int(n * cache_rate), int(budget_bytes) // int(item_bytes)))

    def _fetch(self, path, stream):
        try:
            if stream is None:
                return self.cache.get(path, self.device)
            with torch.cuda.stream(stream):  # the consumer's stream: the copy into the slot is ordered behind the upload
                return self.cache.get(path, self.device)
        except Exception as e:
            return e

    def slots_host(self, paths, on_error=None) -> list:
        """The slots as a list; `on_error(position in paths, exception)` is called for every path that failed to load."""
        pinned, missing = set(), []
        for p in dict.fromkeys(paths):
            if p in self.slot_of:
                self.slot_of.move_to_end(p)
                pinned.add(p)
                self.hits += 1
            else:
                missing.append(p)
        if len(pinned) + len(missing) > self.capacity:
            raise ValueError(f"{len(pinned) + len(missing)} different items in one batch exceed the pool's capacity {self.capacity}")
        failed = {}
        if missing:
            self.misses += len(missing)
            stream = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
            with ThreadPoolExecutor(max_workers=min(self.num_workers, len(missing))) as ex:
                items = list(ex.map(lambda p: self._fetch(p, stream), missing))
            for p, item in zip(missing, items):
                if isinstance(item, Exception):
                    failed[p] = item
                    continue
                if self.free:
                    slot = self.free.pop()
                else:  # evict the least recently used item that this batch does not use
                    victim = next(q for q in self.slot_of if q not in pinned)
                    slot = self.slot_of.pop(victim)
                    self.evictions += 1
                self.buf[slot].copy_(item, non_blocking=True)
                self.slot_of[p] = slot
                pinned.add(p)
        if on_error is not None:
            for i, p in enumerate(paths):
                if p in failed:
                    on_error(i, failed[p])
        return [-1 if p in failed else self.slot_of[p] for p in paths]

    def slots(self, paths, on_error=None) -> torch.Tensor:
        return _to_device(torch.tensor(self.slots_host(paths, on_error), dtype=torch.int32), self.device)


def _distributed_indices(n: int, rank: int, world_size: int, shuffle: bool) -> list:
    """DistributedSampler's indices at epoch 0 with seed 0 (padded by wrapping): the reference never calls `set_epoch`."""
    from torch.utils.data import DistributedSampler
    return list(DistributedSampler(range(n), num_replicas=world_size, rank=rank, shuffle=shuffle, seed=0))


class LabelledVolumes:
    """FinetuneDataset + sampler + ThreadDataLoader of the reference (src/data/datasets.py:186-361) for the device path: yields
    `(volume fp32 [B, C, S, S, S] on device, target int64 [B] on device, names list[str])`, what engine_downstream consumes
    (target fp32 [B, T] where the values of `label_of` are rows of T labels: multi-label mode, an addition of this build).
    `sampler` is iterated once per epoch for the row numbers of `paths` (a list, or a WeightedShardSampler that draws anew);
    the last batch may be short; len() is the number of batches.  `augment` is a DeviceAugment (vit_transforms: flips at 0.1,
    shift +-0.1 at 0.5 for train) or None for the cast alone (val, test).  With a `pool` a batch is one hct_gather_augment launch
    out of the device-resident items; without one the items come through `cache` on `num_workers` threads (the next batch is
    fetched while this one is consumed), are stacked and go through DeviceAugment: the same batches, bit for bit -- also where the
    DeviceAugment carries a RandAffine3D, whose matrices both paths hand to hct_affine_augment.  Any error
    while loading prints the index and yields the zero volume with label 0 and the name "None" (datasets.py:231-233).
    Every batch is a fresh tensor that the consumer may change in place (engine_downstream mixes training batches so: mixup,
    CutMix); a loader that yields tensors it keeps must set `reuses_batches = True`, as the synthetic loaders do."""

    def __init__(self, paths, label_of: dict, sampler, cache: VolumeCache, batch_size: int, device, augment: DeviceAugment = None,
                 pool: DevicePool = None, num_workers: int = 4):
        self.paths, self.label_of, self.sampler = list(paths), label_of, sampler
        if not self.paths:
            raise ValueError("LabelledVolumes: no rows")
        self.cache, self.batch_size, self.device = cache, int(batch_size), torch.device(device)
        self.size = _cubic(list(cache.roi), "MODEL.ROI")
        self.augment, self.pool, self.num_workers = augment, pool, max(1, int(num_workers))
        self._cast = DeviceAugment(flip_prob=0.0, shift_offsets=0.0, shift_prob=0.0)
        first = next(iter(label_of.values()), 0)
        self.num_labels = int(np.size(first)) if np.ndim(first) == 1 else 0  # rows of labels (read_multilabels): fp32 [B, T] targets

    def __len__(self):
        return (len(self.sampler) + self.batch_size - 1) // self.batch_size

    def _report(self, idx: int, e) -> None:
        print(f"Error loading index {idx}: {e}", flush=True)

    def _item(self, idx: int):
        try:
            return self.cache.get(self.paths[idx], self.device)
        except Exception as e:
            self._report(idx, e)
            return None

    def _finish(self, idxs, ok, volume):
        names = [self.paths[i] if good else "None" for i, good in zip(idxs, ok)]
        if self.num_labels:  # multi-label rows: a scan that failed to load is all-missing and adds nothing to loss or metrics
            gone = np.full(self.num_labels, -1.0, dtype=np.float32)
            rows = np.stack([np.asarray(self.label_of[self.paths[i]], dtype=np.float32) if good else gone for i, good in zip(idxs, ok)])
            return volume, _to_device(torch.from_numpy(rows), self.device), names
        target = torch.tensor([self.label_of[self.paths[i]] if good else 0 for i, good in zip(idxs, ok)], dtype=torch.int64)
        return volume, target.to(self.device), names

    def _pooled(self, idxs):
        slots = self.pool.slots_host([self.paths[i] for i in idxs], on_error=lambda pos, e: self._report(idxs[pos], e))
        flip, shift = self.augment.draw(len(idxs)) if self.augment is not None else (None, None)
        mat, fire = self.augment.draw_affine(len(idxs), self.size, flip) if self.augment is not None else (None, None)
        up = lambda t: None if t is None else _to_device(t, self.device)
        volume = gather_augment(self.pool.buf, up(torch.tensor(slots, dtype=torch.int32)), up(flip), up(shift), up(mat), up(fire))
        return self._finish(idxs, [s >= 0 for s in slots], volume)

    def _stacked(self, idxs, items):
        zero = None
        if any(t is None for t in items):
            zero = torch.zeros((self.cache.in_channels,) + self.cache.roi, dtype=torch.float16, device=self.device)
        x = torch.stack([zero if t is None else t for t in items])
        return self._finish(idxs, [t is not None for t in items], (self.augment or self._cast)(x))

    def __iter__(self):
        order = list(self.sampler)
        batches = [order[i:i + self.batch_size] for i in range(0, len(order), self.batch_size)]
        if self.pool is not None:
            for idxs in batches:
                yield self._pooled(idxs)
            return
        with ThreadPoolExecutor(max_workers=self.num_workers) as ex:
            ahead = [ex.submit(self._item, i) for i in batches[0]] if batches else []
            for k, idxs in enumerate(batches):
                items = [f.result() for f in ahead]
                ahead = [ex.submit(self._item, i) for i in batches[k + 1]] if k + 1 < len(batches) else []
                yield self._stacked(idxs, items)


def _to_device(t: torch.Tensor, device) -> torch.Tensor:
    """A small host table on the device by one asynchronous copy out of pinned memory (a pageable copy would make the host wait
    for the stream, and with it for the training step in front of this batch)."""
    if torch.device(device).type != "cuda":
        return t
    return t.pin_memory().to(device, non_blocking=True)


def _labelled_loaders(config, device, rank: int, world_size: int, few_shots: int):
    csvs = []
    for key in ("TRAIN_CSV_PATH", "VAL_CSV_PATH", "TEST_CSV_PATH"):
        path = getattr(config.DATA, key)
        if not path or not os.path.isfile(path):
            raise FileNotFoundError(f"DATA.{key}: {path!r} is not a file (set it, or DATA.SYNTHETIC True to run without data)")
        csvs.append(path)
    roi, in_chans = [int(r) for r in config.MODEL.ROI], config.VIT.IN_CHANS
    if roi != [config.VIT.INPUT_SIZE] * 3 or config.MODEL.IN_CHANS != in_chans:
        raise ValueError(f"MODEL.ROI {roi} x MODEL.IN_CHANS {config.MODEL.IN_CHANS} is the cache item and must be what the model is "
                         f"built for ({[config.VIT.INPUT_SIZE] * 3} x {in_chans})")
    names = expand_label_names(config.DATA.DATASET, config.TRAIN.LABEL_NAMES)
    if names and few_shots != -1:
        raise ValueError(f"DATA.FEW_SHOTS {few_shots} with TRAIN.LABEL_NAMES: few-shot sampling is per class of one label; "
                         "set DATA.FEW_SHOTS -1 or name a single TRAIN.LABEL_NAME")
    if names:
        (p_train, y_train, d_train), (p_val, _, d_val), (p_test, _, d_test) = [read_multilabels(c, config.DATA.DATASET, names) for c in csvs]
    else:
        class_idx = label_column(config.DATA.DATASET, config.TRAIN.LABEL_NAME)
        (p_train, y_train, d_train), (p_val, _, d_val), (p_test, _, d_test) = [read_labels(c, class_idx, config.TRAIN.LABEL_NAME) for c in csvs]
    for c, p in zip(csvs, (p_train, p_val, p_test)):
        if not p:
            raise ValueError(f"{c}: no rows")
    bs, workers, seed = config.DATA.BATCH_SIZE, config.DATA.NUM_WORKERS, config.SEED + rank
    if names:  # the fourth value is the loss's pos_weight [T] (TRAIN.POS_WEIGHT 'balanced') or None
        if config.TRAIN.POS_WEIGHT not in ("none", "balanced"):
            raise ValueError(f"TRAIN.POS_WEIGHT {config.TRAIN.POS_WEIGHT!r} is not 'none' or 'balanced'")
        row_weights = multilabel_sample_weights(y_train, names)
        weights = multilabel_pos_weight(y_train, row_weights, names) if config.TRAIN.POS_WEIGHT == "balanced" else None
        sampler = WeightedShardSampler(row_weights, config.DATA.TRAIN_SAMPLES_PER_RANK, rank, world_size, seed)
        shard = sampler.shard
    elif few_shots == -1:
        weights = class_weights(y_train, config.DATA.NUM_CLASSES)
        sampler = WeightedShardSampler(weights.double().numpy()[y_train], config.DATA.TRAIN_SAMPLES_PER_RANK, rank, world_size, seed)
        shard = sampler.shard
    else:  # the few-shot table replaces the train CSV; the reference computes no class weights for it
        weights = None
        p_train = [p_train[r] for r in fewshot_rows(csvs[0], config.TRAIN.LABEL_NAME, few_shots, config.SEED)]
        sampler = shard = _distributed_indices(len(p_train), rank, world_size, True)
    s_val, s_test = _distributed_indices(len(p_val), rank, world_size, False), _distributed_indices(len(p_test), rank, world_size, False)
    cache = VolumeCache(config.DATA.CACHE_DIR, roi, in_chans)
    # one pool for the three loaders of this rank, sized for the different scans they touch
    n = len({p_train[i] for i in shard} | {p_val[i] for i in s_val} | {p_test[i] for i in s_test})
    item_bytes = 2 * in_chans * roi[0] * roi[1] * roi[2]
    capacity = DevicePool.capacity_for(n, config.DATA.CACHE_NUM, config.DATA.CACHE_RATE, int(config.DATA.DEVICE_POOL_GB * 2 ** 30), item_bytes)
    # a batch holds at most min(batch size, n) different scans: that many slots must exist
    pool = DevicePool(cache, capacity, device, min(bs, n), workers) if config.DATA.DEVICE_POOL_GB > 0 else None
    t = config.TRAIN
    affine = None  # AFFINE_PROB 0: the loader, its draws and its launches are those of a build without the affine
    if t.AFFINE_PROB > 0:
        affine = RandAffine3D(t.AFFINE_ROTATE, t.AFFINE_SCALE, t.AFFINE_TRANSLATE, t.AFFINE_PROB, t.AFFINE_ISOTROPIC, seed=seed)
    augment = DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=seed, affine=affine)
    mk = lambda p, d, s, a: LabelledVolumes(p, d, s, cache, bs, device, a, pool, workers)
    return mk(p_train, d_train, sampler, augment), mk(p_val, d_val, s_val, None), mk(p_test, d_test, s_test, None), weights


def get_finetune_dataloaders(config, device, rank=0, world_size=1):
    """(train, val, test, class weights) of the reference's get_finetune_dataloaders (datasets.py:236-361): labels of
    DATA.DATASET / TRAIN.LABEL_NAME out of the three CSVs, train drawn class-balanced with replacement
    (DATA.TRAIN_SAMPLES_PER_RANK per epoch) under vit_transforms' flips and shift, val and test in file order with the cast
    alone; the items live in a DevicePool of DATA.CACHE_NUM / CACHE_RATE / DEVICE_POOL_GB (0 GB: no pool)."""
    return _labelled_loaders(config, device, rank, world_size, -1)


def get_fewshots_dataloaders(config, device, rank=0, world_size=1):
    """(train, val, test, None) of the reference's get_fewshots_dataloaders (datasets.py:364-477): DATA.FEW_SHOTS rows per class
    of the train CSV (`fewshot_rows`, seeded with SEED), shuffled once by DistributedSampler; val and test as above."""
    if config.DATA.FEW_SHOTS < 1:
        raise ValueError(f"DATA.FEW_SHOTS {config.DATA.FEW_SHOTS}: at least one row per class is needed")
    return _labelled_loaders(config, device, rank, world_size, config.DATA.FEW_SHOTS)


# ---- segmentation: image / mask pairs (an addition of this build) -------------------------------------------------------------------
def read_segmentation_paths(csv_file) -> list:
    """[(img_path, seg_path)] of a CSV with those two columns, in file order."""
    with open(csv_file, newline="") as f:
        reader = csv.DictReader(f)
        cols = reader.fieldnames
        if cols is None or "img_path" not in cols or "seg_path" not in cols:
            raise ValueError(f"{csv_file}: the columns img_path and seg_path are needed (columns: {cols})")
        return [(row["img_path"], row["seg_path"]) for row in reader]


def nearest_tables(d, m, steps) -> np.ndarray:
    """int32 [m0 + m1 + m2], the three per-axis tables of hct_label_to_item one after the other: resampled voxel j of an axis shows
    mask voxel clamp(floor(j * step + 0.5), 0, d - 1), `step` being nifti.spacing_geometry's (output voxel j reads input coordinate
    j * step)."""
    return np.concatenate([np.clip(np.floor(np.arange(m[a], dtype=np.float64) * steps[a] + 0.5), 0, d[a] - 1).astype(np.int32) for a in range(3)])


def load_label_volume(seg_path, dec: DecodedVolume, box: torch.Tensor, roi, device) -> torch.Tensor:
    """The label item uint8 [*roi] on `device` of the mask file `seg_path`, seen through the geometry of its image: `dec` is the image's
    DecodedVolume and `box` the device words its loading chain left (run_loading_chain).  The mask must have the image's shape and
    affine (1e-3 per entry: the two files come from one export).  hct_volume_to_ras reorients the mask, hct_label_to_item takes the
    nearest mask voxel under the centre of every cell of the image's crop + resize; no value is interpolated.  Raises ValueError
    on a mask of another grid and on a value that is no integer in [0, 254]."""
    from . import _lib
    lib = _lib.load()
    roi = _roi3(roi)
    raw, slope, inter, affine = nifti.read_nifti(seg_path)
    nk, nj, ni = raw.shape
    if (ni, nj, nk) != tuple(dec.file_shape):
        raise ValueError(f"{seg_path}: mask shape {(ni, nj, nk)} differs from the image's {tuple(dec.file_shape)} ({dec.path})")
    if float(np.abs(np.asarray(affine) - np.asarray(dec.affine)).max()) > 1e-3:
        raise ValueError(f"{seg_path}: mask affine differs from the image's ({dec.path})")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HctError("load_label_volume runs on the GPU (libheadct_hip); no CPU fallback exists")
    c3 = _lib.c_int * 3
    with torch.cuda.device(device):
        st = _lib.stream_ptr()
        staged = _to_device(torch.from_numpy(np.ascontiguousarray(raw).reshape(-1).view(np.uint8).copy()), device)
        near = _to_device(torch.from_numpy(nearest_tables(dec.d, dec.m, dec.steps)), device)
        ras = torch.empty(dec.d, dtype=torch.float32, device=device)
        _lib.check(lib.hct_volume_to_ras(staged.data_ptr(), _NIFTI_CODE[raw.dtype.name], *dec.file_shape, c3(*dec.perm), c3(*[int(f) for f in dec.flip]),
                                         int(slope is not None), float(slope or 0.0), float(inter or 0.0), ras.data_ptr(), st), "hct_volume_to_ras")
        out = torch.empty(roi, dtype=torch.uint8, device=device)
        status_d = torch.empty(1, dtype=torch.int32, device=device)
        _lib.check(lib.hct_label_to_item(ras.data_ptr(), *dec.d, near.data_ptr(), *dec.m, box.data_ptr(), out.data_ptr(), *roi, status_d.data_ptr(), st),
                   "hct_label_to_item")
        status = torch.empty(1, dtype=torch.int32, pin_memory=True)
        status.copy_(status_d, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    if int(status[0]) != 0:
        raise ValueError(f"{seg_path}: a mask value is no integer in [0, 254]")
    return out


def load_segmentation_pair(img_path, seg_path, roi, in_channels: int, device):
    """(image item fp16 [in_channels, *roi], label item uint8 [*roi]) of one scan: the image through run_loading_chain, unchanged,
    the mask through load_label_volume with the box that chain left on the device."""
    from . import _lib
    roi = _roi3(roi)
    dec = DecodedVolume(img_path)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HctError("load_segmentation_pair runs on the GPU (libheadct_hip); no CPU fallback exists")
    with torch.cuda.device(device):
        item, box = run_loading_chain(dec, dec.host.to(device, non_blocking=True), roi, in_channels)
        status = torch.empty(8, dtype=torch.int32, pin_memory=True)
        status.copy_(box, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        if int(status[6]) != 0:
            raise ValueError(f"{img_path}: no voxel above 0 after resampling (empty foreground)")
        return item, load_label_volume(seg_path, dec, box, roi, device)


class LabelCache:
    """The label twin of VolumeCache, in the same directory: one `.pt` per scan holding the uint8 tensor [*roi], named by a hash of
    what names the volume's file plus the mask path.  A missing item is made by `load_segmentation_pair` (the image's chain runs
    again for its foreground box; its item is not rewritten)."""

    def __init__(self, cache_dir, roi, in_channels: int):
        self.cache_dir, self.roi, self.in_channels = str(cache_dir), _roi3(roi), int(in_channels)
        os.makedirs(self.cache_dir, exist_ok=True)

    def key(self, img_path, seg_path) -> str:
        text = f"v{PIPELINE_VERSION}|{img_path}|{self.roi}|{self.in_channels}|seg|{seg_path}"
        return hashlib.sha256(text.encode()).hexdigest()[:32]

    def file_of(self, img_path, seg_path) -> str:
        return os.path.join(self.cache_dir, self.key(img_path, seg_path) + ".pt")

    def get(self, img_path, seg_path, device) -> torch.Tensor:
        file = self.file_of(img_path, seg_path)
        if os.path.exists(file):
            try:
                t = torch.load(file, map_location="cpu", weights_only=True)
            except Exception:
                t = None
            if isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and tuple(t.shape) == self.roi:
                return t.to(device, non_blocking=True)
        _, lab = load_segmentation_pair(img_path, seg_path, self.roi, self.in_channels, device)
        fd, tmp = tempfile.mkstemp(dir=self.cache_dir, suffix=".tmp")
        try:
            with os.fdopen(fd, "wb") as f:
                torch.save(lab.detach().cpu().contiguous(), f)
            os.replace(tmp, file)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise
        return lab


AFFINE_OUTSIDE = {"background": 0, "ignore": 255}  # SEG.AFFINE_OUTSIDE: the label where the resampled scan is zero-padded


def augment_segmentation_batch(x: torch.Tensor, labels: torch.Tensor, augment: DeviceAugment = None, failed=None, outside: int = 0):
    """The train-time transform of one segmentation batch, scans and masks under the SAME draws: x [B, C, S, S, S] stacked on the
    device (fp16, the cache format; bf16 and fp32 pass too), labels uint8 [B, S, S, S] -> (volume fp32, labels uint8, draws) with
    draws = {flip uint8 [B], mat fp32 [B, 12] or None, fire uint8 [B] or None} on the CPU.  Draw order is LabelledVolumes':
    `augment.draw(B)`, then `augment.draw_affine(B, S, flip)`.  Without an affine on `augment` (or without `augment`: no flips, no
    shift) the launches are hct_augment_volume and hct_gather_flip_labels, and nothing else is drawn.  With one, the scans go
    through hct_affine_augment and the masks through hct_affine_labels with the same mat, fire and flip tensors; `outside` is the
    label where a firing sample reads beyond the volume.  `failed` [B] (booleans or None): scans that did not load -- their fire
    byte is forced to 0, so a zero volume with all-ignore labels stays exactly that."""
    from . import _lib
    from .segmentation import affine_labels, gather_flip_labels
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.HctError("augment_segmentation_batch runs on the GPU (libheadct_hip); no CPU fallback exists")
    B, C, S, dev = x.shape[0], x.shape[1], x.shape[2], x.device
    if augment is not None:
        flip, shift = augment.draw(B)
        mat, fire = augment.draw_affine(B, S, flip)
    else:
        flip, shift, mat, fire = torch.zeros(B, dtype=torch.uint8), torch.zeros(B), None, None
    if fire is not None and failed is not None:
        fire = fire & ~torch.as_tensor(list(failed), dtype=torch.bool).to(torch.uint8) & 1
    draws = {"flip": flip.clone(), "mat": None if mat is None else mat.clone(), "fire": None if fire is None else fire.clone()}
    flip_d, shift_d = _to_device(flip, dev), _to_device(shift.to(torch.float32), dev)
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    if mat is None:
        x = x.contiguous()
        code = {torch.float16: _lib.HCT_F16, torch.bfloat16: _lib.HCT_BF16, torch.float32: _lib.HCT_F32}[x.dtype]
        out = torch.empty(x.shape, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.hct_augment_volume(x.data_ptr(), code, out.data_ptr(), B, C, S, flip_d.data_ptr(), shift_d.data_ptr(),
                                              _lib.stream_ptr()), "hct_augment_volume")
        return out, gather_flip_labels(labels, rows, flip_d), draws
    mat_d, fire_d = _to_device(mat, dev), _to_device(fire, dev)
    with torch.cuda.device(dev):
        out = affine_augment(x, mat_d, fire_d, flip_d, shift_d)
    return out, affine_labels(labels, rows, mat_d, fire_d, flip_d, outside), draws


class AugmentedSegmented:
    """A thin train loader over fixed segmentation batches (SyntheticSegmented): every batch goes through
    `augment_segmentation_batch` anew, so the batches it yields are fresh tensors and the fixed ones stay as they are."""

    def __init__(self, batches, augment: DeviceAugment, outside: int = 0):
        self.batches, self.augment, self.outside = batches, augment, int(outside)
        self.last_draws = None

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for v, y, names in self.batches:
            out, labels, self.last_draws = augment_segmentation_batch(v, y, self.augment, None, self.outside)
            yield out, labels, names


class SegmentedVolumes:
    """Loader of segmentation fine-tuning: yields (volume fp32 [B, C, S, S, S], labels uint8 [B, S, S, S], names) on `device` from
    image / mask pairs in the order `order` gives (DistributedSampler's: shuffled for train, file order for val and test).  Volumes
    come through `cache` (VolumeCache) and the flips and shift of `augment` (a DeviceAugment; None: the plain cast), labels through
    `label_cache` and hct_gather_flip_labels with the SAME flips: one `augment.draw` serves both launches.  Where `augment` carries a
    RandAffine3D, the samples that fire are resampled -- scans trilinear through hct_affine_augment, masks nearest neighbour through
    hct_affine_labels with the same matrices, `affine_outside` (0 or 255) the label beyond the volume (`augment_segmentation_batch`).
    A scan that fails to load yields the zero volume with all-ignore labels and the name "None", and never fires.  `last_flip`,
    `last_mat` and `last_fire` keep the draws of the last batch."""

    def __init__(self, pairs, order, cache: VolumeCache, label_cache: LabelCache, batch_size: int, device, augment: DeviceAugment = None,
                 num_workers: int = 4, affine_outside: int = 0):
        self.pairs, self.order, self.cache, self.label_cache = list(pairs), list(order), cache, label_cache
        self.batch_size, self.device, self.augment, self.num_workers = int(batch_size), torch.device(device), augment, max(1, int(num_workers))
        self.size = _cubic(list(cache.roi), "MODEL.ROI")
        self.affine_outside = int(affine_outside)
        self.last_flip = self.last_mat = self.last_fire = None

    def __len__(self):
        return (len(self.order) + self.batch_size - 1) // self.batch_size

    def _item(self, idx: int):
        img, seg = self.pairs[idx]
        try:
            return self.cache.get(img, self.device), self.label_cache.get(img, seg, self.device)
        except Exception as e:
            print(f"Error loading index {idx}: {e}", flush=True)
            return None

    def _stacked(self, idxs, items):
        from .segmentation import IGNORE_INDEX
        C, dev = self.cache.in_channels, self.device
        zero = torch.zeros((C,) + self.cache.roi, dtype=torch.float16, device=dev)
        gone = torch.full(self.cache.roi, IGNORE_INDEX, dtype=torch.uint8, device=dev)
        x = torch.stack([zero if t is None else t[0] for t in items]).contiguous()
        labs = torch.stack([gone if t is None else t[1] for t in items])
        out, labels, draws = augment_segmentation_batch(x, labs, self.augment, [t is None for t in items], self.affine_outside)
        self.last_flip, self.last_mat, self.last_fire = draws["flip"], draws["mat"], draws["fire"]
        names = [self.pairs[i][0] if t is not None else "None" for i, t in zip(idxs, items)]
        return out, labels, names

    def __iter__(self):
        batches = [self.order[i:i + self.batch_size] for i in range(0, len(self.order), self.batch_size)]
        with ThreadPoolExecutor(max_workers=self.num_workers) as ex:
            ahead = [ex.submit(self._item, i) for i in batches[0]] if batches else []
            for k, idxs in enumerate(batches):
                items = [f.result() for f in ahead]
                ahead = [ex.submit(self._item, i) for i in batches[k + 1]] if k + 1 < len(batches) else []
                yield self._stacked(idxs, items)


def get_segmentation_dataloaders(config, device, rank=0, world_size=1):
    """(train, val, test) SegmentedVolumes over the img_path / seg_path pairs of DATA.TRAIN / VAL / TEST_CSV_PATH: train shuffled once
    by DistributedSampler under flips and shift (vit_transforms' flips at 0.1, shift 0.1 at 0.5), val and test in file order with
    the cast alone; volumes and labels cached side by side in DATA.CACHE_DIR.  SEG.AFFINE_PROB > 0 adds a RandAffine3D seeded
    SEED + rank to the train loader alone (`segmentation_affine`); TRAIN.AFFINE_PROB stays refused here."""
    csvs = []
    for key in ("TRAIN_CSV_PATH", "VAL_CSV_PATH", "TEST_CSV_PATH"):
        path = getattr(config.DATA, key)
        if not path or not os.path.isfile(path):
            raise FileNotFoundError(f"DATA.{key}: {path!r} is not a file (set it, or DATA.SYNTHETIC True to run without data)")
        csvs.append(path)
    roi, in_chans = [int(r) for r in config.MODEL.ROI], config.VIT.IN_CHANS
    if roi != [config.VIT.INPUT_SIZE] * 3 or config.MODEL.IN_CHANS != in_chans:
        raise ValueError(f"MODEL.ROI {roi} x MODEL.IN_CHANS {config.MODEL.IN_CHANS} is the cache item and must be what the model is "
                         f"built for ({[config.VIT.INPUT_SIZE] * 3} x {in_chans})")
    if config.TRAIN.AFFINE_PROB > 0:
        raise ValueError(f"TRAIN.AFFINE_PROB {config.TRAIN.AFFINE_PROB} in segmentation mode: the switch of this mode is SEG.AFFINE_PROB "
                         "(the masks are resampled with the scans)")
    pairs = [read_segmentation_paths(c) for c in csvs]
    for c, p in zip(csvs, pairs):
        if not p:
            raise ValueError(f"{c}: no rows")
    cache, labels = VolumeCache(config.DATA.CACHE_DIR, roi, in_chans), LabelCache(config.DATA.CACHE_DIR, roi, in_chans)
    bs, workers, seed = config.DATA.BATCH_SIZE, config.DATA.NUM_WORKERS, config.SEED + rank
    affine, outside = segmentation_affine(config, seed)  # SEG.AFFINE_PROB 0: the loader, its draws and its launches are those of a build without it
    augment = DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=seed, affine=affine)
    mk = lambda p, shuffle, a: SegmentedVolumes(p, _distributed_indices(len(p), rank, world_size, shuffle), cache, labels, bs, device, a, workers,
                                                outside)
    return mk(pairs[0], True, augment), mk(pairs[1], False, None), mk(pairs[2], False, None)


def segmentation_affine(config, seed: int):
    """(RandAffine3D or None, the label byte beyond the volume) of SEG.AFFINE_PROB / SEG.AFFINE_OUTSIDE; the magnitudes are
    TRAIN.AFFINE_ROTATE / AFFINE_SCALE / AFFINE_TRANSLATE / AFFINE_ISOTROPIC, as in classification fine-tuning."""
    t, g = config.TRAIN, config.SEG
    outside = AFFINE_OUTSIDE[g.AFFINE_OUTSIDE]
    if g.AFFINE_PROB <= 0:
        return None, outside
    return RandAffine3D(t.AFFINE_ROTATE, t.AFFINE_SCALE, t.AFFINE_TRANSLATE, g.AFFINE_PROB, t.AFFINE_ISOTROPIC, seed=seed), outside
