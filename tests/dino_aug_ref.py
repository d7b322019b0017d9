"""CPU restatement of DataAugmentationDINO3D (src/data/transforms.py:39-105) with every random draw explicit, the yardstick of
tests/test_dino_aug_*.py.  It works the way the reference's MONAI chain does -- on a really materialised, zero-padded field and
in FIELD coordinates -- so the device path's coordinate arithmetic (boxes in input coordinates, no field) is checked against an
independent statement of it.  MONAI is not installed here: ResizeWithPadOrCrop's offsets, RandSpatialCrop's distributions,
Resize's default mode ("area") and AdjustContrast's formula are stated from knowledge of MONAI 1.2 / 1.3, and parity with MONAI
itself stays unpinned."""
import math

import torch
import torch.nn.functional as F

from oracle import mae_oracle as O


def pad_or_crop(vol: torch.Tensor, field: int) -> torch.Tensor:
    """ResizeWithPadOrCrop(field) on [C, S, S, S]: centre crop from S // 2 - field // 2 where larger, else zero padding with
    (field - S) // 2 voxels in front and the rest behind."""
    S = vol.shape[-1]
    if S > field:
        a = S // 2 - field // 2
        return vol[:, a:a + field, a:a + field, a:a + field]
    lo = (field - S) // 2
    hi = field - S - lo
    return F.pad(vol, (lo, hi, lo, hi, lo, hi))


def center_crop(vol: torch.Tensor, size: int) -> torch.Tensor:
    """CenterSpatialCrop(size): from extent // 2 - size // 2."""
    a = vol.shape[-1] // 2 - size // 2
    return vol[:, a:a + size, a:a + size, a:a + size]


def crop_resize(vol: torch.Tensor, box, final: int, field: int = 224, local_field=None, flip: int = 0, shift: float = 0.0) -> torch.Tensor:
    """Steps 1-6 for one view of one sample.  vol [C, S, S, S] of any float dtype; box = (start[3], size[3]) in the coordinates
    of the field the crop is cut from: the `field`^3 one, or, with `local_field`, its centre crop.  flip: bit a = spatial axis a;
    shift: the drawn offset (0 = did not fire)."""
    f = pad_or_crop(vol.to(torch.float32), field)
    if local_field is not None:
        f = center_crop(f, local_field)
    (x, y, z), (nx, ny, nz) = box[:3], box[3:]
    assert 0 <= x and x + nx <= f.shape[1] and 0 <= y and y + ny <= f.shape[2] and 0 <= z and z + nz <= f.shape[3], "box outside its field"
    crop = f[:, x:x + nx, y:y + ny, z:z + nz]
    out = F.interpolate(crop.unsqueeze(0), size=(final,) * 3, mode="area")[0]
    dims = [1 + a for a in range(3) if flip & (1 << a)]
    if dims:
        out = torch.flip(out, dims)
    return out + torch.tensor(shift, dtype=torch.float32)


def area_matrix(n: int, final: int) -> torch.Tensor:
    """[final, n] averaging matrix of the area resize along one axis: row i averages inputs [floor(i n / F), ceil((i + 1) n / F))."""
    m = torch.zeros(final, n, dtype=torch.float64)
    for i in range(final):
        lo, hi = (i * n) // final, -((-(i + 1) * n) // final)
        m[i, lo:hi] = 1.0 / (hi - lo)
    return m


def area_windows(n: int, final: int, start: int, flip: bool = False):
    """Per output index of an axis: the window [lo, hi) in the coordinates `start` is given in, mirrored under a flip."""
    w = [(start + (i * n) // final, start + math.ceil((i + 1) * n / final)) for i in range(final)]
    return w[::-1] if flip else w


def adjust_contrast(crop: torch.Tensor, gamma: float) -> torch.Tensor:
    """AdjustContrast on one crop [C, F, F, F] fp32, min / max over the whole crop, evaluated in fp64 and rounded to fp32:
    ((img - mn) / (mx - mn + 1e-7)) ** gamma * (mx - mn) + mn."""
    x = crop.to(torch.float64)
    mn, mx = x.min(), x.max()
    return (((x - mn) / (mx - mn + 1e-7)) ** float(gamma) * (mx - mn) + mn).to(torch.float32)


def adjust_contrast_fp32(crop: torch.Tensor, gamma: float) -> torch.Tensor:
    """The same formula in fp32 on the CPU (what MONAI itself computes): its distance from the fp64 value is the yardstick for
    the kernel's."""
    mn, mx = crop.min(), crop.max()
    return ((crop - mn) / (mx - mn + torch.tensor(1e-7))) ** torch.tensor(gamma, dtype=torch.float32) * (mx - mn) + mn


def views(vol_batch: torch.Tensor, field_boxes, draw: dict, final: int, field: int = 224, local_field: int = 192):
    """The whole chain on a batch [B, C, S, S, S] for explicit draws: `field_boxes` [V][B][6] in field coordinates (global views:
    of `field`, local views: of `local_field`), the rest as DeviceAugmentDINO3D.draw returns it.  List of V tensors [B, C, F, F, F]."""
    V, B = len(field_boxes), vol_batch.shape[0]
    out = []
    for v in range(V):
        crops = torch.stack([crop_resize(vol_batch[b], [int(t) for t in field_boxes[v][b]], final, field, None if v < 2 else local_field,
                                         int(draw["flip"][v][b]), float(draw["shift"][v][b])) for b in range(B)])
        if v == 0 and bool(draw["smooth_fire"].any()):
            crops = O.gaussian_smooth3d(crops, draw["sigma"].tolist(), [bool(t) for t in draw["smooth_fire"]])
        if v == 1:
            for b in range(B):
                if bool(draw["gamma_fire"][b]):
                    crops[b] = adjust_contrast(crops[b], float(draw["gamma"][b]))
        out.append(crops)
    return out
