"""Lesions on each scan's own file grid (an addition of this build): 3-D connected components of a class's mask at connectivity 6, 18
or 26, the removal of predicted components below a volume, and lesion-wise detection counts.

For class c in 1 .. K - 1: P = (pred == c and label != 255), G = (label == c), surface.py's masks.  A component is a maximal set of
mask voxels joined through face (6), face and edge (18) or face, edge and corner (26) neighbours; components are numbered 1 .. n in
raster order of their first voxel, which is scipy.ndimage.label's numbering.  A ground-truth lesion (a component of G) is DETECTED
iff at least one of its voxels lies in P; a predicted lesion (a component of P) is MATCHED iff at least one of its voxels lies in G,
otherwise it is a false alarm.

Everything per voxel runs in csrc/components.hip: `hct_cc_masks` (flag bytes), `hct_cc_label` (a lock-free union-find, root form),
`hct_cc_compact` (the numbering, a fixed-order prefix sum), `hct_cc_sizes`, `hct_cc_overlap`, `hct_cc_remove_small`, `hct_cc_count_small` and
`hct_seg_recount` (class voxels and TP / FP / FN of the filtered prediction, hct_seg_to_native's conventions).  The host reads back
the number of components once per labelling and one table per side.  No CPU path; no arithmetic of the path runs in torch ops.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .surface import _volume, _ws

CONNECTIVITIES = (6, 18, 26)


def _connectivity(connectivity) -> int:
    if connectivity not in CONNECTIVITIES or isinstance(connectivity, bool):
        raise ValueError(f"connectivity must be one of 6, 18, 26: got {connectivity!r}")
    return int(connectivity)


def _classes(num_classes, what: str) -> int:
    K = int(num_classes)
    if not 2 <= K <= 16:
        raise ValueError(f"{what}: num_classes must lie in [2, 16], got {K}")
    return K


def _labels_like(labels, pred: torch.Tensor, what: str) -> torch.Tensor:
    """`labels` as a uint8 device tensor of pred's shape.  surface_metrics' rule: a host uint8 array of exactly that shape is the mask
    file as read and is uploaded to pred's device; anything else that is not on the device is refused."""
    labels = torch.as_tensor(labels)
    if labels.dtype == torch.uint8 and tuple(labels.shape) == tuple(pred.shape) and not labels.is_cuda:
        labels = labels.to(pred.device)  # the mask file as read_native_labels returns it
    labels = _volume(labels, torch.uint8, what, pred.shape)
    if labels.device != pred.device:
        raise _lib.HctError(f"{what} (HIP): pred and labels lie on different devices")
    return labels


def tile_dims() -> tuple:
    """(tk, tj, ti): the extents of the tile one workgroup labels locally (hct_cc_tile_dims; the axis limit where there is no such phase)."""
    t = [C.c_int(0) for _ in range(3)]
    _lib.load().hct_cc_tile_dims(*(C.byref(v) for v in t))
    return tuple(int(v.value) for v in t)


def min_voxels_for(min_ml: float, affine) -> int:
    """The smallest integer n with n * voxel_ml >= min_ml, voxel_ml = |det(affine[:3, :3])| / 1000 in float64 (the volume
    native.class_volumes_ml uses), a volume within 2^-48 relative of min_ml counting as equal; 0 for min_ml = 0."""
    m = float(min_ml)
    if not (math.isfinite(m) and m >= 0):
        raise ValueError(f"min_voxels_for: min_ml must be finite and >= 0, got {min_ml!r}")
    a = np.asarray(affine, dtype=np.float64)
    det = abs(float(np.linalg.det(a[:3, :3])))
    if not (math.isfinite(det) and det > 0):
        raise ValueError(f"min_voxels_for: the affine gives a voxel of {det} mm^3")
    if m == 0.0:
        return 0
    # class_volumes_ml's arithmetic.  The determinant carries a few roundings (0.45 * 0.45 * 1 comes out one ulp below 0.2025), so a
    # volume within 2^-48 relative of the threshold has reached it: 0.2025 mL of 0.45 x 0.45 x 1 mm voxels is 1000 of them, not 1001
    reached = lambda n: n * det / 1000.0 >= m * (1.0 - 2.0 ** -48)
    n = max(int(math.floor(m * 1000.0 / det)) - 2, 0)  # the quotient may be off by a rounding either way: settle it on the product
    while not reached(n):
        n += 1
    return n


def _label(lib, flags, bit, conn, out, n_dev, ws, st) -> int:
    nk, nj, ni = flags.shape
    _lib.check(lib.hct_cc_label(flags.data_ptr(), int(bit), nk, nj, ni, conn, out.data_ptr(), ws.data_ptr(), ws.numel(), st), "hct_cc_label")
    _lib.check(lib.hct_cc_compact(out.data_ptr(), nk, nj, ni, n_dev.data_ptr(), ws.data_ptr(), ws.numel(), st), "hct_cc_compact")
    return int(n_dev.cpu().item())


def _cc_ws(lib, shape, dev, K: int = 0) -> torch.Tensor:
    nk, nj, ni = shape
    need = max(lib.hct_cc_label_workspace_bytes(nk, nj, ni), lib.hct_cc_compact_workspace_bytes(nk, nj, ni),
               lib.hct_seg_recount_workspace_bytes(nk, nj, ni, K) if K else 0)
    return _ws(need, dev)


@torch.no_grad()
def connected_components(flags: torch.Tensor, bit: int = 1, connectivity: int = 26):
    """`flags` uint8 [nk, nj, ni] on the device -> (labels int32 [nk, nj, ni] on the device, n): the components of the voxels whose
    flag byte has a bit of `bit` set, numbered 1 .. n as scipy.ndimage.label numbers them, 0 elsewhere.  One read-back (n)."""
    conn = _connectivity(connectivity)
    if not 1 <= int(bit) <= 255:
        raise ValueError(f"connected_components: bit mask {bit!r} outside [1, 255]")
    f = _volume(flags, torch.uint8, "connected_components")
    lib = _lib.load()
    with torch.cuda.device(f.device):
        out = torch.empty(tuple(f.shape), dtype=torch.int32, device=f.device)
        n_dev = torch.empty(1, dtype=torch.int64, device=f.device)
        n = _label(lib, f, bit, conn, out, n_dev, _cc_ws(lib, f.shape, f.device), _lib.stream_ptr(f.device))
    return out, n


@torch.no_grad()
def component_sizes(labels: torch.Tensor, n: int) -> torch.Tensor:
    """int64 [n + 1] on the device: voxels per component of `labels` (what connected_components returns); entry 0 is 0."""
    lab = _volume(labels, torch.int32, "component_sizes")
    n = int(n)
    if not 0 <= n <= lab.numel():
        raise ValueError(f"component_sizes: {n} components of {lab.numel()} voxels")
    with torch.cuda.device(lab.device):
        sizes = torch.empty(n + 1, dtype=torch.int64, device=lab.device)
        _lib.check(_lib.load().hct_cc_sizes(lab.data_ptr(), lab.numel(), n, sizes.data_ptr(), _lib.stream_ptr(lab.device)), "hct_cc_sizes")
    return sizes


@torch.no_grad()
def remove_small_components(pred: torch.Tensor, num_classes: int, min_voxels: int, connectivity: int = 26, labels=None, class_voxels=None,
                            counts=None) -> dict:
    """Every component of a foreground class of `pred` (int16 [nk, nj, ni] on the device) with fewer than `min_voxels` voxels becomes
    background, class by class; the annotation plays no part in it.  -> {"pred": the filtered copy, "class_voxels": int64 [K],
    "counts": int64 [K, 3] TP / FP / FN against `labels` (None without labels), "removed": int64 [K] components removed per class},
    the first three on the device; one read-back of n per class and one of "removed".  `labels` is a uint8 tensor on the device;
    as in surface_metrics, a host uint8 array of the right shape (the mask file as read) is accepted too and uploaded.  With
    min_voxels <= 1 no component can be removed and nothing is launched: `pred` itself comes back, "removed" is all 0, and
    "class_voxels" / "counts" are the figures of the unfiltered prediction the caller hands in as `class_voxels` / `counts` (what
    seg_to_native returned; None where none were given) -- the two parameters serve this path alone."""
    K = _classes(num_classes, "remove_small_components")
    conn = _connectivity(connectivity)
    pred = _volume(pred, torch.int16, "remove_small_components")
    if labels is not None:
        labels = _labels_like(labels, pred, "remove_small_components")
    removed = np.zeros(K, dtype=np.int64)
    if int(min_voxels) <= 1:
        return {"pred": pred, "class_voxels": class_voxels, "counts": counts, "removed": removed}
    nk, nj, ni = pred.shape
    dev, nvox = pred.device, pred.numel()
    lib = _lib.load()
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        out = pred.clone()
        flags = torch.empty(nk, nj, ni, dtype=torch.uint8, device=dev)
        lab = torch.empty(nk, nj, ni, dtype=torch.int32, device=dev)
        n_dev = torch.empty(1, dtype=torch.int64, device=dev)
        ws = _cc_ws(lib, pred.shape, dev, K)
        removed_d = torch.zeros(K, dtype=torch.int64, device=dev)
        for c in range(1, K):
            _lib.check(lib.hct_cc_masks(out.data_ptr(), None, nk, nj, ni, c, flags.data_ptr(), st), "hct_cc_masks")
            n = _label(lib, flags, 1, conn, lab, n_dev, ws, st)
            if n == 0:
                continue
            sizes = torch.empty(n + 1, dtype=torch.int64, device=dev)
            _lib.check(lib.hct_cc_sizes(lab.data_ptr(), nvox, n, sizes.data_ptr(), st), "hct_cc_sizes")
            _lib.check(lib.hct_cc_remove_small(out.data_ptr(), lab.data_ptr(), sizes.data_ptr(), int(min_voxels), nvox, st), "hct_cc_remove_small")
            _lib.check(lib.hct_cc_count_small(sizes.data_ptr(), n, int(min_voxels), removed_d[c:].data_ptr(), st), "hct_cc_count_small")
        removed = removed_d.cpu().numpy()  # one read-back for all classes, not a table of sizes per class
        cv = torch.empty(K, dtype=torch.int64, device=dev)
        cn = torch.empty(K, 3, dtype=torch.int64, device=dev) if labels is not None else None
        _lib.check(lib.hct_seg_recount(out.data_ptr(), _lib.ptr(labels), nk, nj, ni, K, cv.data_ptr(), _lib.ptr(cn), ws.data_ptr(), ws.numel(), st),
                   "hct_seg_recount")
    return {"pred": out, "class_voxels": cv, "counts": cn, "removed": removed}


@torch.no_grad()
def lesion_metrics(pred: torch.Tensor, labels, num_classes: int, connectivity: int = 26) -> dict:
    """`pred` int16 [nk, nj, ni] on the device, `labels` uint8 of the same shape (255 = ignore) -> {"n_gt", "n_pred", "gt_detected",
    "pred_matched": int64 [K] numpy arrays, index 0 (the background) all 0; "lesions": [(class, side, index, voxels, overlap_voxels)]
    with side "gt" (overlap with P) or "pred" (overlap with G), in component order, the truth's before the prediction's within a
    class}.  Per class and side one read-back of n and one of the [2, n + 1] table of sizes and overlaps.  `labels` on the device;
    as in surface_metrics, a host uint8 array of the right shape is accepted too and uploaded once."""
    K = _classes(num_classes, "lesion_metrics")
    conn = _connectivity(connectivity)
    pred = _volume(pred, torch.int16, "lesion_metrics")
    labels = _labels_like(labels, pred, "lesion_metrics")
    nk, nj, ni = pred.shape
    dev, nvox = pred.device, pred.numel()
    lib = _lib.load()
    out = {k: np.zeros(K, dtype=np.int64) for k in ("n_gt", "n_pred", "gt_detected", "pred_matched")}
    lesions = []
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        flags = torch.empty(nk, nj, ni, dtype=torch.uint8, device=dev)
        lab = torch.empty(nk, nj, ni, dtype=torch.int32, device=dev)
        n_dev = torch.empty(1, dtype=torch.int64, device=dev)
        ws = _cc_ws(lib, pred.shape, dev)
        for c in range(1, K):
            _lib.check(lib.hct_cc_masks(pred.data_ptr(), labels.data_ptr(), nk, nj, ni, c, flags.data_ptr(), st), "hct_cc_masks")
            for side, bit, other, n_key, hit_key in (("gt", 2, 1, "n_gt", "gt_detected"), ("pred", 1, 2, "n_pred", "pred_matched")):
                n = _label(lib, flags, bit, conn, lab, n_dev, ws, st)
                out[n_key][c] = n
                if n == 0:
                    continue
                table = torch.empty(2, n + 1, dtype=torch.int64, device=dev)
                _lib.check(lib.hct_cc_sizes(lab.data_ptr(), nvox, n, table[0].data_ptr(), st), "hct_cc_sizes")
                _lib.check(lib.hct_cc_overlap(lab.data_ptr(), n, flags.data_ptr(), other, nvox, table[1].data_ptr(), st), "hct_cc_overlap")
                t = table.cpu().numpy()
                out[hit_key][c] = int((t[1, 1:] > 0).sum())
                lesions.extend((c, side, m, int(t[0, m]), int(t[1, m])) for m in range(1, n + 1))
    out["lesions"] = lesions
    return out
