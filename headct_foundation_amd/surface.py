"""Surface-distance metrics on each scan's own file grid, in millimetres (an addition of this build): the Hausdorff distance HD, its
95th percentile HD95, the average symmetric surface distance ASSD and the normalised surface Dice NSD at a tolerance, per class,
with MONAI's voxel-based definitions.

For class c in 1 .. K - 1: P = (pred == c), G = (label == c), a voxel labelled 255 being background in both.  The surface E(M) of
a mask is M without its erosion by the 6-neighbourhood, with everything outside the volume background.  d(p -> G) is the Euclidean
distance of a voxel p of E(P) to the nearest voxel of E(G) under the voxel spacing, d(g -> P) likewise:
    HD = max(max d(p -> G), max d(g -> P))           HD95 = max(q95 d(p -> G), q95 d(g -> P)), numpy's linear percentile
    ASSD = (sum d(p -> G) + sum d(g -> P)) / (n_p + n_g)      NSD = (#{d(p -> G) <= tau} + #{d(g -> P) <= tau}) / (n_p + n_g)
Both masks empty: every figure NaN.  One empty: HD, HD95, ASSD NaN and NSD 0.

Everything per voxel runs in csrc/surface.hip: `hct_surface_edges` (flags, counts, the box of both surfaces), `hct_edt3d` (the exact
squared Euclidean distance transform in float64, confined to the box), `hct_surface_stats` (sums, maxima, counts within the
tolerance) and `hct_surface_select` (the two order statistics of each percentile, an exact radix select).  The host reads back eight
integers per class for the box and twelve numbers for the result.  No CPU path; no arithmetic of the path runs in torch ops.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib


def voxel_spacing(affine) -> tuple:
    """(s_k, s_j, s_i) in millimetres for arrays in file order [nk, nj, ni]: the norms of the columns of affine[:3, :3], column 0
    being file axis i.  Shear is ignored, as MONAI and nnU-Net ignore it: a sheared grid is measured as if its axes were
    orthogonal.  Raises ValueError on a spacing that is not finite or not above 0."""
    a = np.asarray(affine, dtype=np.float64)
    if a.shape != (4, 4) and a.shape != (3, 3):
        raise ValueError(f"voxel_spacing: affine [4, 4] expected, got {a.shape}")
    s = np.sqrt((a[:3, :3] ** 2).sum(axis=0))
    if not (np.all(np.isfinite(s)) and np.all(s > 0)):
        raise ValueError(f"voxel_spacing: column norms {s.tolist()} of the affine must be finite and > 0")
    return float(s[2]), float(s[1]), float(s[0])


def _spacing3(spacing) -> tuple:
    s = tuple(float(v) for v in spacing)
    if len(s) != 3 or not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"spacing must be three finite values > 0 in array order (s_k, s_j, s_i): got {spacing!r}")
    return s


def _volume(t, dtype, what: str, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 3 or t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "[nk, nj, ni]" if shape is None else str(list(shape))
        raise _lib.HctError(f"{what} (HIP): a {dtype} tensor {want} on 'cuda' expected, got {getattr(t, 'dtype', type(t))} "
                            f"{tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', 'the host')} (no CPU fallback exists)")
    return t.contiguous()


def _ws(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(16, int(nbytes)), dtype=torch.uint8, device=dev)


@torch.no_grad()
def distance_transform(flags: torch.Tensor, spacing, bit: int = 1) -> torch.Tensor:
    """The SQUARED Euclidean distance (mm^2, float64, the shape of `flags`) of every voxel to the nearest voxel whose flag byte has a
    bit of `bit` set, under `spacing` = (s_k, s_j, s_i): hct_edt3d over the whole volume.  Its square root is what
    scipy.ndimage.distance_transform_edt(~features, sampling=spacing) returns.  +inf everywhere where no voxel is flagged.  An axis
    longer than 2048 voxels is refused (_lib.HctError)."""
    f = _volume(flags, torch.uint8, "distance_transform")
    sk, sj, si = _spacing3(spacing)
    nk, nj, ni = f.shape
    out = torch.empty(nk, nj, ni, dtype=torch.float64, device=f.device)
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().hct_edt3d(f.data_ptr(), int(bit), nk, nj, ni, 0, 0, 0, nk, nj, ni, sk, sj, si, out.data_ptr(), _lib.stream_ptr(f.device)),
                   "hct_edt3d")
    return out


def percentile_ranks(n: int, q: float = 95.0):
    """(lo, hi, r) of numpy's linear percentile over n sorted values: r = q / 100 * (n - 1), lo = floor(r), hi = min(lo + 1, n - 1)."""
    r = (q / 100.0) * (n - 1)
    lo = int(math.floor(r))
    return lo, min(lo + 1, n - 1), r


def lerp_percentile(d_lo: float, d_hi: float, r: float) -> float:
    """numpy's linear interpolation between the two order statistics: d_lo + (r - lo) (d_hi - d_lo), taken from the upper value
    where r - lo >= 0.5, as numpy takes it."""
    t = r - math.floor(r)
    diff = d_hi - d_lo
    return d_hi - diff * (1.0 - t) if t >= 0.5 else d_lo + diff * t


@torch.no_grad()
def surface_metrics(pred: torch.Tensor, labels: torch.Tensor, num_classes: int, spacing, tolerance_mm: float = 2.0) -> dict:
    """`pred` int16 [nk, nj, ni] on the device (what seg_to_native returns), `labels` uint8 of the same shape (255 = ignore),
    `spacing` = (s_k, s_j, s_i) in mm (voxel_spacing) -> {"HD", "HD95", "ASSD", "NSD": float64 [K], "n_pred", "n_gt": int64 [K]} as
    numpy arrays; index 0 (the background) is NaN / 0, it is not scored.  One host read-back of the box and one of the result per
    class.  Raises _lib.HctError for anything that is not on the device; shapes, dtypes and the device are checked before any
    launch."""
    K = int(num_classes)
    if not 2 <= K <= 255:
        raise ValueError(f"surface_metrics: num_classes must lie in [2, 255], got {K}")
    tau = float(tolerance_mm)
    if not (math.isfinite(tau) and tau >= 0):
        raise ValueError(f"surface_metrics: tolerance_mm must be finite and >= 0, got {tolerance_mm!r}")
    sk, sj, si = _spacing3(spacing)
    pred = _volume(pred, torch.int16, "surface_metrics")
    labels = torch.as_tensor(labels)
    if labels.dtype == torch.uint8 and tuple(labels.shape) == tuple(pred.shape) and not labels.is_cuda:
        labels = labels.to(pred.device)
    labels = _volume(labels, torch.uint8, "surface_metrics", pred.shape)
    if labels.device != pred.device:
        raise _lib.HctError("surface_metrics (HIP): pred and labels lie on different devices")
    nk, nj, ni = pred.shape
    dev = pred.device
    lib = _lib.load()
    out = {k: np.full(K, np.nan, dtype=np.float64) for k in ("HD", "HD95", "ASSD", "NSD")}
    out["n_pred"], out["n_gt"] = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        flags = torch.empty(nk, nj, ni, dtype=torch.uint8, device=dev)
        dist_g = dist_p = None
        ws = _ws(max(lib.hct_surface_edges_workspace_bytes(nk, nj, ni), lib.hct_surface_stats_workspace_bytes(nk, nj, ni),
                     lib.hct_surface_select_workspace_bytes()), dev)
        head = torch.empty(8, dtype=torch.int64, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        vals = torch.empty(8, dtype=torch.float64, device=dev)  # sum, max per direction, then the four order statistics
        for c in range(1, K):
            _lib.check(lib.hct_surface_edges(pred.data_ptr(), labels.data_ptr(), nk, nj, ni, c, flags.data_ptr(), head.data_ptr(), ws.data_ptr(),
                                             ws.numel(), st), "hct_surface_edges")
            n_p, n_g, *box = (int(v) for v in head.cpu().tolist())
            out["n_pred"][c], out["n_gt"][c] = n_p, n_g
            if n_p == 0 and n_g == 0:
                continue
            if n_p == 0 or n_g == 0:
                out["NSD"][c] = 0.0
                continue
            if dist_g is None:
                dist_g = torch.empty(nk, nj, ni, dtype=torch.float64, device=dev)
                dist_p = torch.empty(nk, nj, ni, dtype=torch.float64, device=dev)
            _lib.check(lib.hct_edt3d(flags.data_ptr(), 2, nk, nj, ni, *box, sk, sj, si, dist_g.data_ptr(), st), "hct_edt3d")
            _lib.check(lib.hct_edt3d(flags.data_ptr(), 1, nk, nj, ni, *box, sk, sj, si, dist_p.data_ptr(), st), "hct_edt3d")
            _lib.check(lib.hct_surface_stats(flags.data_ptr(), dist_g.data_ptr(), dist_p.data_ptr(), nk, nj, ni, *box, tau, counts.data_ptr(),
                                             vals.data_ptr(), ws.data_ptr(), ws.numel(), st), "hct_surface_stats")
            lo_p, hi_p, r_p = percentile_ranks(n_p)
            lo_g, hi_g, r_g = percentile_ranks(n_g)
            _lib.check(lib.hct_surface_select(flags.data_ptr(), dist_g.data_ptr(), dist_p.data_ptr(), nk, nj, ni, *box, lo_p, hi_p, lo_g, hi_g,
                                              vals[4:].data_ptr(), ws.data_ptr(), ws.numel(), st), "hct_surface_select")
            cn, v = counts.cpu().tolist(), vals.cpu().tolist()
            if cn[0] != n_p or cn[2] != n_g:
                raise _lib.HctError(f"surface_metrics (HIP): class {c}: {cn[0]} / {cn[2]} surface voxels scanned, {n_p} / {n_g} flagged")
            out["HD"][c] = max(v[1], v[3])
            out["HD95"][c] = max(lerp_percentile(v[4], v[5], r_p), lerp_percentile(v[6], v[7], r_g))
            out["ASSD"][c] = (v[0] + v[2]) / (n_p + n_g)
            out["NSD"][c] = (cn[1] + cn[3]) / (n_p + n_g)
    return out
