"""Segmentation on each scan's own grid (an addition of this build): the decoder's logits go back through the loading chain's
geometry onto the voxels of the file, where the arg-max can be laid over the scan, scored against the annotator's mask and
measured in millilitres.

The forward chain (file -> RAS -> 1 mm -> foreground box -> item, data.run_loading_chain) is a per-axis map at every step.
`ScanGeometry` keeps what it needs of one scan -- file shape, `perm` / `flip` to RAS, RAS shape `d`, resampled shape `m`, the
float64 `steps` of nifti.spacing_geometry, the file's affine and the foreground box -- and `GeometryCache` stores it as a small
JSON file beside the scan's cache item.  `native_tables` folds the chain, inverted, into four tables per FILE axis in float64;
`seg_to_native` hands them with one sample's token-layout logits to `hct_seg_to_native` (csrc/native.hip), which blends
trilinearly, takes the arg-max and counts on the device.  No CPU path; no arithmetic of the path runs in torch ops.
"""
from __future__ import annotations

import hashlib
import json
import os
import tempfile
from dataclasses import asdict, dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

INTERPS = ("linear", "nearest")


@dataclass
class ScanGeometry:
    """Host-side geometry of one scan.  `file_shape` is (ni, nj, nk); RAS axis o is file axis perm[o], reversed where flip[o], has
    d[o] voxels and m[o] after the 1 mm resampling, whose voxel j sits at RAS coordinate j * steps[o]; `start` / `size` is the
    foreground box in resampled voxels (confined to the volume), `affine` the file's own [4, 4]."""
    file_shape: tuple
    perm: tuple
    flip: tuple
    d: tuple
    m: tuple
    steps: tuple
    affine: tuple
    start: tuple
    size: tuple

    def __post_init__(self):
        i3 = lambda v: tuple(int(x) for x in v)
        self.file_shape, self.perm, self.d, self.m, self.start, self.size = (i3(v) for v in (self.file_shape, self.perm, self.d, self.m, self.start,
                                                                                              self.size))
        self.flip = tuple(bool(f) for f in self.flip)
        self.steps = tuple(float(s) for s in self.steps)
        self.affine = tuple(tuple(float(x) for x in row) for row in np.asarray(self.affine, dtype=np.float64).reshape(4, 4))
        if sorted(self.perm) != [0, 1, 2] or any(len(v) != 3 for v in (self.file_shape, self.flip, self.d, self.m, self.steps, self.start, self.size)):
            raise ValueError("ScanGeometry: perm must be a permutation of (0, 1, 2) and every field three long")
        if any(self.d[o] != self.file_shape[self.perm[o]] for o in range(3)) or min(self.file_shape) < 1:
            raise ValueError(f"ScanGeometry: d {self.d} is not file_shape {self.file_shape} under perm {self.perm}")
        if min(self.steps) <= 0 or not all(np.isfinite(self.steps)):
            raise ValueError(f"ScanGeometry: steps {self.steps} must be positive")
        if any(not (0 <= self.start[o] < self.m[o] and 1 <= self.size[o] <= self.m[o] - self.start[o]) for o in range(3)):
            raise ValueError(f"ScanGeometry: box start {self.start} size {self.size} leaves the resampled volume {self.m}")

    def to_json(self) -> str:
        return json.dumps(asdict(self))

    @classmethod
    def from_json(cls, text: str) -> "ScanGeometry":
        return cls(**json.loads(text))


def confine_box(box, m):
    """(start[3], size[3]) of the six box words as label_to_item_kernel confines them to the resampled volume `m`."""
    start = [min(max(int(box[a]), 0), int(m[a]) - 1) for a in range(3)]
    size = [min(max(int(box[3 + a]), 1), int(m[a]) - start[a]) for a in range(3)]
    return start, size


def scan_geometry(path, roi, in_channels: int, device) -> ScanGeometry:
    """The geometry of the scan at `path`: the header through DecodedVolume, the foreground box through one run of
    run_loading_chain (the item it makes is dropped).  Raises ValueError where load_volume does."""
    from .data import DecodedVolume, _roi3, run_loading_chain
    roi = _roi3(roi)
    dec = DecodedVolume(path)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HctError("scan_geometry runs on the GPU (libheadct_hip); no CPU fallback exists")
    with torch.cuda.device(device):
        _, box = run_loading_chain(dec, dec.host.to(device, non_blocking=True), roi, in_channels)
        words = torch.empty(8, dtype=torch.int32, pin_memory=True)
        words.copy_(box, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    if int(words[6]) != 0:
        raise ValueError(f"{path}: no voxel above 0 after resampling (empty foreground)")
    start, size = confine_box(words.tolist(), dec.m)
    return ScanGeometry(dec.file_shape, dec.perm, dec.flip, dec.d, dec.m, dec.steps, dec.affine, start, size)


class GeometryCache:
    """ScanGeometry files beside VolumeCache's items: one small JSON per scan, named by VolumeCache's hash text with a `|geom`
    suffix, written under a temporary name and renamed, rebuilt when it fails to load.  `maker(path, roi, in_channels, device)`
    makes a missing one; `scan_geometry` by default."""

    def __init__(self, cache_dir, roi, in_channels: int, maker=None):
        from .data import _roi3
        self.cache_dir, self.roi, self.in_channels = str(cache_dir), _roi3(roi), int(in_channels)
        self.maker = scan_geometry if maker is None else maker
        os.makedirs(self.cache_dir, exist_ok=True)

    def key(self, path) -> str:
        from .data import PIPELINE_VERSION
        text = f"v{PIPELINE_VERSION}|{path}|{self.roi}|{self.in_channels}|geom"
        return hashlib.sha256(text.encode()).hexdigest()[:32]

    def file_of(self, path) -> str:
        return os.path.join(self.cache_dir, self.key(path) + ".json")

    def _read(self, file) -> Optional[ScanGeometry]:
        try:
            with open(file) as f:
                return ScanGeometry.from_json(f.read())
        except Exception:
            return None

    def get(self, path, device) -> ScanGeometry:
        file = self.file_of(path)
        if os.path.exists(file):
            geom = self._read(file)
            if geom is not None:
                return geom
        geom = self.maker(path, self.roi, self.in_channels, device)
        fd, tmp = tempfile.mkstemp(dir=self.cache_dir, suffix=".tmp")
        try:
            with os.fdopen(fd, "w") as f:
                f.write(geom.to_json())
            os.replace(tmp, file)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise
        return geom


def native_tables(geom: ScanGeometry, roi, interp: str = "linear") -> list:
    """For each FILE axis a = 0, 1, 2 (i, j, k) a dict of tables of length n_a: `i0`, `i1` int32, `w` float32, `inside` uint8.
    File index f of axis a, feeding RAS axis o (perm[o] == a), lies at
        r = d[o] - 1 - f where flip[o], else f            the RAS index
        u = r / steps[o]                                  resampled voxel j sits at RAS coordinate j * step
        c = u - start[o]                                  inside iff -0.5 <= c < size[o] - 0.5
        t = (c + 0.5) * R[o] / size[o] - 0.5              the item coordinate, voxel-centre convention (align_corners=False)
    all in float64.  linear: t clamped to [0, R - 1], i0 = floor(t), i1 = min(i0 + 1, R - 1), w = float32(t - i0).  nearest:
    i0 = i1 = clamp(floor(t + 0.5), 0, R - 1), w = 0."""
    from .data import _roi3
    if interp not in INTERPS:
        raise ValueError(f"interp must be one of {INTERPS}, got {interp!r}")
    R = _roi3(roi)
    out = []
    for a in range(3):
        o = geom.perm.index(a)
        f = np.arange(geom.file_shape[a], dtype=np.float64)
        r = (geom.d[o] - 1 - f) if geom.flip[o] else f
        c = r / np.float64(geom.steps[o]) - geom.start[o]
        inside = (c >= -0.5) & (c < geom.size[o] - 0.5)
        t = (c + 0.5) * R[o] / geom.size[o] - 0.5
        if interp == "linear":
            t = np.clip(t, 0.0, R[o] - 1.0)
            i0 = np.floor(t)
            i1 = np.minimum(i0 + 1, R[o] - 1)
            w = (t - i0).astype(np.float32)
        else:
            i0 = i1 = np.clip(np.floor(t + 0.5), 0, R[o] - 1)
            w = np.zeros(f.size, dtype=np.float32)
        out.append({"i0": i0.astype(np.int32), "i1": i1.astype(np.int32), "w": w, "inside": inside.astype(np.uint8)})
    return out


def upload_tables(tables, device) -> dict:
    """The three axes' tables one after the other (i, then j, then k), as hct_seg_to_native reads them, on `device`."""
    return {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([t[k] for t in tables]))).to(device) for k in ("i0", "i1", "w", "inside")}


def _sample_rows(logits_b: torch.Tensor):
    if logits_b.dim() == 3 and logits_b.shape[0] == 1:
        logits_b = logits_b[0]
    if not logits_b.is_cuda or logits_b.dim() != 2 or logits_b.dtype not in (torch.float32, torch.bfloat16) or logits_b.stride(1) != 1:
        raise _lib.HctError("seg_to_native (HIP): one sample's logits [T, K * P^3] in fp32 or bf16 on 'cuda' with unit column stride expected "
                            "(no CPU fallback exists)")
    return logits_b


@torch.no_grad()
def seg_to_native(logits_b: torch.Tensor, patch_size: int, num_classes: int, first: int, geom: ScanGeometry, interp: str = "linear",
                  labels=None, tables: Optional[dict] = None) -> dict:
    """One sample's token-layout logits [T, K * P^3] (a row view of SegmentationHead's output; `first` leading rows are no patches)
    on the file grid of `geom`: {"pred": int16 [nk, nj, ni], "class_voxels": int64 [K], "counts": int64 [K, 3] = TP, FP, FN against
    `labels` (uint8 [nk, nj, ni] in file order, 255 = ignore; None: no counts)}, all on the logits' device.  `tables` takes what
    `upload_tables(native_tables(...))` gave for this geometry, to save the upload on a repeated call."""
    from .segmentation import MAX_CLASSES
    x = _sample_rows(logits_b)
    T, N = x.shape
    P, K, first = int(patch_size), int(num_classes), int(first)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"seg_to_native: num_classes must lie in [2, {MAX_CLASSES}], got {K}")
    if N != K * P ** 3:
        raise _lib.HctError(f"seg_to_native (HIP): {N} columns, K * P^3 = {K * P ** 3} expected")
    L = T - first
    G = round(L ** (1.0 / 3.0)) if L > 0 else 0
    if first < 0 or G < 1 or G ** 3 != L:
        raise _lib.HctError(f"seg_to_native (HIP): T - first = {L} tokens are no cubic patch grid")
    dev = x.device
    ni, nj, nk = geom.file_shape
    if tables is None:
        tables = upload_tables(native_tables(geom, G * P, interp), dev)
    if any(tables[k].numel() != ni + nj + nk for k in ("i0", "i1", "w", "inside")):
        raise _lib.HctError("seg_to_native (HIP): the tables do not belong to this geometry")
    lib = _lib.load()
    with torch.cuda.device(dev):
        counts = None
        if labels is not None:
            labels = torch.as_tensor(labels)
            if labels.dtype != torch.uint8 or tuple(labels.shape) != (nk, nj, ni):
                raise _lib.HctError(f"seg_to_native (HIP): labels uint8 [{nk}, {nj}, {ni}] expected, got {labels.dtype} {tuple(labels.shape)}")
            labels = labels.to(dev).contiguous()
            counts = torch.empty(K, 3, dtype=torch.int64, device=dev)
        pred = torch.empty(nk, nj, ni, dtype=torch.int16, device=dev)
        class_voxels = torch.empty(K, dtype=torch.int64, device=dev)
        ws = torch.empty(max(16, lib.hct_seg_to_native_workspace_bytes(ni, nj, nk, K)), dtype=torch.uint8, device=dev)
        _lib.check(lib.hct_seg_to_native(x.data_ptr(), _lib.dtype_code(x), x.stride(0), T, first, G, P, K, tables["i0"].data_ptr(),
                                         tables["i1"].data_ptr(), tables["w"].data_ptr(), tables["inside"].data_ptr(), *geom.perm, ni, nj, nk,
                                         _lib.ptr(labels), pred.data_ptr(), class_voxels.data_ptr(), _lib.ptr(counts), ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr(dev)), "hct_seg_to_native")
    return {"pred": pred, "class_voxels": class_voxels, "counts": counts}


def class_volumes_ml(class_voxels, affine) -> np.ndarray:
    """Millilitres per class: voxels * |det(affine[:3, :3])| / 1000 (the affine maps voxel indices to millimetres)."""
    v = class_voxels.detach().cpu().numpy() if isinstance(class_voxels, torch.Tensor) else np.asarray(class_voxels)
    a = np.asarray(affine, dtype=np.float64)
    return v.astype(np.float64) * abs(float(np.linalg.det(a[:3, :3]))) / 1000.0


def read_native_labels(seg_path, geom: ScanGeometry, img_path="") -> np.ndarray:
    """The mask file as uint8 [nk, nj, ni] in file order, validated like data.load_label_volume: the image's shape and affine (1e-3
    per entry), every value an integer in [0, 254].  Raises ValueError otherwise."""
    from . import nifti
    raw, slope, inter, affine = nifti.read_nifti(seg_path)
    nk, nj, ni = raw.shape
    if (ni, nj, nk) != tuple(geom.file_shape):
        raise ValueError(f"{seg_path}: mask shape {(ni, nj, nk)} differs from the image's {tuple(geom.file_shape)} ({img_path})")
    if float(np.abs(np.asarray(affine) - np.asarray(geom.affine)).max()) > 1e-3:
        raise ValueError(f"{seg_path}: mask affine differs from the image's ({img_path})")
    v = raw if slope is None else raw.astype(np.float64) * slope + inter
    if not bool(np.all((v >= 0) & (v <= 254) & (v == np.floor(v)))):
        raise ValueError(f"{seg_path}: a mask value is no integer in [0, 254]")
    return np.ascontiguousarray(v.astype(np.uint8))
