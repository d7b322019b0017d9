"""CPU restatement of the loading chain (loading_transforms, src/data/transforms.py:108-178) in the reference's order, for the
loading tests: scipy.ndimage.map_coordinates(order=3, mode="nearest") in float64 (what MONAI's Spacing computes in, dtype
float64, before it casts back to float32), the > 0 box, the HU windows, F.adaptive_avg_pool3d, the fp16 cast.  Beside it an
fp32 numpy restatement of the device's algorithm (one 32-tap FIR per axis), which sizes the error bars, a small NIfTI-1 writer and
the phantoms.  Nothing here imports the code under test except the HU windows."""
import gzip
import itertools
import struct

import numpy as np
import torch
import torch.nn.functional as F
from scipy import ndimage

NIFTI_CODES = {"uint8": (2, 8), "int16": (4, 16), "int32": (8, 32), "float32": (16, 32), "float64": (64, 64), "int8": (256, 8), "uint16": (512, 16)}
REACH = 14
TAPS = 4 + 2 * REACH


# ---- NIfTI-1 writer -----------------------------------------------------------------------------------------------------------------
def quaternion_of(R):
    """(a, b, c, d), a >= 0, of a proper rotation matrix."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    return -q if q[0] < 0 else q


def write_nifti(path, data, affine, slope=0.0, inter=0.0, byteorder="<", form="sform", dim4=False, sizeof_hdr=348, magic=b"n+1\0",
                n_volumes=1, pixdim=None):
    """`data` [ni, nj, nk] (nibabel's index order) of one of the NIfTI dtypes -> a single-file NIfTI-1 at `path` (.nii or .nii.gz).
    form: 'sform', 'qform' (quaternion from the affine) or 'none' (both codes 0: only pixdim speaks)."""
    data = np.asarray(data)
    code, bitpix = NIFTI_CODES[data.dtype.name]
    affine = np.asarray(affine, dtype=np.float64)
    zooms = np.sqrt((affine[:3, :3] ** 2).sum(0)) if pixdim is None else np.asarray(pixdim, dtype=np.float64)
    hdr = bytearray(352)
    bo = byteorder
    struct.pack_into(bo + "i", hdr, 0, sizeof_hdr)
    dims = [4 if (dim4 or n_volumes > 1) else 3, *data.shape[:3], n_volumes if (dim4 or n_volumes > 1) else 1, 1, 1, 1]
    struct.pack_into(bo + "8h", hdr, 40, *dims)
    struct.pack_into(bo + "2h", hdr, 70, code, bitpix)
    qfac, quat = 1.0, (0.0, 0.0, 0.0)
    if form == "qform":
        R = affine[:3, :3] / zooms
        if np.linalg.det(R) < 0:
            qfac, R = -1.0, R * np.array([1.0, 1.0, -1.0])
        quat = tuple(quaternion_of(R)[1:])
    struct.pack_into(bo + "8f", hdr, 76, qfac, *zooms, 0.0, 0.0, 0.0, 0.0)
    struct.pack_into(bo + "3f", hdr, 108, 352.0, slope, inter)
    struct.pack_into(bo + "2h", hdr, 252, 1 if form == "qform" else 0, 1 if form == "sform" else 0)
    struct.pack_into(bo + "6f", hdr, 256, *quat, *(affine[:3, 3] if form == "qform" else (0.0, 0.0, 0.0)))
    if form == "sform":
        struct.pack_into(bo + "12f", hdr, 280, *affine[:3].reshape(-1))
    hdr[344:348] = magic
    body = np.asfortranarray(data).astype(data.dtype.newbyteorder(bo)).tobytes(order="F")  # axis i contiguous
    blob = bytes(hdr) + body * n_volumes
    with (gzip.open(path, "wb", compresslevel=1) if str(path).endswith(".gz") else open(path, "wb")) as f:
        f.write(blob)


# ---- phantoms -----------------------------------------------------------------------------------------------------------------------
def phantom(shape, seed=0, fill=0.78, shell=0.12):
    """HU volume [x, y, z] float64: an ellipsoid of tissue (40 +- 20 HU noise) inside a 1200 HU shell, in -1000 HU air.  `fill`:
    outer semi-axes as a share of the half extents (air all around, so the foreground box is not the volume)."""
    g = np.random.default_rng(seed)
    ax = [(np.arange(n) - (n - 1) / 2.0 + o) / (fill * n / 2.0) for n, o in zip(shape, (0.7, -1.3, 0.4))]
    r = np.sqrt(ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2)
    hu = np.full(shape, -1000.0)
    hu[r <= 1.0] = 1200.0
    inner = r <= 1.0 - shell
    hu[inner] = 40.0 + 20.0 * g.standard_normal(int(inner.sum()))
    return hu


def to_int16(hu, slope, inter):
    return np.clip(np.round((hu - inter) / slope), -32768, 32767).astype(np.int16)


def scaled(raw, slope, inter):
    """nibabel's read scaling followed by MONAI's float32: float64 arithmetic, then the cast."""
    if slope is None or slope == 0 or not np.isfinite(slope):
        return raw.astype(np.float32)
    return (raw.astype(np.float64) * slope + inter).astype(np.float32)


PHANTOMS = {  # name -> (RAS shape, zooms, seed, fill): in-plane downsampling with thick slices; coarse slices to be upsampled five-fold;
    # and a head that the faces of the volume cut, so that the resampling reads beyond the border where the signal is not flat
    "fine": ((150, 138, 44), (0.47, 0.47, 1.3), 1, 0.78),
    "thick": ((52, 60, 17), (0.9, 0.8, 5.0), 2, 0.78),
    "cut": ((60, 56, 21), (0.6, 0.7, 2.5), 3, 1.2),
}
INT16_SLOPE, INT16_INTER = 0.5, -1024.0
# (phantom, roi, channels) that the GPU tests run end to end; the CPU tests assert the conditions of the comparison for each
END_TO_END_CASES = [("fine", (32, 32, 32), 1), ("fine", (24, 40, 16), 3), ("thick", (32, 32, 32), 3), ("thick", (20, 28, 12), 1),
                    ("cut", (32, 32, 32), 1), ("cut", (16, 24, 40), 3)]


def phantom_ras(name):
    """(raw int16 [x, y, z], float32 values [x, y, z], zooms, RAS affine) of a named phantom."""
    shape, zooms, seed, fill = PHANTOMS[name]
    raw = to_int16(phantom(shape, seed, fill), INT16_SLOPE, INT16_INTER)
    aff = np.diag([*zooms, 1.0])
    aff[:3, 3] = [-30.0, -40.0, 10.0]
    return raw, scaled(raw, INT16_SLOPE, INT16_INTER), zooms, aff


SIGNED_PERMUTATIONS = [(p, s) for p in itertools.permutations(range(3)) for s in itertools.product((1, -1), repeat=3)]


def stored_as(data_ras, affine_ras, out_of, sign):
    """The RAS volume stored under another axis order: stored axis p runs along RAS axis out_of[p], in direction sign[p].
    Returns (stored data [i, j, k], its affine); reorienting that pair to RAS gives `data_ras` and `affine_ras` back."""
    stored = np.transpose(data_ras, out_of)
    aff = np.eye(4)
    aff[:3, 3] = affine_ras[:3, 3]
    for p in range(3):
        col = affine_ras[:3, out_of[p]]
        if sign[p] < 0:
            stored = np.flip(stored, axis=p)
            aff[:3, 3] += col * (data_ras.shape[out_of[p]] - 1)
        aff[:3, p] = col * sign[p]
    return np.ascontiguousarray(stored), aff


def tilted(affine, degrees=15.0):
    """The affine with its frame rotated about the x axis (a tilted gantry): same closest axes, same zooms."""
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    T = np.eye(4)
    T[1:3, 1:3] = [[c, -s], [s, c]]
    return T @ affine


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
def out_length(n, zoom, pixdim=1.0):
    return int(np.round((n - 1) * zoom / pixdim + 1))


def resample_f64(values, zooms):
    """Spacingd(pixdim=1, mode=3) on a RAS volume with a per-axis scale: float64 [m0, m1, m2]."""
    m = [out_length(n, z) for n, z in zip(values.shape, zooms)]
    grids = np.meshgrid(*[np.arange(mm, dtype=np.float64) * (1.0 / z) for mm, z in zip(m, zooms)], indexing="ij")
    return ndimage.map_coordinates(values.astype(np.float64), grids, order=3, mode="nearest", output=np.float64)


def fir_tables(n, m, step):
    """Row j of one axis as the device reads it: base[j] and TAPS weights on the samples clamp(base[j] + t): the four cubic
    B-spline weights at j * step times the prefilter's impulse response sqrt(3) z^|k|, |k| <= REACH.  Built entry by entry."""
    z = np.sqrt(3.0) - 2.0
    base, w = np.zeros(m, dtype=np.int64), np.zeros((TAPS, m))
    for j in range(m):
        x = j * step
        fl = int(np.floor(x))
        t = x - fl
        bw = [(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6]
        base[j] = fl - 1 - REACH
        for q in range(4):
            for k in range(-REACH, REACH + 1):
                w[q + k + REACH, j] += bw[q] * np.sqrt(3.0) * z ** abs(k)
    return base, w.astype(np.float32)


def fir_axis_f32(x, axis, base, w):
    n = x.shape[axis]
    acc = None
    for t in range(TAPS):
        idx = np.clip(base + t, 0, n - 1)
        shape = [1, 1, 1]
        shape[axis] = -1
        term = w[t].reshape(shape) * np.take(x, idx, axis=axis)
        acc = term if acc is None else (acc + term).astype(np.float32)
    return acc.astype(np.float32)


def resample_fir_f32(values, zooms):
    """The device's algorithm in float32 numpy: axis 0, 1, 2, ascending taps (no fused multiply-add)."""
    x = values.astype(np.float32)
    for a in range(3):
        m = out_length(x.shape[a], zooms[a])
        base, w = fir_tables(x.shape[a], m, 1.0 / zooms[a])
        x = fir_axis_f32(x, a, base, w)
    return x


def foreground_box(vol, threshold=0.0):
    """(start[3], size[3]) of the voxels > threshold, or None where there is none."""
    mask = vol > threshold
    if not mask.any():
        return None
    start, size = [], []
    for a in range(3):
        hit = np.nonzero(mask.any(axis=tuple(b for b in range(3) if b != a)))[0]
        start.append(int(hit[0]))
        size.append(int(hit[-1] - hit[0] + 1))
    return start, size


def hu_windows(in_channels):
    from headct_foundation_amd.data import HU_WINDOWS
    return HU_WINDOWS[in_channels]


def window_resize(vol_f32, box, roi, in_channels):
    """crop -> windows (ScaleIntensityRange, clip) -> Resized(mode "area") -> fp16, on a float32 volume: torch [C, *roi] fp16."""
    (s0, s1, s2), (n0, n1, n2) = box
    crop = torch.from_numpy(np.ascontiguousarray(vol_f32[s0:s0 + n0, s1:s1 + n1, s2:s2 + n2])).float()
    chans = [((crop - lo) / (hi - lo)).clamp(0.0, 1.0) for lo, hi in hu_windows(in_channels)]
    return F.adaptive_avg_pool3d(torch.stack(chans)[None], tuple(roi))[0].to(torch.float16)


def chain(values, zooms, roi, in_channels, resample=resample_f64):
    """RAS float32 values -> cache item, the whole chain; `resample` picks the float64 scipy chain or the fp32 restatement."""
    vol = resample(values, zooms)
    box = foreground_box(vol)
    if box is None:
        raise ValueError("empty foreground")
    return window_resize(vol.astype(np.float32), box, roi, in_channels)


def fp16_steps(a, b):
    """Distance in fp16 steps between two non-negative fp16 tensors (their bit patterns are ordered like their values)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.dtype == torch.float16 and b.dtype == torch.float16 and float(a.min()) >= 0 and float(b.min()) >= 0
    return (a.view(torch.int16).int() - b.view(torch.int16).int()).abs()


EQUAL_SHARE = 0.995  # share of voxels on which a device result must equal the restatement (the rest within one fp16 step)
