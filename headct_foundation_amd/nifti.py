"""Host side of the loading chain (src/data/transforms.py:108-178): a NIfTI-1 reader (and a writer for maps in model space), the RAS reorientation and the geometry of
Spacingd(pixdim=(1, 1, 1), mode=3), with numpy, gzip and struct only.  nibabel and MONAI are not dependencies of this build:
what they do is written out here from knowledge of nibabel 5 and MONAI 1.2 / 1.3 (`get_best_affine`, `io_orientation`,
`Orientation`, `compute_shape_offset`), and pinned by the tests against scipy.ndimage and hand-built headers, not against
those libraries themselves.

The arithmetic of the resampling is that of `scipy.ndimage.map_coordinates(order=3, mode="nearest")`, which MONAI's `Resample`
runs for an integer mode (padding mode "border" -> "nearest").  For a per-axis scale it is separable, and per axis it is linear:
edge-pad, cubic B-spline prefilter (pole z = sqrt(3) - 2, impulse response sqrt(3) z^|k|), four interpolation weights.
`bspline3_tables` folds the three into one table of TAPS weights per output voxel, so that the device runs one truncated FIR
per axis and no serial recursion.  MONAI's Spacing computes in float64 and casts the result to float32; the tables are float64 and
the device accumulates in float64 for the same reason (csrc/loading.hip)."""
from __future__ import annotations

import gzip
import struct
import zlib

import numpy as np

# NIfTI-1 datatype code -> numpy type character (the codes this build reads)
_DTYPES = {2: "u1", 4: "i2", 8: "i4", 16: "f4", 64: "f8", 256: "i1", 512: "u2"}

PREFILTER_REACH = 14            # taps kept on each side of the prefilter's impulse response: |z|^15 = 2.6e-9
TAPS = 4 + 2 * PREFILTER_REACH  # input samples one output voxel reads along an axis
MAX_AXIS = 1024                 # longest axis the resampling kernels take, in and out


def read_nifti(path):
    """(raw, slope, inter, affine): `raw` is the volume in file order and file dtype as an array [nk, nj, ni] (C order, so the
    first NIfTI axis i is the contiguous one: raw[k, j, i] is nibabel's dataobj[i, j, k]) in native byte order; value = raw *
    slope + inter, or raw where slope is None (scl_slope 0 or NaN, as nibabel reads it); affine [4, 4] float64 is nibabel's
    `get_best_affine`.  Single-file NIfTI-1 (.nii, .nii.gz), either byte order, one 3-D volume; anything else raises ValueError."""
    path = str(path)
    try:
        with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
            data = f.read()
    except (OSError, EOFError, zlib.error) as e:
        raise ValueError(f"{path}: cannot be read ({e})") from e
    if len(data) < 348:
        raise ValueError(f"{path}: {len(data)} bytes is shorter than a NIfTI-1 header")
    size_le, size_be = struct.unpack_from("<i", data)[0], struct.unpack_from(">i", data)[0]
    if size_le == 348:
        bo = "<"
    elif size_be == 348:
        bo = ">"
    elif 540 in (size_le, size_be):
        raise ValueError(f"{path}: NIfTI-2 is not read (sizeof_hdr 540)")
    else:
        raise ValueError(f"{path}: not a NIfTI-1 file (sizeof_hdr {size_le})")
    magic = data[344:348]
    if magic != b"n+1\0":
        what = "an Analyze / NIfTI header-image pair" if magic in (b"ni1\0", b"\0\0\0\0") else f"magic {magic!r}"
        raise ValueError(f"{path}: only single-file NIfTI-1 (magic n+1) is read, this is {what}")
    dim = struct.unpack_from(bo + "8h", data, 40)
    datatype, bitpix = struct.unpack_from(bo + "2h", data, 70)
    pixdim = np.array(struct.unpack_from(bo + "8f", data, 76), dtype=np.float64)
    vox_offset, slope, inter = struct.unpack_from(bo + "3f", data, 108)
    qform_code, sform_code = struct.unpack_from(bo + "2h", data, 252)
    quat = struct.unpack_from(bo + "6f", data, 256)  # quatern b, c, d, qoffset x, y, z
    srows = np.array(struct.unpack_from(bo + "12f", data, 280), dtype=np.float64).reshape(3, 4)
    if dim[0] == 4 and dim[4] == 1:
        pass  # a single volume with a time axis of one: squeezed
    elif dim[0] != 3:
        raise ValueError(f"{path}: dim {dim[:dim[0] + 1] if 0 < dim[0] < 8 else dim} is not one 3-D volume")
    shape = tuple(int(d) for d in dim[1:4])
    if min(shape) < 1:
        raise ValueError(f"{path}: bad shape {shape}")
    if datatype not in _DTYPES:
        raise ValueError(f"{path}: datatype code {datatype} is not read (uint8, int16, int32, float32, float64, int8 and uint16 are)")
    dt = np.dtype(bo + _DTYPES[datatype])
    start, count = int(vox_offset), shape[0] * shape[1] * shape[2]
    if start < 348 or start + count * dt.itemsize > len(data):
        raise ValueError(f"{path}: truncated ({len(data)} bytes, the volume needs {start + count * dt.itemsize})")
    raw = np.frombuffer(data, dtype=dt, count=count, offset=start).reshape(shape[::-1])
    raw = raw.astype(dt.newbyteorder("="), copy=False)
    if slope == 0 or not np.isfinite(slope) or not np.isfinite(inter):
        slope, inter = None, None
    return raw, slope, inter, _best_affine(shape, pixdim, qform_code, sform_code, quat, srows, path)


def write_nifti(path, array, affine=None, dtype="f4"):
    """Write `array` [nk, nj, ni] (C order, as `read_nifti` returns it) as a single-file NIfTI-1 volume (.nii, or .nii.gz through
    gzip) of float32 (`dtype` "f4") or int16 ("i2"), little-endian.  The sform (code 2, "aligned") is written from `affine` [4, 4],
    the identity when None; no qform; scl_slope 0 (the stored values are the values).  float32 keeps the bits of the array;
    int16 requires values that int16 holds exactly."""
    codes = {"f4": (16, 32), "i2": (4, 16)}
    key = np.dtype(dtype).newbyteorder("=").str[1:]
    if key not in codes:
        raise ValueError(f"write_nifti writes float32 ('f4') or int16 ('i2'), not {dtype!r}")
    a = np.asarray(array)
    if a.ndim != 3 or min(a.shape) < 1 or max(a.shape) > 32767:
        raise ValueError(f"write_nifti takes one 3-D volume [nk, nj, ni] with axes up to 32767, got shape {a.shape}")
    out = np.ascontiguousarray(a, dtype="<" + key)
    if key == "i2" and not np.array_equal(out, a):
        raise ValueError("write_nifti: the array does not fit int16 exactly")
    aff = np.eye(4) if affine is None else np.asarray(affine, dtype=np.float64)
    if aff.shape != (4, 4):
        raise ValueError(f"affine must be [4, 4], got {aff.shape}")
    nk, nj, ni = a.shape
    zooms = np.sqrt((aff[:3, :3] ** 2).sum(axis=0))
    hdr = bytearray(352)  # the 348-byte header and four bytes of "no extension"
    struct.pack_into("<i", hdr, 0, 348)
    struct.pack_into("<8h", hdr, 40, 3, ni, nj, nk, 1, 1, 1, 1)
    struct.pack_into("<2h", hdr, 70, *codes[key])
    struct.pack_into("<8f", hdr, 76, 1.0, zooms[0], zooms[1], zooms[2], 1.0, 1.0, 1.0, 1.0)
    struct.pack_into("<3f", hdr, 108, 352.0, 0.0, 0.0)  # vox_offset, scl_slope, scl_inter
    hdr[123] = 2  # xyzt_units: millimetres
    struct.pack_into("<2h", hdr, 252, 0, 2)  # qform_code, sform_code
    struct.pack_into("<12f", hdr, 280, *aff[:3].reshape(-1))
    hdr[344:348] = b"n+1\0"
    path = str(path)
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(bytes(hdr))
        f.write(out.tobytes())


def _best_affine(shape, pixdim, qform_code, sform_code, quat, srows, path):
    aff = np.eye(4)
    if sform_code > 0:
        aff[:3] = srows
        return aff
    if qform_code > 0:
        b, c, d = (float(q) for q in quat[:3])
        w2 = 1.0 - (b * b + c * c + d * d)
        if w2 < -3 * np.finfo(np.float32).eps:
            raise ValueError(f"{path}: quaternion ({b}, {c}, {d}) is longer than one")
        a = np.sqrt(max(w2, 0.0))
        s = 2.0 / (a * a + b * b + c * c + d * d)
        R = np.array([[1 - s * (c * c + d * d), s * (b * c - a * d), s * (b * d + a * c)],
                      [s * (b * c + a * d), 1 - s * (b * b + d * d), s * (c * d - a * b)],
                      [s * (b * d - a * c), s * (c * d + a * b), 1 - s * (b * b + c * c)]])
        vox = pixdim[1:4].copy()
        if (vox < 0).any():
            raise ValueError(f"{path}: negative pixdim {vox}")
        vox[2] *= -1.0 if pixdim[0] == -1 else 1.0  # qfac; anything but -1 reads as 1
        aff[:3, :3] = R * vox
        aff[:3, 3] = quat[3:6]
        return aff
    zooms = pixdim[1:4]
    aff[:3, :3] = np.diag(zooms)
    aff[:3, 3] = -(np.array(shape, dtype=np.float64) - 1) / 2.0 * zooms  # the centre of the volume at the origin
    return aff


def ras_axes(affine, shape=None):
    """(perm, flip, zooms, affine_ras): output axis o of the RAS volume is input axis perm[o], reversed where flip[o]; zooms[o] is
    its voxel size and affine_ras the affine of the reoriented volume (the translation moves only when `shape`, the input shape
    (ni, nj, nk), is given).  The assignment is nibabel's `io_orientation`, the reordering MONAI's `Orientation(axcodes="RAS")`."""
    affine = np.asarray(affine, dtype=np.float64)
    RZS = affine[:3, :3]
    zooms = np.sqrt((RZS * RZS).sum(axis=0))
    zooms[zooms == 0] = 1.0
    RS = RZS / zooms
    P, S, Qs = np.linalg.svd(RS, full_matrices=False)
    keep = S > S.max() * 3 * np.finfo(S.dtype).eps
    R = P[:, keep] @ Qs[keep]
    out_of, sign = [-1] * 3, [1] * 3
    for in_ax in range(3):
        col = R[:, in_ax]
        if np.allclose(col, 0):
            raise ValueError("affine has a degenerate axis")
        o = int(np.argmax(np.abs(col)))
        out_of[in_ax], sign[in_ax] = o, -1 if col[o] < 0 else 1
        R[o, :] = 0  # taken
    perm = [out_of.index(o) for o in range(3)]
    flip = [sign[perm[o]] < 0 for o in range(3)]
    ras = np.eye(4)
    ras[:3, 3] = affine[:3, 3]
    for o in range(3):
        col = affine[:3, perm[o]]
        ras[:3, o] = -col if flip[o] else col
        if flip[o] and shape is not None:
            ras[:3, 3] += col * (shape[perm[o]] - 1)
    return perm, flip, [float(zooms[perm[o]]) for o in range(3)], ras


def spacing_geometry(n, zoom, pixdim=1.0):
    """(m, step) along one axis of Spacingd(pixdim, diagonal=False, align_corners=False, scale_extent=False) after the
    reorientation, where it is a per-axis scale: an axis of n voxels of size zoom becomes m = round((n - 1) zoom / pixdim + 1)
    voxels (numpy's round: half to even), and output voxel j reads input coordinate j * step, step = pixdim / zoom."""
    m = int(np.round((n - 1) * float(zoom) / pixdim + 1))
    return max(m, 1), pixdim / float(zoom)


def bspline3_tables(n, m, step):
    """(base int32 [m], weights float64 [TAPS, m]) of one axis: out[j] = sum_t weights[t, j] * in[clamp(base[j] + t, 0, n - 1)].
    Row j is the product, in float64, of the four cubic B-spline weights at x = j * step (nodes floor(x) - 1 ... floor(x) + 2) and
    the prefilter's impulse response truncated to +- PREFILTER_REACH, read from the edge-extended signal.  The nodes beyond the
    volume get coefficients of their own that way, as scipy computes them on its padded copy; they are not copies of the border
    coefficient."""
    x = np.arange(m, dtype=np.float64) * step
    fl = np.floor(x)
    t = x - fl
    w4 = np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6])
    z = np.sqrt(3.0) - 2.0
    h = np.sqrt(3.0) * z ** np.abs(np.arange(-PREFILTER_REACH, PREFILTER_REACH + 1))
    w = np.zeros((TAPS, m))
    for q in range(4):  # node fl - 1 + q reads samples fl - 1 + q - REACH ... + REACH: taps q ... q + 2 REACH
        w[q:q + 2 * PREFILTER_REACH + 1] += w4[q] * h[:, None]
    base = (fl - 1 - PREFILTER_REACH).astype(np.int32)
    return base, w
