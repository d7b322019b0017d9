"""Plain restatements, case tables and per-element bounds for the kernels that turn a NIfTI file into a training batch
(csrc/loading.hip, csrc/augment.hip and the volume kernels of csrc/elementwise.hip), shared by tests/test_volume_ref_cpu.py and
tests/test_volume_kernels_gpu.py.  What exists is reused, not restated: tests/loading_ref.py (scipy's float64 spline, the fp32 FIR, the
foreground box), tests/dino_aug_ref.py (the contrast formula), tests/affine_ref.py::plain, oracle/mae_oracle.py.

Every restatement takes an optional description of a way the kernel could be subtly wrong -- a block, a trip of a grid-stride loop
or a chunk that is never run, two axes' taps exchanged -- and then computes what such a kernel would leave behind (NaN where an
output is never written, since the GPU tests pre-fill with NaN).  The CPU file asserts that the comparison each GPU test applies
rejects that result; nothing is broken on the GPU to show it.

The launch constants below restate the kernels' own (block sizes, grid caps); the CPU file derives from them that every planted
voxel, block and trip falls where its case says."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import loading_ref as L

U = 2.0 ** -24  # fp32 unit roundoff

# ---- launch constants of the kernels under test ---------------------------------------------------------------------------------------
RAS_DIRECT_BLOCK = 256        # to_ras_direct_kernel: outputs of axis 2 per block
RAS_TILE = 32                 # to_ras_tile_kernel: 32 x 32 tiles
ROWS_BLOCK = 256              # resample_rows_kernel: outputs of a row per block (blockIdx.y)
ROWS_PER_BLOCK = 4            # ... and rows per block
STRIDED_MAX_BLOCK = 256       # resample_strided_kernel: at most 256 lanes along `inner` per block
MAX_AXIS = 1024               # kMaxAxis
BOX_MAX_CHUNKS = 1024         # kBoxMaxChunks
BOX_ROWS_PER_BLOCK = 4        # bbox_partial_kernel: one wave per row, four waves
WAVE = 64
HU_MAX_BLOCKS = 1024          # hu_window_kernel: grid cap; 256 threads of 4 voxels each
CONTRAST_MAX_CHUNKS = 256     # kContrastMaxChunks; a chunk is 1024 vec4 = 4096 values
GATHER_BLOCKS = 4096          # hct_gather_augment: blocks wanted over a launch
GAUSS_TAPS = 9
CROP_RESIZE_MAX_F = 2044      # hct_crop_resize_area: the largest multiple of 4 with F * F * (F / 4) + 255 <= INT_MAX


def bits_equal(got, want):
    """Same shape, same dtype, same bit patterns (a NaN never equals by value; it does here only against the same NaN)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---- hct_volume_to_ras ----------------------------------------------------------------------------------------------------------------
RAS_TILED_SHAPE = (33, 34, 65)   # two tiles along either tiled axis, three along axis 2, none a multiple of 32
RAS_LONG_SHAPE = (2, 3, 300)     # the file's contiguous axis on output axis 2: elements 255 / 256 straddle the direct kernel's block
RAS_DTYPES = ["int16", "uint8", "int32", "float32", "float64", "int8", "uint16"]
RAS_SCALINGS = ((None, None), (0.4878, -1024.25))
RAS_LONG_ORDERS = [((2, 0, 1), (1, 1, 1)), ((2, 0, 1), (-1, 1, -1)), ((2, 1, 0), (1, -1, 1)), ((2, 1, 0), (-1, -1, -1))]  # out_of[0] == 2


def ras_orders(dtype):
    """(out_of, sign) of the tiled-shape cases: all 48 signed permutations for int16, six for every other datatype."""
    return L.SIGNED_PERMUTATIONS if dtype == "int16" else L.SIGNED_PERMUTATIONS[::9] + [L.SIGNED_PERMUTATIONS[-1]]


def ras_data(dtype, shape, seed=3):
    g = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return (g.standard_normal(shape) * 900).astype(dtype)
    info = np.iinfo(dtype)
    return g.integers(info.min, int(info.max) + 1, size=shape).astype(dtype)


def ras_contiguous_axis(perm):
    """The output axis along which the file is contiguous: the kernel family's switch (2: direct, 0 / 1: tiles over that axis)."""
    return list(perm).index(0)


def ras_blocks(d, contiguous_axis):
    """Per output element [d0, d1, d2] the index of the block along the grid dimensions that can exceed one: for the direct kernel
    {"x": x2 // 256}, for the tile kernels {"a": xa // 32, "z": x2 // 32}."""
    idx = np.meshgrid(*[np.arange(n) for n in d], indexing="ij")
    if contiguous_axis == 2:
        return {"x": idx[2] // RAS_DIRECT_BLOCK}
    return {"a": idx[contiguous_axis] // RAS_TILE, "z": idx[2] // RAS_TILE}


def to_ras(file_order, shape_ijk, perm, flip, slope=None, inter=None, never_run=None):
    """The kernel's own statement: output element (x0, x1, x2) reads the file's flat buffer (axis i contiguous) at
    sum_o stride[perm[o]] * (flip[o] ? d[o] - 1 - x_o : x_o), scales in float64 and casts once.  `never_run` = (grid name, index):
    elements of the blocks with that index or beyond along that grid dimension stay NaN."""
    ni, nj, nk = shape_ijk
    stride = (1, ni, ni * nj)
    d = [shape_ijk[perm[o]] for o in range(3)]
    off = 0
    for o in range(3):
        x = np.arange(d[o], dtype=np.int64)
        x = d[o] - 1 - x if flip[o] else x
        shape = [1, 1, 1]
        shape[o] = -1
        off = off + (stride[perm[o]] * x).reshape(shape)
    out = L.scaled(np.asarray(file_order).reshape(-1)[off], slope, inter)
    if never_run is not None:
        name, first = never_run
        out = out.copy()
        out[ras_blocks(d, ras_contiguous_axis(perm))[name] >= first] = np.nan
    return out


def transpose_flip(stored, perm, flip):
    out = np.transpose(stored, perm)
    for o in range(3):
        if flip[o]:
            out = np.flip(out, axis=o)
    return np.ascontiguousarray(out)


# ---- hct_bspline3_resample ------------------------------------------------------------------------------------------------------------
# name -> (shape, zooms = voxel spacing in mm per axis, resampled to 1 mm).  An output axis has round((n - 1) * zoom + 1) voxels, so
# "twice as many" is a spacing a little above 2 (a step of about 0.5 input voxels between outputs): 2.007 makes exactly 300 out of
# 150 and 2.002 exactly 1024 out of 512.
RESAMPLE_CASES = {
    "rows kernel, second column block": ((2, 3, 150), (1.0, 1.0, 2.007)),       # m2 = 300 > 256
    "strided kernel, second block of the middle pass": ((2, 3, 300), (1.5, 1.4, 0.9)),  # inner = n2 = 300 > 256
    "row tail, 1 row": ((1, 1, 40), (1.0, 1.0, 1.3)),
    "row tail, 2 rows": ((1, 2, 40), (1.0, 1.0, 1.3)),
    "row tail, 3 rows": ((1, 3, 40), (1.0, 1.0, 1.3)),
    "row tail, 4 k + 1 rows": ((3, 3, 40), (1.0, 1.0, 1.3)),
    "longest axis accepted": ((1, 1, 512), (1.0, 1.0, 2.002)),                  # m2 = 1024 = kMaxAxis
}


def resample_input(name):
    shape, zooms = RESAMPLE_CASES[name]
    g = np.random.default_rng(sorted(RESAMPLE_CASES).index(name))
    return (g.standard_normal(shape) * 300).astype(np.float32), zooms


def resample_shape(shape, zooms):
    return [L.out_length(n, z) for n, z in zip(shape, zooms)]


def resample_bar(values, zooms, want):
    """The project's rule (tests/test_loading_gpu.py): four times the error of the fp32 FIR restatement on the same input."""
    return 4 * float(np.abs(L.resample_fir_f32(values, zooms) - want).max())


def resample_ok(got, want, bar):
    return got.shape == want.shape and bool(np.isfinite(got).all()) and float(np.abs(got.astype(np.float64) - want).max()) <= bar


def strided_block(inner):
    """Threads per block of resample_strided_kernel for `inner` contiguous elements."""
    return STRIDED_MAX_BLOCK if inner > 128 else 128 if inner > 64 else 64


def resample_blocks(shape, m):
    """Per output element [m0, m1, m2]: {"rows_y": column block of the rows kernel, "rows_q": the row's place among its block's four,
    "mid_x": block of the middle (strided) pass along n2 -- an output column k of the last pass draws on every column of the middle
    pass, so that one is per middle-pass element [m0, m1, n2]}."""
    i0, i1, i2 = np.meshgrid(*[np.arange(n) for n in m], indexing="ij")
    return {"rows_y": i2 // ROWS_BLOCK, "rows_q": (i0 * m[1] + i1) % ROWS_PER_BLOCK, "mid_x": np.arange(shape[2]) // strided_block(shape[2])}


def resample_never_run(values, zooms, which):
    """The fp32 FIR's result as a kernel would leave it that never ran the rows kernel's column blocks >= 1 ("rows_y": those outputs
    stay NaN) or the middle pass's blocks >= 1 ("mid_x": those columns of the intermediate volume are whatever the workspace held,
    NaN in the GPU tests, and every output draws on them)."""
    if which == "rows_y":
        out = L.resample_fir_f32(values, zooms).copy()
        out[resample_blocks(values.shape, out.shape)["rows_y"] >= 1] = np.nan
        return out
    x = values.astype(np.float32)
    for a in range(3):
        m = L.out_length(x.shape[a], zooms[a])
        base, w = L.fir_tables(x.shape[a], m, 1.0 / zooms[a])
        x = L.fir_axis_f32(x, a, base, w)
        if a == 1:
            x[:, :, np.arange(x.shape[2]) // strided_block(x.shape[2]) >= 1] = np.nan
    return x


# ---- hct_foreground_bbox --------------------------------------------------------------------------------------------------------------
BBOX_TRIP_SHAPE = (70, 130, 5)   # 9,100 rows: 1024 blocks of 4 rows take three trips
BBOX_CASES = {  # name -> (shape, (row, z) of the lone positive voxel)
    "row 0": (BBOX_TRIP_SHAPE, (0, 2)),
    "row 4095, last of the first trip": (BBOX_TRIP_SHAPE, (4095, 0)),
    "row 4096, first of the second trip": (BBOX_TRIP_SHAPE, (4096, 4)),
    "last row, third trip": (BBOX_TRIP_SHAPE, (9099, 3)),
    "last lane, m2 1": ((3, 5, 1), (7, 0)),
    "last lane, m2 63": ((3, 5, 63), (7, 62)),
    "last lane, m2 64": ((3, 5, 64), (7, 63)),
    "last lane, m2 65": ((3, 5, 65), (7, 64)),
    "last lane, m2 129": ((3, 5, 129), (7, 128)),
    "one chunk": ((1, 1, 4), (0, 2)),
}


def bbox_chunks(rows):
    return int(min(BOX_MAX_CHUNKS, max(1, (rows + 3) // 4)))


def bbox_volume(name):
    shape, (row, z) = BBOX_CASES[name]
    g = np.random.default_rng(sorted(BBOX_CASES).index(name))
    vol = -np.abs(g.standard_normal(shape)).astype(np.float32) - np.float32(0.001)
    vol.reshape(-1, shape[2])[row, z] = 1e-30
    return vol


def bbox_place(shape, row, z):
    """(trip of the partial kernel's loop, block, lane pass along z) in which the kernel meets voxel (row, z)."""
    chunks = bbox_chunks(shape[0] * shape[1])
    per_trip = chunks * BOX_ROWS_PER_BLOCK
    return row // per_trip, (row % per_trip) // BOX_ROWS_PER_BLOCK, z // WAVE


def foreground_box_as_run(vol, max_trips=None, max_lane_passes=None):
    """The box as bbox_partial_kernel + bbox_fold_kernel build it -- rows dealt to `chunks` blocks of four, trip after trip, lanes
    along z in passes of 64 -- optionally stopping after `max_trips` trips or `max_lane_passes` passes.  Returns ([start, size],
    status) in the kernel's terms: an empty foreground is the whole volume with status 1."""
    m0, m1, m2 = vol.shape
    rows = m0 * m1
    per_trip = bbox_chunks(rows) * BOX_ROWS_PER_BLOCK
    seen = vol.reshape(rows, m2) > 0
    if max_trips is not None:
        seen = seen & (np.arange(rows)[:, None] < max_trips * per_trip)
    if max_lane_passes is not None:
        seen = seen & (np.arange(m2)[None, :] < max_lane_passes * WAVE)
    r, z = np.nonzero(seen)
    if r.size == 0:
        return [[0, 0, 0], [m0, m1, m2]], 1
    x, y = r // m1, r % m1
    mn = [int(x.min()), int(y.min()), int(z.min())]
    mx = [int(x.max()), int(y.max()), int(z.max())]
    return [mn, [b - a + 1 for a, b in zip(mn, mx)]], 0


# ---- hct_crop_window_resize_area ------------------------------------------------------------------------------------------------------
WINDOWS = {  # window tables of the tests' own, (a_min, a_max) per channel; 1 and 3 are the project's
    1: [(-110.0, 190.0)],
    2: [(-100.0, 300.0), (-15.5, 64.25)],
    3: [(0.0, 80.0), (-20.0, 180.0), (-800.0, 2000.0)],
    4: [(-110.0, 190.0), (0.0, 80.0), (-20.0, 180.0), (-800.0, 2000.0)],
    8: [(-110.0, 190.0), (0.0, 80.0), (-20.0, 180.0), (-800.0, 2000.0), (-1000.0, 1000.0), (-50.5, 49.5), (100.0, 101.0), (-1024.0, 3071.0)],
}
CWR_VOLUME = (20, 22, 37)
CWR_CASES = {}  # name -> (box = (start, size), roi, n_windows)
for _r2 in (1, 5, 8, 9, 15):  # R2 % 8: a lone output, a ragged group, one full vector, a vector and one, a vector and seven
    for _w in (2, 4):
        CWR_CASES[f"R2 {_r2}, {_w} windows"] = (((2, 3, 4), (13, 14, 29)), (5, 6, _r2), _w)
for _w in (2, 4):
    CWR_CASES[f"3 voxels to 8, {_w} windows"] = (((9, 10, 11), (3, 3, 3)), (8, 8, 8), _w)           # up-sampling: windows repeat voxels
    CWR_CASES[f"box ends at the far corner, {_w} windows"] = (((7, 8, 9), (13, 14, 28)), (5, 6, 9), _w)


def cwr_volume():
    """HU-like fp32 values that every window of WINDOWS cuts on both sides."""
    g = np.random.default_rng(11)
    return (g.standard_normal(CWR_VOLUME) * 150 + 60).astype(np.float32)


def window_resize_f64(vol_f32, box, roi, windows):
    """loading_ref.window_resize for any window table, in float64: crop -> (v - lo) / (hi - lo) clipped -> area resize -> fp16."""
    (s0, s1, s2), (n0, n1, n2) = box
    crop = torch.from_numpy(np.ascontiguousarray(vol_f32[s0:s0 + n0, s1:s1 + n1, s2:s2 + n2])).double()
    chans = [((crop - lo) / (hi - lo)).clamp(0.0, 1.0) for lo, hi in windows]
    return F.adaptive_avg_pool3d(torch.stack(chans)[None], tuple(roi))[0].to(torch.float16)


def window_resize_f32(vol_f32, box, roi, windows):
    """The kernel's arithmetic in fp32 numpy: fp32 subtract, divide and clip per voxel, window sums in ascending x, y, z order, one
    divide by (nx * ny) * nz, the fp16 cast."""
    (s0, s1, s2), n = box
    f = np.float32
    out = np.zeros((len(windows),) + tuple(roi), dtype=np.float16)
    span = lambda i, a, s: (s + (i * n[a]) // roi[a], s + -((-(i + 1) * n[a]) // roi[a]))  # [floor(i n / R), ceil((i + 1) n / R))
    for c, (lo, hi) in enumerate(windows):
        rng = f(hi) - f(lo)
        win = np.minimum(np.maximum((vol_f32 - f(lo)) / rng, f(0)), f(1)).astype(np.float32)
        for i in range(roi[0]):
            x0, x1 = span(i, 0, s0)
            for j in range(roi[1]):
                y0, y1 = span(j, 1, s1)
                for k in range(roi[2]):
                    z0, z1 = span(k, 2, s2)
                    acc = f(0)
                    for v in win[x0:x1, y0:y1, z0:z1].reshape(-1):
                        acc = f(acc + v)
                    out[c, i, j, k] = np.float16(f(acc / f(f((x1 - x0) * (y1 - y0)) * f(z1 - z0))))
    return torch.from_numpy(out)


def item_rule(got, want):
    """tests/test_loading_gpu.py::_assert_item as a predicate: within one fp16 step everywhere, equal on at least EQUAL_SHARE."""
    if got.shape != want.shape or got.dtype != torch.float16 or not bool(torch.isfinite(got.float()).all()):
        return False
    steps = L.fp16_steps(got, want)
    return int(steps.max()) <= 1 and float((steps == 0).float().mean()) >= L.EQUAL_SHARE


# ---- hct_hu_window --------------------------------------------------------------------------------------------------------------------
HU_VOXELS = 1048576 + 4 * 257   # one full pass of 1024 blocks x 256 threads x 4 voxels, then a block and one thread more
HU_BATCH = 2
HU_WINDOW_COUNTS = (1, 2, 3, 8)


def hu_edges(windows):
    """Integer HU on, just inside and just outside both edges of every window."""
    return [v for lo, hi in windows for v in (np.floor(lo) - 1, np.floor(lo), np.floor(lo) + 1, np.ceil(hi) - 1, np.ceil(hi), np.ceil(hi) + 1)]


def hu_volume(windows, seed=5):
    """[HU_BATCH, HU_VOXELS] integer HU as fp32, the edges of every window planted at the start of the first pass and in the tail that
    only the second pass reaches (both samples)."""
    g = torch.Generator().manual_seed(seed)
    hu = torch.randint(-1200, 2801, (HU_BATCH, HU_VOXELS), generator=g).float()
    e = torch.tensor(hu_edges(windows), dtype=torch.float32)
    hu[:, :e.numel()] = e
    hu[:, HU_VOXELS - e.numel():] = e.flip(0)
    return hu


def hu_window_f32(hu, windows, skip_second_pass=False):
    """[B, V] -> [B, W, V] fp32 in the kernel's order: fp32 subtract, IEEE divide by the fp32 range, clamp.  `skip_second_pass`: the
    voxels beyond the grid's first pass stay NaN."""
    x = hu.float()
    lo = torch.tensor([w[0] for w in windows], dtype=torch.float32)
    hi = torch.tensor([w[1] for w in windows], dtype=torch.float32)
    out = torch.stack([((x - lo[w]) / (hi[w] - lo[w])).clamp(0.0, 1.0) for w in range(len(windows))], dim=1)
    if skip_second_pass:
        out[:, :, HU_MAX_BLOCKS * 256 * 4:] = float("nan")
    return out


def hu_passes(voxels):
    """(passes of the grid-stride loop, vec4 left for the last pass)."""
    vox4 = voxels // 4
    per_pass = min(HU_MAX_BLOCKS, (vox4 + 255) // 256) * 256
    return -(-vox4 // per_pass), vox4 - (-(-vox4 // per_pass) - 1) * per_pass


# ---- hct_adjust_contrast --------------------------------------------------------------------------------------------------------------
CONTRAST_TOL = 2e-6            # tests/test_dino_aug_gpu.py TOL: the project's bar for values in [-0.2, 1.2]
CONTRAST_N = 1048576 + 4096    # 257 chunks wanted, 256 given: the blocks' loops take a fifth trip for the last 4096 values
CONTRAST_TAIL = 1048576        # first value of the 257th chunk
CONTRAST_CASES = {  # name -> (n, position of the minimum, position of the maximum, apply per sample, gamma per sample)
    "minimum last, maximum first of the last chunk": (CONTRAST_N, CONTRAST_N - 1, CONTRAST_TAIL, (1, 0), (0.37, 0.5)),
    "maximum last, minimum first of the last chunk": (CONTRAST_N, CONTRAST_TAIL, CONTRAST_N - 1, (0, 1), (0.5, 0.61)),
    "four values": (4, 1, 2, (1, 0), (0.2, 0.5)),
}


def contrast_chunks(n):
    return int(min(CONTRAST_MAX_CHUNKS, max(1, (n // 4 + 1023) // 1024)))


def contrast_place(n, pos):
    """(trip, block, thread) of contrast_minmax_kernel's grid-stride loop that reads value `pos` of a sample."""
    i, per_trip = pos // 4, contrast_chunks(n) * 256
    return i // per_trip, (i % per_trip) // 256, i % 256


def contrast_input(name):
    """[2, n] fp32: uniform(0, 1), the unique minimum -0.2 and maximum 1.2 planted in both samples."""
    n, at_min, at_max, _, _ = CONTRAST_CASES[name]
    g = torch.Generator().manual_seed(sorted(CONTRAST_CASES).index(name))
    x = torch.rand(2, n, generator=g) * 0.98 + 0.01
    x[:, at_min], x[:, at_max] = -0.2, 1.2
    return x


def adjust_contrast_f64(x, gamma, seen=None, applied=None):
    """dino_aug_ref.adjust_contrast on one sample [n]; with `seen`, min and max are taken over x[:seen] only (a kernel whose first
    pass drops what lies beyond); with `applied`, the curve is applied to x[:applied] only (one whose second pass does)."""
    from tests import dino_aug_ref as D
    if seen is None and applied is None:
        return D.adjust_contrast(x, gamma)
    v = x.double()
    mn, mx = v[:seen].min(), v[:seen].max()
    out = (((v - mn) / (mx - mn + 1e-7)) ** float(gamma) * (mx - mn) + mn).to(torch.float32)
    if applied is not None:
        out[applied:] = x[applied:]
    return out


def contrast_ok(got, want):
    return got.shape == want.shape and bool(torch.isfinite(got).all()) and float((got.double() - want.double()).abs().max()) <= CONTRAST_TOL


# ---- hct_gaussian_smooth3d ------------------------------------------------------------------------------------------------------------
GAUSS_SHAPES = [(S, C) for S in (4, 8, 12, 20) for C in (1, 3)]
GAUSS_SIGMA = [[0.5, 0.75, 1.0], [0.62, 1.0, 0.81], [0.93, 0.55, 0.7], [1.0, 0.5, 0.66]]  # three different sigmas per sample
GAUSS_FIRE = [False, True, True, False]                                                # first and last sample not firing


def gauss_impulses(S):
    return {"corner": (0, 0, S - 1), "edge midpoint": (S - 1, S // 2, 0), "centre": (S // 2, S // 2, S // 2)}


def _correlate_axis(v, k, dim):
    """out[p] = sum_u k[u] v[p + u - 4] along `dim`, zeros outside the volume; ascending u (float64: the order does not matter)."""
    S = v.shape[dim]
    pad = [0, 0] * (v.dim() - 1 - dim) + [GAUSS_TAPS // 2, GAUSS_TAPS // 2]
    p = F.pad(v, pad)
    out = torch.zeros_like(v)
    for u in range(GAUSS_TAPS):
        out = out + k[u] * p.narrow(dim, u, S)
    return out


def gaussian_f64(x, taps, fire, axes=(0, 1, 2)):
    """Separable zero-padded filtering in float64 with the fp32 taps [B, 3, 9] the kernel is given: spatial axis a of sample b is
    filtered with taps[b, axes[a]] (axes other than (0, 1, 2): a kernel that exchanges two axes' taps).  x [B, C, S, S, S]."""
    out = x.double().clone()
    for b in range(x.shape[0]):
        if fire[b]:
            v = out[b]
            for a in range(3):
                v = _correlate_axis(v, taps[b, axes[a]].double(), 1 + a)
            out[b] = v
    return out


def gaussian_bound(x, taps, fire):
    """|kernel - gaussian_f64| <= bound per element, from the kernel's order of operations.  A pass computes
    acc = 0; acc += k[u] * v[u] for the (at most nine) taps inside the volume, in fp32 without contraction: each term is rounded once
    as a product and then takes part in at most eight additions (0 + p is exact), so by the standard analysis of recursive summation
    the pass returns sum_u k[u] v[u] (1 + t_u) with |t_u| <= g = 9 u / (1 - 9 u), u = 2^-24: its error is at most g sum |k||v|.
    The accumulator is already fp32, so storing the intermediate volume rounds nothing further.  With A_1 = |k_0| * |x| and
    A_(n+1) = |k_n| * A_n (the same filtering of absolute values), the computed pass n satisfies |c_n| <= (1 + g)^n A_n and, by
    induction over |c_n - exact_n| <= sum |k| |c_(n-1) - exact_(n-1)| + g sum |k| |c_(n-1)|,
        |c_3 - exact_3| <= ((1 + g)^3 - 1) A_3.
    The float64 reference's own rounding (27 terms, unit roundoff 2^-53) is added.  Samples that did not fire are copied: bound 0."""
    a3 = gaussian_f64(x.abs(), taps.abs(), fire)
    g = GAUSS_TAPS * U / (1 - GAUSS_TAPS * U)
    bound = ((1 + g) ** 3 - 1 + 27 * 2.0 ** -53) * a3
    for b in range(x.shape[0]):
        if not fire[b]:
            bound[b] = 0.0
    return bound


def impulse_response(taps_b, at, S):
    """The response of one sample's filter to a unit impulse at `at`: the outer product of the three axes' taps, written down
    directly (out[p] = k_0[at_0 - p_0 + 4] k_1[at_1 - p_1 + 4] k_2[at_2 - p_2 + 4], zero beyond the nine taps).  [S, S, S] float64."""
    line = []
    for a in range(3):
        u = at[a] - torch.arange(S) + GAUSS_TAPS // 2
        ok = (u >= 0) & (u < GAUSS_TAPS)
        line.append(torch.where(ok, taps_b[a].double()[u.clamp(0, GAUSS_TAPS - 1)], torch.zeros((), dtype=torch.float64)))
    return line[0][:, None, None] * line[1][None, :, None] * line[2][None, None, :]


def within(got, ref, bound):
    """(every element within its bound, worst |got - ref| / bound; 0 / 0 counts as 0)."""
    err = (got.double() - ref).abs()
    ratio = float((err / bound).nan_to_num(nan=0.0).max())
    return bool((err <= bound).all()), ratio


# ---- hct_pos_embed_interp3d -----------------------------------------------------------------------------------------------------------
POS_TOL = 2e-6  # the project's bar for this kernel on uniform(-1, 1) tables (tests/test_kernels_gpu.py)
POS_GRIDS = [(3, 3), (4, 1), (1, 3), (8, 3), (2, 7)]  # identity; to a single token; from a single token; strong down-scaling; up-scaling
POS_EXTRA = (0, 1, 5)
POS_D = (4, 48)


def pos_table(gs, extra, D, seed=0):
    g = torch.Generator().manual_seed(1000 * gs + 10 * extra + D + seed)
    return torch.rand(extra + gs ** 3, D, generator=g) * 2 - 1


def pos_interp_f64(table, gs, gd, extra):
    """[extra + gs^3, D] fp32 -> [extra + gd^3, D] float64: the extra rows as they are, the grid through
    F.interpolate(mode="trilinear", align_corners=False) in float64."""
    D = table.shape[1]
    grid = table[extra:].double().reshape(1, gs, gs, gs, D).permute(0, 4, 1, 2, 3)
    out = F.interpolate(grid, size=(gd, gd, gd), mode="trilinear", align_corners=False)
    return torch.cat([table[:extra].double(), out.permute(0, 2, 3, 4, 1).reshape(gd ** 3, D)])


# ---- hct_gather_augment ---------------------------------------------------------------------------------------------------------------
GATHER_TRIPS_CASE = dict(S=12, B=2048, C=2, n_slots=3, offset_halves=0)   # B * C = 4096: one block per volume, 432 threads' work
GATHER_NARROW_CASE = dict(S=16, B=8, C=2, n_slots=3, offset_halves=4)     # rows would allow 16-byte loads, the pool pointer does not


def gather_launch(S, B, C, pool_aligned_16):
    """(V, per_vol, blocks per volume, trips) of hct_gather_augment's launch."""
    V = 8 if (S % 8 == 0 and pool_aligned_16) else 4
    per_vol = S * S * (S // V)
    want = (GATHER_BLOCKS + B * C - 1) // (B * C)
    blocks = max(1, min((per_vol + 255) // 256, want))
    return V, per_vol, blocks, -(-per_vol // (blocks * 256))


def gather_case(case, seed=9):
    """(pool [n_slots, C, S, S, S] fp16, slot [B] int32, flip [B] uint8 -- all eight codes --, shift [B] fp32)."""
    S, B, C, n = case["S"], case["B"], case["C"], case["n_slots"]
    g = torch.Generator().manual_seed(seed)
    pool = torch.randn(n, C, S, S, S, generator=g).half()
    b = torch.arange(B)
    return pool, (b * 7 % n).to(torch.int32), (b % 8).to(torch.uint8), ((b % 5).float() - 2) * 0.05


def gather_plain(pool, slot, flip, shift, max_trips=None, pool_aligned_16=True):
    """affine_ref.plain on the gathered batch; with `max_trips`, the outputs that only a later trip of the block's loop would write
    stay NaN (thread u of a volume writes V consecutive outputs starting at V * u)."""
    from tests import affine_ref
    out = affine_ref.plain(pool[slot.long()], flip, shift)
    if max_trips is not None:
        B, C, S = out.shape[:3]
        V, per_vol, blocks, _ = gather_launch(S, B, C, pool_aligned_16)
        flat = out.view(B * C, S * S * S)
        flat[:, max_trips * blocks * 256 * V:] = float("nan")
    return out
