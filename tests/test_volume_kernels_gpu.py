"""GPU: the kernels that turn a NIfTI file into a training batch, one by one through the C ABI, against the plain restatements of
tests/volume_ref.py at the shapes where the grid takes a second block, a loop a second trip or a template instance runs that no
other test reaches.  tests/test_volume_ref_cpu.py asserts, without a GPU, that each case lands where this list says and that the
comparison applied here rejects a kernel that skips that block, trip or chunk.

What each case reaches:
  hct_volume_to_ras        RAS (33, 34, 65), all 48 signed permutations (int16; six for the other datatypes), scaled and not:
                           to_ras_tile_kernel<T, 0> and <T, 1> with blockIdx.x = 1 (second tile of the tiled axis) and blockIdx.y = 1, 2
                           (second and third z-tile), ragged on both; to_ras_direct_kernel with 65 of 256 lanes.  RAS (2, 3, 300), file
                           contiguous along output axis 2: to_ras_direct_kernel with blockIdx.x = 1, read forwards and backwards.
  hct_bspline3_resample    (2, 3, 150) -> m2 = 300: resample_rows_kernel blockIdx.y = 1.  (2, 3, 300): the second
                           resample_strided_kernel launch (inner = n2 = 300) blockIdx.x = 1.  m0 * m1 = 1, 2, 3, 9: nr = 1, 2, 3 and a
                           last block of one row.  (1, 1, 512) -> 1024 = kMaxAxis accepted; 1025 refused.
  hct_foreground_bbox      (70, 130, 5): 9,100 rows over 1024 blocks of 4: three trips; the lone positive voxel in row 0 (trip 0, block 0),
                           4095 (trip 0, block 1023), 4096 (trip 1, block 0), 9099 (trip 2).  m2 = 1, 63, 64, 65, 129 with the voxel in the
                           last lane: lane passes 1, 1, 1, 2, 3 of a wave.  (1, 1, 4): one chunk.
  hct_crop_window_resize_area  crop_window_resize_kernel<2> and <4>; R2 = 1, 5, 8 (vector store), 9, 15 (scalar tails); a 3-voxel box
                           up-sampled to 8; a box that ends at the far corner of the volume.
  hct_hu_window            1,048,576 + 4 * 257 voxels, B = 2: 1024 blocks, a second trip for block 0 and thread 0 of block 1; W = 1, 2, 3, 8;
                           the four <TIn, TOut> instances; W = 9 and voxels % 4 != 0 refused.
  hct_adjust_contrast      n = 1,048,576 + 4096: 257 chunks wanted, 256 launched, a fifth trip for blocks 0 ... 3 that alone holds the
                           minimum and the maximum (both orders); a sample that does not fire; n = 4: one chunk, one thread.
  hct_gaussian_smooth3d    S = 4 (narrower than the nine taps), 8, 12, 20; C = 1, 3; per-axis sigmas; first and last sample skipped, all
                           skipped; unit impulses at a corner, an edge midpoint and the centre; aliased buffers refused.
  hct_pos_embed_interp3d   3 -> 3 (weights 1 and 0), 4 -> 1, 1 -> 3 (i1 clamped to i0), 8 -> 3 (strong down-scaling), 2 -> 7 (negative source
                           coordinate clamped, i1 clamped); extra = 0, 1, 5; D = 4, 48.
  hct_gather_augment       S = 12, B * C = 4096: gather_augment_kernel<4>, one block per volume, two trips (432 threads' work); S = 16 with
                           the pool 8-byte aligned: <4> on rows that would allow <8>.  (tests/test_affine_gpu.py::test_more_than_one_trip
                           drives hct_affine_augment, not this entry point.)
  hct_crop_resize_area     F = 2052 and 2048 refused: F * F * (F / 4) no longer fits the int the kernel counts its threads in.

Bit-equality is asked where the arithmetic is exact (index remaps, casts, one IEEE operation per element, weights of exactly 0 and 1).
The resample, contrast and position-table cases are held to the bars the project already holds those kernels to.  The Gaussian filter is
held element by element to `volume_ref.gaussian_bound`, derived from the kernel's order of operations; no element is left out.

Measured on an MI355X: worst |got - ref| / bound over every Gaussian case 0.117 (S 8, C 3, Gaussian input); 0.064 on the impulses.

Every output is NaN-filled (integers: a sentinel) between guard bands that must come back untouched, every call is made twice on fresh
outputs that must agree bit for bit, and a refusal returns HCT_E_BADARG and writes nothing.  Inputs whose neighbourhood a kernel could
read by mistake (the Gaussian input, the position table, the pool, the workspaces) lie between NaN bands too."""
import ctypes as C

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib, nifti
from headct_foundation_amd._lib import HCT_F16, HCT_F32
from headct_foundation_amd.data import gaussian_taps
from tests import loading_ref as L
from tests import volume_ref as V
from tests.test_assembly_kernels_gpu import _Out, _bits, _p, _st, _twice
from tests.test_dino_aug_gpu import TOL as DINO_TOL
from tests.test_loading_gpu import _assert_item

pytestmark = pytest.mark.gpu

F32, F16, I32 = torch.float32, torch.float16, torch.int32
HCT_E_BADARG = -1
GAUSS_WORST = {"ratio": 0.0}


def _banded(x, dev, band=256):
    """x on the device between two NaN bands (floating point only); the view keeps 512-byte alignment for band = 256."""
    buf = torch.full((x.numel() + 2 * band,), float("nan"), dtype=x.dtype, device=dev)
    buf[band:band + x.numel()] = x.reshape(-1).to(dev)
    return buf, buf[band:band + x.numel()].view(x.shape)


def _refused(lib, rc, name, outs):
    torch.cuda.synchronize()
    assert rc == HCT_E_BADARG and name.encode() in lib.hct_last_error_string(), (name, rc)
    for o in outs:
        o.result()
        assert o.untouched(), name


# ---- hct_volume_to_ras ----------------------------------------------------------------------------------------------------------------
def _to_ras(lib, cuda, stored, perm, flip, slope, inter):
    raw = torch.from_numpy(np.ascontiguousarray(stored.transpose(2, 1, 0)).view(np.uint8).reshape(-1)).to(cuda)
    ni, nj, nk = stored.shape
    d = [stored.shape[int(perm[o])] for o in range(3)]
    c3 = C.c_int * 3

    def run():
        o = _Out(d, F32, cuda)
        rc = lib.hct_volume_to_ras(raw.data_ptr(), L.NIFTI_CODES[stored.dtype.name][0], ni, nj, nk, c3(*[int(p) for p in perm]),
                                   c3(*[int(f) for f in flip]), int(slope is not None), float(slope or 0.0), float(inter or 0.0), o.ptr, _st())
        assert rc == 0, lib.hct_last_error_string()
        o.keep = raw
        return {"out": o}
    return _twice(run)["out"].numpy()


@pytest.mark.parametrize("dtype", V.RAS_DTYPES)
def test_volume_to_ras_second_tiles_and_second_block(lib, cuda, dtype):
    for shape, orders in ((V.RAS_TILED_SHAPE, V.ras_orders(dtype)), (V.RAS_LONG_SHAPE, V.RAS_LONG_ORDERS)):
        data = V.ras_data(dtype, shape)
        for out_of, sign in orders:
            stored, saff = L.stored_as(data, np.diag([0.5, 0.75, 2.5, 1.0]), out_of, sign)
            perm, flip, _, _ = nifti.ras_axes(saff, stored.shape)
            for slope, inter in V.RAS_SCALINGS:
                got = _to_ras(lib, cuda, stored, perm, flip, slope, inter)
                want = L.scaled(V.transpose_flip(stored, perm, flip), slope, inter)
                assert V.bits_equal(got, want), (dtype, shape, out_of, sign, slope)
                assert V.bits_equal(got, L.scaled(data, slope, inter))


# ---- hct_bspline3_resample ------------------------------------------------------------------------------------------------------------
def _resample_tables(shape, zooms, cuda):
    geom = [nifti.spacing_geometry(shape[a], zooms[a]) for a in range(3)]
    m = [g[0] for g in geom]
    tables = [nifti.bspline3_tables(shape[a], m[a], geom[a][1]) for a in range(3)]
    base = torch.from_numpy(np.concatenate([t[0] for t in tables])).to(cuda)
    w = torch.from_numpy(np.concatenate([t[1].reshape(-1) for t in tables])).to(cuda)
    return m, base, w


def _resample(lib, cuda, values, zooms):
    d = list(values.shape)
    m, base, w = _resample_tables(d, zooms, cuda)
    x = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(cuda)

    def run():
        o = _Out(m, F32, cuda)
        ws = torch.full((lib.hct_bspline3_resample_workspace_bytes(*d, *m),), 255, dtype=torch.uint8, device=cuda)  # doubles of all ones: NaN
        rc = lib.hct_bspline3_resample(x.data_ptr(), *d, o.ptr, *m, base.data_ptr(), w.data_ptr(), ws.data_ptr(), ws.numel(), _st())
        assert rc == 0, lib.hct_last_error_string()
        o.keep = (ws, x, base, w)
        return {"out": o}
    return _twice(run)["out"].numpy()


@pytest.mark.parametrize("name", sorted(V.RESAMPLE_CASES))
def test_bspline3_resample_second_blocks_and_row_tails(lib, cuda, name):
    values, zooms = V.resample_input(name)
    want = L.resample_f64(values, zooms)
    bar = V.resample_bar(values, zooms, want)
    got = _resample(lib, cuda, values, zooms)
    err = float(np.abs(got - want).max()) if got.shape == want.shape else float("nan")
    print(f"{name}: {values.shape} -> {got.shape}: device vs scipy float64 max abs {err:.3g}, bar {bar:.3g}")
    assert V.resample_ok(got, want, bar), (name, err, bar)


def test_bspline3_resample_refuses_1025_beside_the_accepted_1024(lib, cuda):
    values, zooms = V.resample_input("longest axis accepted")
    d = list(values.shape)
    m, base, w = _resample_tables(d, zooms, cuda)
    assert m == [1, 1, V.MAX_AXIS]
    x = torch.zeros(2048, device=cuda)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    wide = torch.zeros(32 * 1027, dtype=torch.float64, device=cuda)
    ibase = torch.zeros(1027, dtype=torch.int32, device=cuda)
    for dims in ((1, 1, 512, 1, 1, 1025), (1, 1, 1025, 1, 1, 512)):
        o = _Out(dims[3:], F32, cuda)
        rc = lib.hct_bspline3_resample(x.data_ptr(), *dims[:3], o.ptr, *dims[3:], ibase.data_ptr(), wide.data_ptr(), ws.data_ptr(), ws.numel(), _st())
        _refused(lib, rc, "hct_bspline3_resample", [o])


# ---- hct_foreground_bbox --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.BBOX_CASES))
def test_foreground_bbox_finds_a_lone_voxel_in_every_trip_and_lane(lib, cuda, name):
    shape, (row, z) = V.BBOX_CASES[name]
    vol = V.bbox_volume(name)
    vd = torch.from_numpy(vol).to(cuda)

    def run():
        box, status = _Out((6,), I32, cuda), _Out((1,), I32, cuda)
        ws = torch.full((lib.hct_foreground_bbox_workspace_bytes(*shape),), 255, dtype=torch.uint8, device=cuda)  # -1 where a block wrote nothing
        rc = lib.hct_foreground_bbox(vd.data_ptr(), *shape, box.ptr, status.ptr, ws.data_ptr(), ws.numel(), _st())
        assert rc == 0, lib.hct_last_error_string()
        box.keep = ws
        return {"box": box, "status": status}
    got = _twice(run)
    (start, size), status = L.foreground_box(vol), 0
    assert (got["box"].tolist(), got["status"].tolist()) == (list(start) + list(size), [status]), name
    assert got["box"].tolist() == [row // shape[1], row % shape[1], z, 1, 1, 1]


# ---- hct_crop_window_resize_area ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.CWR_CASES))
def test_crop_window_resize_area_two_and_four_windows(lib, cuda, name):
    box, roi, w = V.CWR_CASES[name]
    vol = V.cwr_volume()
    vd = torch.from_numpy(vol).to(cuda)
    lo = torch.tensor([t[0] for t in V.WINDOWS[w]], dtype=F32, device=cuda)
    hi = torch.tensor([t[1] for t in V.WINDOWS[w]], dtype=F32, device=cuda)
    boxd = torch.tensor(list(box[0]) + list(box[1]), dtype=I32, device=cuda)

    def run():
        o = _Out((w,) + tuple(roi), F16, cuda)
        rc = lib.hct_crop_window_resize_area(vd.data_ptr(), *vol.shape, boxd.data_ptr(), w, lo.data_ptr(), hi.data_ptr(), o.ptr, *roi, _st())
        assert rc == 0, lib.hct_last_error_string()
        return {"out": o}
    _assert_item(_twice(run)["out"], V.window_resize_f64(vol, box, roi, V.WINDOWS[w]), name)


def test_crop_window_resize_area_refuses_five_windows(lib, cuda):
    vd = torch.zeros(4, 4, 4, device=cuda)
    t = torch.zeros(8, device=cuda)
    boxd = torch.tensor([0, 0, 0, 4, 4, 4], dtype=I32, device=cuda)
    for w in (0, 5):
        o = _Out((5, 4, 4, 4), F16, cuda)
        rc = lib.hct_crop_window_resize_area(vd.data_ptr(), 4, 4, 4, boxd.data_ptr(), w, t.data_ptr(), t.data_ptr(), o.ptr, 4, 4, 4, _st())
        _refused(lib, rc, "hct_crop_window_resize_area", [o])


# ---- hct_hu_window --------------------------------------------------------------------------------------------------------------------
def _hu_call(lib, cuda, hd, in_dtype, out_dtype, W, lo, hi):
    o = _Out((V.HU_BATCH, W, V.HU_VOXELS // 4, 4), out_dtype, cuda)
    code = {F32: HCT_F32, F16: HCT_F16}
    rc = lib.hct_hu_window(hd.data_ptr(), code[in_dtype], o.ptr, code[out_dtype], V.HU_BATCH, V.HU_VOXELS, W, lo.data_ptr(), hi.data_ptr(), _st())
    return rc, o


@pytest.mark.parametrize("W", V.HU_WINDOW_COUNTS)
def test_hu_window_second_pass_every_window_count_and_dtype_pair(lib, cuda, W):
    windows = V.WINDOWS[W]
    hu = V.hu_volume(windows)
    lo = torch.tensor([t[0] for t in windows], dtype=F32, device=cuda)
    hi = torch.tensor([t[1] for t in windows], dtype=F32, device=cuda)
    for in_dtype in (F32, F16):
        src = hu.to(in_dtype)
        hd = src.to(cuda)
        want = V.hu_window_f32(src, windows)
        for out_dtype in (F32, F16):
            def run():
                rc, o = _hu_call(lib, cuda, hd, in_dtype, out_dtype, W, lo, hi)
                assert rc == 0, lib.hct_last_error_string()
                return {"out": o}
            got = _twice(run)["out"].view(V.HU_BATCH, W, V.HU_VOXELS)
            assert torch.equal(_bits(got), _bits(want.to(out_dtype))), (W, in_dtype, out_dtype)
            assert float(got.float().min()) == 0.0 and float(got.float().max()) == 1.0


def test_hu_window_refuses_nine_windows_and_ragged_volumes(lib, cuda):
    hd = torch.zeros(V.HU_BATCH, V.HU_VOXELS + 4, device=cuda)
    t = torch.zeros(16, device=cuda)
    o = _Out((V.HU_BATCH, 9, V.HU_VOXELS // 4 + 1, 4), F16, cuda)  # room for whatever a launch would have written
    for W, voxels in ((9, V.HU_VOXELS), (0, V.HU_VOXELS), (3, V.HU_VOXELS + 2), (3, 0)):
        rc = lib.hct_hu_window(hd.data_ptr(), HCT_F32, o.ptr, HCT_F16, V.HU_BATCH, voxels, W, t.data_ptr(), (t + 1).data_ptr(), _st())
        _refused(lib, rc, "hct_hu_window", [o])


# ---- hct_adjust_contrast --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.CONTRAST_CASES))
def test_adjust_contrast_extrema_in_the_chunk_that_was_not_launched(lib, cuda, name):
    assert V.CONTRAST_TOL == DINO_TOL
    n, _, _, apply, gamma = V.CONTRAST_CASES[name]
    x = V.contrast_input(name)
    gd, ad = torch.tensor(gamma, dtype=F32, device=cuda), torch.tensor(apply, dtype=torch.uint8, device=cuda)
    need = lib.hct_adjust_contrast_workspace_bytes(2, n)
    assert need == 2 * V.contrast_chunks(n) * 8

    def run():
        o = _Out((2, n // 4, 4), F32, cuda)
        o.t.copy_(x.view(2, n // 4, 4))
        ws = torch.tensor([-1e30, 1e30], device=cuda).repeat(need // 8)  # a partial that no block wrote would win the minimum and the maximum
        rc = lib.hct_adjust_contrast(o.ptr, 2, n, gd.data_ptr(), ad.data_ptr(), ws.data_ptr(), need, _st())
        assert rc == 0, lib.hct_last_error_string()
        o.keep = ws
        return {"x": o}
    got = _twice(run)["x"].view(2, n)
    for b in range(2):
        if apply[b]:
            want = V.adjust_contrast_f64(x[b], gamma[b])
            err = float((got[b].double() - want.double()).abs().max())
            print(f"{name}: sample {b}: max abs err {err:.3g}, bar {V.CONTRAST_TOL:.3g}")
            assert V.contrast_ok(got[b], want), (name, b, err)
            assert float(got[b].min()) == pytest.approx(-0.2, abs=V.CONTRAST_TOL) and float(got[b].max()) == pytest.approx(1.2, abs=V.CONTRAST_TOL)
        else:
            assert torch.equal(_bits(got[b]), _bits(x[b])), (name, b)


# ---- hct_gaussian_smooth3d ------------------------------------------------------------------------------------------------------------
def _gaussian(lib, cuda, x, taps, fire):
    keep, xd = _banded(x, cuda)
    td, fd = taps.to(cuda), torch.tensor(fire, dtype=torch.uint8, device=cuda)

    def run():
        out, tmp = _Out(tuple(x.shape), F32, cuda), _Out(tuple(x.shape), F32, cuda)
        rc = lib.hct_gaussian_smooth3d(xd.data_ptr(), out.ptr, tmp.ptr, x.shape[0], x.shape[1], x.shape[2], td.data_ptr(), fd.data_ptr(), _st())
        assert rc == 0, lib.hct_last_error_string()
        out.keep = (keep, td, fd)
        return {"out": out, "tmp": tmp}
    return _twice(run)["out"]


def _held_to_the_bound(got, ref, bound, what):
    ok, ratio = V.within(got, ref, bound)
    GAUSS_WORST["ratio"] = max(GAUSS_WORST["ratio"], ratio)
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f} (worst so far {GAUSS_WORST['ratio']:.3f})")
    assert ok and bool(torch.isfinite(got).all()), (what, ratio)


@pytest.mark.parametrize("S,Cc", V.GAUSS_SHAPES)
def test_gaussian_smooth3d_within_the_derived_bound(lib, cuda, S, Cc):
    B = len(V.GAUSS_SIGMA)
    taps = gaussian_taps(torch.tensor(V.GAUSS_SIGMA))
    x = torch.randn(B, Cc, S, S, S, generator=torch.Generator().manual_seed(41 + S + Cc))
    got = _gaussian(lib, cuda, x, taps, V.GAUSS_FIRE)
    _held_to_the_bound(got, V.gaussian_f64(x, taps, V.GAUSS_FIRE), V.gaussian_bound(x, taps, V.GAUSS_FIRE), f"S {S} C {Cc}")
    for b, fire in enumerate(V.GAUSS_FIRE):
        assert fire != torch.equal(_bits(got[b]), _bits(x[b])), b  # a skipped sample is copied bit for bit, a filtered one is not
    nobody = _gaussian(lib, cuda, x, taps, [False] * B)
    assert torch.equal(_bits(nobody), _bits(x))
    # unit impulses: the response is the outer product of the three axes' taps (exchanged taps would be another response)
    everybody = [True] * B
    for name, at in V.gauss_impulses(S).items():
        imp = torch.zeros(B, Cc, S, S, S)
        imp[(slice(None), slice(None)) + tuple(at)] = 1.0
        got = _gaussian(lib, cuda, imp, taps, everybody)
        bound = V.gaussian_bound(imp, taps, everybody)
        want = torch.stack([V.impulse_response(taps[b], at, S) for b in range(B)])[:, None].expand(B, Cc, S, S, S)
        _held_to_the_bound(got, want, bound, f"S {S} C {Cc} impulse at the {name}")


def test_gaussian_smooth3d_refuses_aliased_buffers(lib, cuda):
    B, Cc, S = 2, 1, 8
    x = torch.randn(B, Cc, S, S, S, device=cuda)
    taps = gaussian_taps(torch.tensor([[0.5, 0.75, 1.0]] * B)).to(cuda)
    fire = torch.ones(B, dtype=torch.uint8, device=cuda)
    before = x.clone()
    a, b = _Out(tuple(x.shape), F32, cuda), _Out(tuple(x.shape), F32, cuda)
    for args in ((x.data_ptr(), x.data_ptr(), b.ptr), (x.data_ptr(), a.ptr, x.data_ptr()), (x.data_ptr(), a.ptr, a.ptr), (x.data_ptr(), a.ptr, None)):
        rc = lib.hct_gaussian_smooth3d(*args, B, Cc, S, taps.data_ptr(), fire.data_ptr(), _st())
        _refused(lib, rc, "hct_gaussian_smooth3d", [a, b])
    rc = lib.hct_gaussian_smooth3d(x.data_ptr(), a.ptr, b.ptr, B, Cc, 6, taps.data_ptr(), fire.data_ptr(), _st())
    _refused(lib, rc, "hct_gaussian_smooth3d", [a, b])
    assert torch.equal(x, before)


# ---- hct_pos_embed_interp3d -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs,gd", V.POS_GRIDS)
def test_pos_embed_interp3d_identity_single_tokens_and_extra_rows(lib, cuda, gs, gd):
    for extra in V.POS_EXTRA:
        for D in V.POS_D:
            t = V.pos_table(gs, extra, D)
            keep, src = _banded(t, cuda)

            def run():
                o = _Out((extra + gd ** 3, D), F32, cuda)
                rc = lib.hct_pos_embed_interp3d(src.data_ptr(), gs, o.ptr, gd, D, extra, _st())
                assert rc == 0, lib.hct_last_error_string()
                o.keep = keep
                return {"out": o}
            got = _twice(run)["out"]
            want = V.pos_interp_f64(t, gs, gd, extra)
            err = float((got.double() - want).abs().max())
            print(f"{gs} -> {gd}, extra {extra}, D {D}: max abs err {err:.3g}, bar {V.POS_TOL:.3g}")
            assert bool(torch.isfinite(got).all()) and err <= V.POS_TOL, (gs, gd, extra, D, err)
            assert torch.equal(_bits(got[:extra]), _bits(t[:extra]))
            if gs == gd:
                assert torch.equal(_bits(got), _bits(t))


# ---- hct_gather_augment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [V.GATHER_TRIPS_CASE, V.GATHER_NARROW_CASE], ids=["two trips", "pool 8-byte aligned"])
def test_gather_augment_second_trip_and_narrow_instance(lib, cuda, case):
    S, B, Cc, n = case["S"], case["B"], case["C"], case["n_slots"]
    pool, slot, flip, shift = V.gather_case(case)
    band = 256 + case["offset_halves"]
    buf = torch.full((pool.numel() + 2 * band,), float("nan"), dtype=F16, device=cuda)
    buf[band:band + pool.numel()] = pool.reshape(-1).to(cuda)
    pd = buf[band:band + pool.numel()]
    assert pd.data_ptr() % 16 == (2 * case["offset_halves"]) % 16 and pd.data_ptr() % 8 == 0
    sd, fd, hd = slot.to(cuda), flip.to(cuda), shift.to(cuda)
    for f, s in ((fd, hd), (fd, None)):
        def run():
            o = _Out((B, Cc, S, S, S), F32, cuda)
            rc = lib.hct_gather_augment(pd.data_ptr(), sd.data_ptr(), o.ptr, B, Cc, S, n, _p(f), _p(s), _st())
            assert rc == 0, lib.hct_last_error_string()
            o.keep = buf
            return {"out": o}
        got = _twice(run)["out"]
        want = V.gather_plain(pool, slot, flip, None if s is None else shift)
        assert torch.equal(_bits(got), _bits(want)), (case, s is None)


# ---- hct_crop_resize_area -------------------------------------------------------------------------------------------------------------
def test_crop_resize_area_refuses_an_f_whose_thread_count_overflows(lib, cuda):
    """The kernel counts a volume's F * F * (F / 4) threads, rounded up to whole blocks, in an int, which wraps beyond F = 2044: the entry
    point refuses such an F before it launches anything."""
    x = torch.rand(1, 1, 4, 4, 4, device=cuda)
    boxes = torch.tensor([0, 0, 0, 4, 4, 4], dtype=I32, device=cuda)
    for Fv in (2052, 2048, 4096):
        assert Fv > V.CROP_RESIZE_MAX_F
        o = _Out((64, 64), F32, cuda)
        rc = lib.hct_crop_resize_area(x.data_ptr(), HCT_F32, 1, 1, 4, o.ptr, Fv, 1, boxes.data_ptr(), None, None, _st())
        _refused(lib, rc, "hct_crop_resize_area", [o])
    o = _Out((1, 1, 8, 8, 8), F32, cuda)  # and the door is still open below
    _lib.check(lib.hct_crop_resize_area(x.data_ptr(), HCT_F32, 1, 1, 4, o.ptr, 8, 1, boxes.data_ptr(), None, None, _st()), "hct_crop_resize_area")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o.result()).all())
