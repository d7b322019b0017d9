"""No GPU: tests/volume_ref.py held to independent sources on the cases the GPU tests run (numpy transpose / flip, scipy's float64
spline, F.interpolate in float64, the oracle's Gaussian filter and HU windows), and every condition that
tests/test_volume_kernels_gpu.py relies on asserted from the references alone: that each case reaches the block, trip, chunk or
template instance it is named for (computed from the kernels' launch constants, restated in volume_ref), that a planted voxel is
the unique minimum, maximum or positive voxel of its volume, that the borrowed bars are met by the fp32 restatements, and that the
comparison each GPU test applies rejects the result of a subtly wrong kernel -- a block, trip or chunk never run, taps exchanged."""
import numpy as np
import pytest
import torch

from headct_foundation_amd import nifti
from headct_foundation_amd.data import GAUSS_TAPS, HU_WINDOWS, gaussian_taps
from oracle import mae_oracle as O
from tests import affine_ref
from tests import loading_ref as L
from tests import volume_ref as V


# ---- hct_volume_to_ras ----------------------------------------------------------------------------------------------------------------
def _ras_case(dtype, shape, out_of, sign):
    data = V.ras_data(dtype, shape)
    stored, saff = L.stored_as(data, np.diag([0.5, 0.75, 2.5, 1.0]), out_of, sign)
    perm, flip, _, _ = nifti.ras_axes(saff, stored.shape)
    return data, stored, perm, flip


@pytest.mark.parametrize("dtype", V.RAS_DTYPES)
def test_to_ras_restatement_is_transpose_and_flip(dtype):
    cases = [(V.RAS_TILED_SHAPE, o, s) for o, s in V.ras_orders(dtype)] + [(V.RAS_LONG_SHAPE, o, s) for o, s in V.RAS_LONG_ORDERS]
    assert len(V.ras_orders("int16")) == 48 and len(V.ras_orders(dtype)) >= 6
    for shape, out_of, sign in cases:
        data, stored, perm, flip = _ras_case(dtype, shape, out_of, sign)
        file_order = np.ascontiguousarray(stored.transpose(2, 1, 0)).reshape(-1)
        for slope, inter in V.RAS_SCALINGS:
            got = V.to_ras(file_order, stored.shape, perm, flip, slope, inter)
            assert V.bits_equal(got, L.scaled(V.transpose_flip(stored, perm, flip), slope, inter)), (dtype, out_of, sign, slope)
            assert V.bits_equal(got, L.scaled(data, slope, inter))


def test_to_ras_cases_reach_every_block_and_a_kernel_without_them_is_rejected():
    seen = set()
    for shape, orders in ((V.RAS_TILED_SHAPE, V.ras_orders("int16")), (V.RAS_LONG_SHAPE, V.RAS_LONG_ORDERS)):
        assert all(n % V.RAS_TILE for n in shape)
        for out_of, sign in orders:
            data, stored, perm, flip = _ras_case("int16", shape, out_of, sign)
            axis = V.ras_contiguous_axis(perm)
            blocks = V.ras_blocks(data.shape, axis)
            file_order = np.ascontiguousarray(stored.transpose(2, 1, 0)).reshape(-1)
            want = L.scaled(data, None, None)
            for name, b in blocks.items():
                for first in range(1, int(b.max()) + 1):
                    seen.add((axis, name, first, bool(flip[2]) if axis == 2 else None))
                    assert not V.bits_equal(V.to_ras(file_order, stored.shape, perm, flip, never_run=(name, first)), want)
    # the tile kernels: a second tile along the tiled axis, a second and a third along axis 2, for both instances
    assert {(a, n, f) for a, n, f, _ in seen if a != 2} == {(a, n, f) for a in (0, 1) for n, f in (("a", 1), ("z", 1), ("z", 2))}
    # the direct kernel: a second x-block (d[2] = 300 > 256), read forwards and backwards; d[2] = 65 stays in one block
    assert {(n, f, fl) for a, n, f, fl in seen if a == 2} == {("x", 1, False), ("x", 1, True)}
    assert V.RAS_LONG_SHAPE[2] > V.RAS_DIRECT_BLOCK and all(o[0] == 2 for o, _ in V.RAS_LONG_ORDERS)


# ---- hct_bspline3_resample ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.RESAMPLE_CASES))
def test_resample_cases_reach_their_blocks_and_the_bar_is_the_number_formats(name):
    """The bar of the GPU test is 4 x the fp32 FIR's error; that error is itself within the bound tests/test_loading_cpu.py derives
    from the number format, and not zero."""
    values, zooms = V.resample_input(name)
    m = V.resample_shape(values.shape, zooms)
    want = L.resample_f64(values, zooms)
    assert list(want.shape) == m and max(m) <= V.MAX_AXIS
    err = float(np.abs(L.resample_fir_f32(values, zooms) - want).max())
    bound = 3 * (L.TAPS + 2) * 2.0 ** -24 * 27 * float(np.abs(values).max()) + 1e-4
    print(f"{name}: {values.shape} -> {m}: fp32 FIR vs scipy float64 {err:.3g}, format bound {bound:.3g}")
    assert 0 < err <= bound
    blocks = V.resample_blocks(values.shape, m)
    rows = m[0] * m[1]
    if name.startswith("rows kernel"):
        assert m[2] == 300 and int(blocks["rows_y"].max()) == 1
        assert not V.resample_ok(V.resample_never_run(values, zooms, "rows_y"), want, V.resample_bar(values, zooms, want))
    if name.startswith("strided kernel"):
        assert values.shape[2] == 300 and int(blocks["mid_x"].max()) == 1 and m[1] != values.shape[1]
        assert not V.resample_ok(V.resample_never_run(values, zooms, "mid_x"), want, V.resample_bar(values, zooms, want))
    if name.startswith("row tail"):
        want_rows = {"1 row": 1, "2 rows": 2, "3 rows": 3}.get(name.split(", ")[1])
        assert rows == want_rows if want_rows else (rows > 4 and rows % 4 == 1)
    if name.startswith("longest"):
        assert m[2] == V.MAX_AXIS == nifti.MAX_AXIS
    assert V.resample_ok(L.resample_fir_f32(values, zooms), want, V.resample_bar(values, zooms, want))
    assert len([n for n in V.RESAMPLE_CASES if n.startswith("row tail")]) == 4


# ---- hct_foreground_bbox --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.BBOX_CASES))
def test_bbox_planted_voxel_is_alone_and_where_the_case_says(name):
    shape, (row, z) = V.BBOX_CASES[name]
    vol = V.bbox_volume(name)
    assert int((vol > 0).sum()) == 1 and vol.reshape(-1, shape[2])[row, z] > 0
    x, y = divmod(row, shape[1])
    want = ([[x, y, z], [1, 1, 1]], 0)
    assert V.foreground_box_as_run(vol) == want and list(L.foreground_box(vol)) == want[0]
    rows = shape[0] * shape[1]
    trip, block, lane_pass = V.bbox_place(shape, row, z)
    trips = -(-rows // (V.bbox_chunks(rows) * V.BOX_ROWS_PER_BLOCK))
    if shape == V.BBOX_TRIP_SHAPE:
        assert rows == 9100 and V.bbox_chunks(rows) == V.BOX_MAX_CHUNKS and trips == 3
        assert (trip, block) == {"row 0": (0, 0), "row 4095, last of the first trip": (0, 1023), "row 4096, first of the second trip": (1, 0),
                                 "last row, third trip": (2, (9099 - 8192) // 4)}[name]
        if trip > 0:  # a kernel that stops after the trip before never sees it, and says "empty"
            assert V.foreground_box_as_run(vol, max_trips=trip) != want
            assert V.foreground_box_as_run(vol, max_trips=trip + 1) == want
    elif name == "one chunk":
        assert V.bbox_chunks(rows) == 1 and trips == 1
    else:
        assert z == shape[2] - 1 and lane_pass == (shape[2] - 1) // V.WAVE and (z % V.WAVE) == (shape[2] - 1) % V.WAVE
        if lane_pass > 0:
            assert V.foreground_box_as_run(vol, max_lane_passes=lane_pass) != want
    assert sorted(s[2] for s, _ in V.BBOX_CASES.values() if s[:2] == (3, 5)) == [1, 63, 64, 65, 129]


def test_bbox_restatement_equals_numpy_on_a_scattered_foreground():
    g = np.random.default_rng(2)
    vol = g.standard_normal(V.BBOX_TRIP_SHAPE).astype(np.float32) - 3.2  # a few dozen positive voxels
    assert 3 < int((vol > 0).sum()) < 200
    assert V.foreground_box_as_run(vol) == (list(L.foreground_box(vol)), 0)
    assert V.foreground_box_as_run(-np.abs(vol)) == ([[0, 0, 0], list(V.BBOX_TRIP_SHAPE)], 1)


# ---- hct_crop_window_resize_area ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.CWR_CASES))
def test_crop_window_resize_cases_meet_the_rule_in_fp32(name):
    """The GPU test holds the kernel to `_assert_item` against the float64 restatement; the kernel's arithmetic in fp32 numpy meets
    that rule on the same case, so the rule is not what the case hangs on."""
    box, roi, w = V.CWR_CASES[name]
    vol = V.cwr_volume()
    a, b = V.window_resize_f64(vol, box, roi, V.WINDOWS[w]), V.window_resize_f32(vol, box, roi, V.WINDOWS[w])
    steps = L.fp16_steps(a, b)
    print(f"{name}: fp32 vs float64: {float((steps > 0).float().mean()):.3%} differ, max {int(steps.max())} step")
    assert a.shape == (w,) + tuple(roi) and V.item_rule(b, a)
    assert len(torch.unique(a)) > 2 * w  # nothing degenerate: the channels are not constants
    if not name.startswith("3 voxels"):
        assert all(len(torch.unique(a[c])) > 4 for c in range(w))
    assert all(s + n <= m for s, n, m in zip(box[0], box[1], V.CWR_VOLUME))
    if name.startswith("box ends"):
        assert all(s + n == m for s, n, m in zip(box[0], box[1], V.CWR_VOLUME))
    if name.startswith("3 voxels"):
        assert box[1] == (3, 3, 3) and roi == (8, 8, 8)
    # a wrong window table (two channels exchanged) or a window one voxel off does not pass the rule
    swapped = [V.WINDOWS[w][1], V.WINDOWS[w][0]] + V.WINDOWS[w][2:]
    assert not V.item_rule(V.window_resize_f64(vol, box, roi, swapped), a)
    moved = ((box[0][0], box[0][1], box[0][2] - 1), box[1])
    assert not V.item_rule(V.window_resize_f64(vol, moved, roi, V.WINDOWS[w]), a)


def test_crop_window_resize_restatements_agree_with_the_existing_one():
    vol = V.cwr_volume()
    box, roi = ((2, 3, 4), (13, 14, 29)), (5, 6, 9)
    for chans in (1, 3):
        assert V.WINDOWS[chans] == [tuple(float(v) for v in w) for w in HU_WINDOWS[chans]]
        assert V.item_rule(V.window_resize_f64(vol, box, roi, V.WINDOWS[chans]), L.window_resize(vol, box, roi, chans))
    assert sorted({c[1][2] for n, c in V.CWR_CASES.items() if n.startswith("R2")}) == [1, 5, 8, 9, 15]
    assert {c[2] for c in V.CWR_CASES.values()} == {2, 4}


# ---- hct_hu_window --------------------------------------------------------------------------------------------------------------------
def test_hu_window_restatement_is_the_oracle_and_the_case_takes_a_second_pass():
    assert V.HU_VOXELS % 4 == 0 and V.hu_passes(V.HU_VOXELS) == (2, 257)  # block 0 whole and one thread of block 1
    assert V.hu_passes(V.HU_MAX_BLOCKS * 256 * 4) == (1, V.HU_MAX_BLOCKS * 256) and V.hu_passes(1536) == (1, 384)
    for W in V.HU_WINDOW_COUNTS:
        windows = V.WINDOWS[W]
        hu = V.hu_volume(windows)
        edges = V.hu_edges(windows)
        first, tail = hu[0, :V.HU_MAX_BLOCKS * 1024].tolist(), hu[0, V.HU_MAX_BLOCKS * 1024:].tolist()
        assert len(tail) == 4 * 257 and all(e in first[:len(edges)] and e in tail for e in edges)
        assert all(float(lo) in edges and float(hi) in edges for lo, hi in windows if lo == int(lo) and hi == int(hi))
        assert torch.equal(hu, hu.round()) and torch.equal(hu.half().float().round(), hu.half().float())
        want = V.hu_window_f32(hu, windows)
        assert want.shape == (V.HU_BATCH, W, V.HU_VOXELS) and float(want.min()) == 0.0 and float(want.max()) == 1.0
        if W in HU_WINDOWS:
            assert torch.equal(want, O.hu_window(hu[:, None], W))
        broken = V.hu_window_f32(hu, windows, skip_second_pass=True)
        assert not V.bits_equal(broken.numpy(), want.numpy()) and not V.bits_equal(broken.half().numpy(), want.half().numpy())
        assert V.bits_equal(broken[:, :, :V.HU_MAX_BLOCKS * 1024].numpy(), want[:, :, :V.HU_MAX_BLOCKS * 1024].numpy())


# ---- hct_adjust_contrast --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.CONTRAST_CASES))
def test_contrast_extrema_are_unique_and_in_the_last_chunk(name):
    n, at_min, at_max, apply, gamma = V.CONTRAST_CASES[name]
    x = V.contrast_input(name)
    assert n % 4 == 0 and sum(apply) == 1
    for b in range(2):
        assert int(x[b].argmin()) == at_min and int(x[b].argmax()) == at_max
        assert int((x[b] == x[b].min()).sum()) == 1 and int((x[b] == x[b].max()).sum()) == 1
        assert float(x[b].min()) == pytest.approx(-0.2) and float(x[b].max()) == pytest.approx(1.2)
    if n == 4:
        assert V.contrast_chunks(n) == 1
        return
    assert (n // 4 + 1023) // 1024 == 257 and V.contrast_chunks(n) == V.CONTRAST_MAX_CHUNKS
    first, last = min(at_min, at_max), max(at_min, at_max)
    assert first == V.CONTRAST_TAIL and last == n - 1
    # 256 blocks of 256 threads cover 262,144 values per trip; what a 257th chunk would have held is the fifth trip of blocks 0 ... 3
    assert V.contrast_place(n, first) == (4, 0, 0) and V.contrast_place(n, last) == (4, 3, 255) and V.contrast_place(n, first - 1)[0] == 3
    b = apply.index(1)
    want = V.adjust_contrast_f64(x[b], gamma[b])
    dropped = V.adjust_contrast_f64(x[b], gamma[b], seen=V.CONTRAST_TAIL)  # a kernel that drops the last chunk from min / max
    assert V.contrast_ok(want, want) and not V.contrast_ok(dropped, want)
    assert not V.contrast_ok(V.adjust_contrast_f64(x[b], gamma[b], applied=V.CONTRAST_TAIL), want)  # ... or from the curve
    assert V.contrast_ok(V.adjust_contrast_f64(x[b], gamma[b], seen=n, applied=n), want)
    from tests import dino_aug_ref as D
    assert V.contrast_ok(D.adjust_contrast_fp32(x[b], gamma[b]), want)  # the fp32 formula on the CPU meets the bar on this input


# ---- hct_gaussian_smooth3d ------------------------------------------------------------------------------------------------------------
def _gauss_input(S, C, seed=41):
    return torch.randn(len(V.GAUSS_SIGMA), C, S, S, S, generator=torch.Generator().manual_seed(seed + S + C))


@pytest.mark.parametrize("S,C", V.GAUSS_SHAPES)
def test_gaussian_restatement_against_the_oracle_within_the_bound(S, C):
    """The oracle filters with F.conv3d in fp32: nine products and eight additions per pass in some order, which the derivation of
    `gaussian_bound` covers as well (a term passes through at most nine roundings in any order)."""
    assert V.GAUSS_TAPS == GAUSS_TAPS and all(len(set(s)) == 3 for s in V.GAUSS_SIGMA)
    assert V.GAUSS_FIRE[0] is False and V.GAUSS_FIRE[-1] is False and any(V.GAUSS_FIRE)
    x = _gauss_input(S, C)
    taps = gaussian_taps(torch.tensor(V.GAUSS_SIGMA))
    ref, bound = V.gaussian_f64(x, taps, V.GAUSS_FIRE), V.gaussian_bound(x, taps, V.GAUSS_FIRE)
    ok, ratio = V.within(O.gaussian_smooth3d(x, V.GAUSS_SIGMA, V.GAUSS_FIRE), ref, bound)
    print(f"S {S} C {C}: oracle (fp32 conv3d) vs float64: worst |err| / bound {ratio:.3f}")
    assert ok
    for b, fire in enumerate(V.GAUSS_FIRE):
        assert fire or (torch.equal(ref[b], x[b].double()) and float(bound[b].max()) == 0.0)
    # exchanged taps are far outside the bound
    for axes in ((2, 1, 0), (1, 0, 2), (0, 2, 1)):
        assert not V.within(V.gaussian_f64(x, taps, V.GAUSS_FIRE, axes).float(), ref, bound)[0], axes


@pytest.mark.parametrize("S", sorted({s for s, _ in V.GAUSS_SHAPES}))
def test_gaussian_impulse_response_is_the_outer_product_of_the_taps(S):
    taps = gaussian_taps(torch.tensor(V.GAUSS_SIGMA))
    fire = [True] * len(V.GAUSS_SIGMA)
    for name, at in V.gauss_impulses(S).items():
        x = torch.zeros(len(V.GAUSS_SIGMA), 1, S, S, S)
        x[(slice(None), 0) + tuple(at)] = 1.0
        assert int((x[0] != 0).sum()) == 1 and all(0 <= p < S for p in at)
        ref, bound = V.gaussian_f64(x, taps, fire), V.gaussian_bound(x, taps, fire)
        for b in range(len(V.GAUSS_SIGMA)):
            want = V.impulse_response(taps[b], at, S)
            assert float((ref[b, 0] - want).abs().max()) <= 1e-16, (name, b)
            assert float(want.max()) > 0.01 and V.within(want.float(), want, bound[b, 0])[0]
            for axes in ((2, 1, 0), (1, 0, 2), (0, 2, 1)):  # exchanged taps: another response, by far more than the bound
                wrong = V.impulse_response(taps[b][list(axes)], at, S)
                assert not V.within(wrong.float(), want, bound[b, 0])[0], (name, b, axes)


# ---- hct_pos_embed_interp3d -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs,gd", V.POS_GRIDS)
def test_pos_embed_restatement_against_the_oracle_index_arithmetic(gs, gd):
    """F.interpolate in float64 against the oracle's explicit fp32 index arithmetic (the kernel's): within the project's 2e-6, which
    is therefore wide enough for fp32 coordinates on these grids; identity and the extra rows exact."""
    for extra in V.POS_EXTRA:
        for D in V.POS_D:
            t = V.pos_table(gs, extra, D)
            assert float(t.min()) >= -1 and float(t.max()) < 1 and t.shape == (extra + gs ** 3, D)
            want = V.pos_interp_f64(t, gs, gd, extra)
            got = O.interpolate_pos_embed_3d(t[None], gd, extra)[0]
            assert want.shape == (extra + gd ** 3, D) and float((got.double() - want).abs().max()) <= V.POS_TOL / 2
            assert torch.equal(want[:extra], t[:extra].double())
            if gs == gd:
                assert torch.equal(want, t.double())
            if gs == 1:
                assert float((want[extra:] - t[extra:].double()).abs().max()) <= 1e-15  # weights that sum to one, on one token
            # rows read one place off (the extra rows not skipped) do not pass
            if gs > 1:
                shifted = V.pos_interp_f64(torch.cat([t[extra:extra + 1], t[:-1]]), gs, gd, extra)
                assert float((shifted - want)[extra:].abs().max()) > V.POS_TOL


# ---- hct_gather_augment ---------------------------------------------------------------------------------------------------------------
def test_gather_cases_take_two_trips_and_the_narrow_instance():
    c = V.GATHER_TRIPS_CASE
    assert c["B"] * c["C"] == V.GATHER_BLOCKS and V.gather_launch(c["S"], c["B"], c["C"], True) == (4, 432, 1, 2)
    pool, slot, flip, shift = V.gather_case(c)
    assert sorted(set(slot.tolist())) == [0, 1, 2] and sorted(set(flip.tolist())) == list(range(8))
    assert {(int(s), int(f)) for s, f in zip(slot, flip)} == {(s, f) for s in range(3) for f in range(8)}  # every slot under every flip
    want = V.gather_plain(pool, slot, flip, shift)
    assert want.shape == (c["B"], c["C"]) + (c["S"],) * 3 and want.numel() * 4 < 30e6
    one_trip = V.gather_plain(pool, slot, flip, shift, max_trips=1)
    assert not V.bits_equal(one_trip.numpy(), want.numpy()) and int(torch.isnan(one_trip[0, 0]).sum()) == (432 - 256) * 4
    n = V.GATHER_NARROW_CASE
    assert n["S"] % 8 == 0 and n["offset_halves"] * 2 % 16 == 8
    assert V.gather_launch(n["S"], n["B"], n["C"], True)[0] == 8 and V.gather_launch(n["S"], n["B"], n["C"], False) == (4, 1024, 4, 1)
    assert sorted(set(V.gather_case(n)[2].tolist())) == list(range(8))
    # the restatement is plain indexing
    x = pool[slot.long()][:16]
    got = affine_ref.plain(x, flip[:16], shift[:16])
    for b in range(16):
        dims = [a for a in range(3) if (int(flip[b]) >> a) & 1]
        assert torch.equal(got[b], (x[b].float().flip([d + 1 for d in dims]) if dims else x[b].float()) + shift[b])


# ---- hct_crop_resize_area -------------------------------------------------------------------------------------------------------------
def test_crop_resize_area_thread_count_fits_an_int_up_to_2044():
    int_max = 2 ** 31 - 1
    fits = lambda F: F * F * (F // 4) + 255 <= int_max
    assert fits(V.CROP_RESIZE_MAX_F) and not fits(V.CROP_RESIZE_MAX_F + 4) and not fits(2052) and V.CROP_RESIZE_MAX_F % 4 == 0
    assert 2048 * 2048 * 512 == int_max + 1  # 2048 itself already wraps
