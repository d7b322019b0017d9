"""The loading chain on the device against its restatement (tests/loading_ref.py): each kernel of csrc/loading.hip on its own, then
`load_volume` of written NIfTI files end to end, the cache, and the two pre-training entry points fed from a CSV of phantom files.
The conditions under which the end-to-end comparison with the float64 chain is meaningful (box not hanging on a rounding, fp32
restatement within a quarter of the allowance) are asserted for the same cases in tests/test_loading_cpu.py."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib, nifti
from headct_foundation_amd.data import HU_WINDOWS, VolumeCache, load_volume
from tests import loading_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernels through the C ABI --------------------------------------------------------------------------------------------------
def _to_ras(lib, cuda, stored, perm, flip, slope=None, inter=None):
    """stored [i, j, k] -> device fp32 RAS volume; the kernel takes the file order (axis i contiguous)."""
    raw = torch.from_numpy(np.ascontiguousarray(stored.transpose(2, 1, 0)).view(np.uint8).reshape(-1)).to(cuda)
    ni, nj, nk = stored.shape
    d = [stored.shape[perm[o]] for o in range(3)]
    out = torch.full(d, float("nan"), dtype=torch.float32, device=cuda)
    c3 = C.c_int * 3
    _lib.check(lib.hct_volume_to_ras(raw.data_ptr(), R.NIFTI_CODES[stored.dtype.name][0], ni, nj, nk, c3(*perm), c3(*[int(f) for f in flip]),
                                     int(slope is not None), float(slope or 0.0), float(inter or 0.0), out.data_ptr(), _lib.stream_ptr()),
               "hct_volume_to_ras")
    return out


def _resample(lib, cuda, values, zooms):
    d = list(values.shape)
    geom = [nifti.spacing_geometry(d[a], zooms[a]) for a in range(3)]
    m = [g[0] for g in geom]
    tables = [nifti.bspline3_tables(d[a], m[a], geom[a][1]) for a in range(3)]
    base = torch.from_numpy(np.concatenate([t[0] for t in tables])).to(cuda)
    w = torch.from_numpy(np.concatenate([t[1].reshape(-1) for t in tables])).to(cuda)
    x = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(cuda)
    out = torch.full(m, float("nan"), dtype=torch.float32, device=cuda)
    ws = torch.empty(lib.hct_bspline3_resample_workspace_bytes(*d, *m), dtype=torch.uint8, device=cuda)
    _lib.check(lib.hct_bspline3_resample(x.data_ptr(), *d, out.data_ptr(), *m, base.data_ptr(), w.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr()), "hct_bspline3_resample")
    return out


def _bbox(lib, cuda, vol):
    m = list(vol.shape)
    box = torch.full((8,), -7, dtype=torch.int32, device=cuda)
    ws = torch.empty(lib.hct_foreground_bbox_workspace_bytes(*m), dtype=torch.uint8, device=cuda)
    _lib.check(lib.hct_foreground_bbox(vol.data_ptr(), *m, box.data_ptr(), box.data_ptr() + 24, ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "hct_foreground_bbox")
    b = box.cpu().tolist()
    return (b[:3], b[3:6]), b[6]


def _window_resize(lib, cuda, vol, box, roi, chans):
    lo = torch.tensor([w[0] for w in HU_WINDOWS[chans]], dtype=torch.float32, device=cuda)
    hi = torch.tensor([w[1] for w in HU_WINDOWS[chans]], dtype=torch.float32, device=cuda)
    boxd = torch.tensor(list(box[0]) + list(box[1]), dtype=torch.int32, device=cuda)
    out = torch.full((chans,) + tuple(roi), float("nan"), dtype=torch.float16, device=cuda)
    _lib.check(lib.hct_crop_window_resize_area(vol.data_ptr(), *vol.shape, boxd.data_ptr(), chans, lo.data_ptr(), hi.data_ptr(), out.data_ptr(),
                                               *roi, _lib.stream_ptr()), "hct_crop_window_resize_area")
    return out


def _apply(stored, perm, flip):
    out = np.transpose(stored, perm)
    for o in range(3):
        if flip[o]:
            out = np.flip(out, axis=o)
    return np.ascontiguousarray(out)


def _assert_item(got, want, what):
    """Within one fp16 step everywhere, equal on at least 99.5 % of the voxels."""
    assert got.shape == want.shape and got.dtype == torch.float16 and bool(torch.isfinite(got.float()).all()), what
    steps = R.fp16_steps(got, want)
    share = float((steps == 0).float().mean())
    print(f"{what}: {1 - share:.3%} of voxels differ, max {int(steps.max())} fp16 step")
    assert int(steps.max()) <= 1 and share >= R.EQUAL_SHARE, what


@pytest.mark.parametrize("dtype", ["int16", "uint8", "int32", "float32", "float64", "int8", "uint16"])
def test_volume_to_ras_is_bit_equal(lib, cuda, dtype):
    """Every axis order and flip (all 48 for int16, six for the other types), scaled in float64 and cast like nibabel + MONAI, and
    unscaled: the shape is no multiple of the 32 x 32 tile."""
    g = np.random.default_rng(3)
    shape = (37, 50, 19)
    if np.dtype(dtype).kind == "f":
        data = (g.standard_normal(shape) * 900).astype(dtype)
    else:
        info = np.iinfo(dtype)
        data = g.integers(info.min, int(info.max) + 1, size=shape).astype(dtype)
    cases = R.SIGNED_PERMUTATIONS if dtype == "int16" else R.SIGNED_PERMUTATIONS[::9] + [R.SIGNED_PERMUTATIONS[-1]]
    for out_of, sign in cases:
        stored, saff = R.stored_as(data, np.diag([0.5, 0.75, 2.5, 1.0]), out_of, sign)
        perm, flip, _, _ = nifti.ras_axes(saff, stored.shape)
        for slope, inter in ((None, None), (0.4878, -1024.25)):
            got = _to_ras(lib, cuda, stored, perm, flip, slope, inter).cpu().numpy()
            want = R.scaled(_apply(stored, perm, flip), slope, inter)
            assert got.shape == data.shape and np.array_equal(got, want), (dtype, out_of, sign, slope)
            if slope is None:
                assert np.array_equal(got, data.astype(np.float32))


@pytest.mark.parametrize("name", sorted(R.PHANTOMS))
def test_bspline3_resample_against_scipy(lib, cuda, name):
    """Bar: four times the error of the fp32 numpy restatement on the same input (summation order, fused multiply-adds)."""
    _, values, zooms, _ = R.phantom_ras(name)
    want = R.resample_f64(values, zooms)
    bar = 4 * float(np.abs(R.resample_fir_f32(values, zooms) - want).max())
    got = _resample(lib, cuda, values, zooms).cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    print(f"{name}: {values.shape} -> {got.shape}: device vs scipy float64 max abs {err:.3g} HU, bar {bar:.3g}")
    assert err <= bar
    again = _resample(lib, cuda, values, zooms).cpu().numpy()
    assert np.array_equal(got, again)  # fixed order


def test_bspline3_resample_degenerate_axes_and_refusals(lib, cuda):
    g = np.random.default_rng(0)
    for shape, zooms in (((9, 1, 7), (0.3, 2.0, 1.0)), ((1, 1, 40), (1.0, 1.0, 0.5)), ((3, 70, 1), (4.0, 1.7, 1.0))):
        values = (g.standard_normal(shape) * 300).astype(np.float32)
        want = R.resample_f64(values, zooms)
        bar = 4 * float(np.abs(R.resample_fir_f32(values, zooms) - want).max())
        got = _resample(lib, cuda, values, zooms).cpu().numpy()
        assert got.shape == want.shape and float(np.abs(got - want).max()) <= bar, shape
    x = torch.zeros(8, device=cuda)
    for dims in ((1025, 1, 1, 4, 1, 1), (4, 1, 1, 1025, 1, 1), (4, 0, 1, 4, 1, 1)):
        assert lib.hct_bspline3_resample(x.data_ptr(), *dims[:3], x.data_ptr() + 16, *dims[3:], x.data_ptr(), x.data_ptr(), x.data_ptr(), 1 << 30,
                                         _lib.stream_ptr()) == -1


def test_foreground_bbox_equals_the_restatement(lib, cuda):
    for name in sorted(R.PHANTOMS):
        _, values, zooms, _ = R.phantom_ras(name)
        vol = R.resample_fir_f32(values, zooms)
        (start, size), status = _bbox(lib, cuda, torch.from_numpy(vol).to(cuda))
        assert ([start, size], status) == (list(R.foreground_box(vol)), 0), name
    g = np.random.default_rng(1)
    vol = -np.abs(g.standard_normal((33, 70, 129))).astype(np.float32)
    vol[5, 6, 7] = 0.0  # not > 0
    (start, size), status = _bbox(lib, cuda, torch.from_numpy(vol).to(cuda))
    assert status == 1 and (start, size) == ([0, 0, 0], [33, 70, 129])  # empty: flagged, the box stays in range
    vol[31, 2, 128] = 1e-30
    assert _bbox(lib, cuda, torch.from_numpy(vol).to(cuda)) == (([31, 2, 128], [1, 1, 1]), 0)
    vol[2, 69, 0] = 3.0
    vol[4, 4, 4] = float("nan")  # compares false, as in numpy
    assert _bbox(lib, cuda, torch.from_numpy(vol).to(cuda)) == (([2, 2, 0], [30, 68, 129]), 0)
    assert list(R.foreground_box(vol)) == [[2, 2, 0], [30, 68, 129]]


@pytest.mark.parametrize("name,roi,chans", R.END_TO_END_CASES + [("fine", (96, 96, 96), 3), ("thick", (5, 9, 13), 1)])
def test_crop_window_resize_area_on_the_same_fp32_input(lib, cuda, name, roi, chans):
    _, values, zooms, _ = R.phantom_ras(name)
    vol = R.resample_fir_f32(values, zooms)
    box = R.foreground_box(vol)
    got = _window_resize(lib, cuda, torch.from_numpy(vol).to(cuda), box, roi, chans)
    _assert_item(got, R.window_resize(vol, box, roi, chans), f"{name} {roi} x {chans}")


def test_crop_window_resize_area_confines_a_bad_box(lib, cuda):
    vol = torch.rand(10, 11, 12, device=cuda) * 100
    got = _window_resize(lib, cuda, vol, ([-5, 9, 20], [4, 100, 0]), (8, 8, 8), 1)
    assert bool(torch.isfinite(got.float()).all())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _write_phantom(path, name, out_of=(0, 1, 2), sign=(1, 1, 1), tilt=None, form="sform", byteorder="<"):
    raw, values, zooms, aff = R.phantom_ras(name)
    stored, saff = R.stored_as(raw, aff if tilt is None else R.tilted(aff, tilt), out_of, sign)
    R.write_nifti(path, stored, saff, slope=R.INT16_SLOPE, inter=R.INT16_INTER, form=form, byteorder=byteorder)
    held = (aff if tilt is None else R.tilted(aff, tilt))[:3, :3].astype(np.float32).astype(np.float64)  # the header holds float32
    return values, [float(z) for z in np.sqrt((held * held).sum(0))]


@pytest.mark.parametrize("name,roi,chans", R.END_TO_END_CASES)
def test_load_volume_against_the_float64_chain(cuda, tmp_path, name, roi, chans):
    values, zooms = _write_phantom(tmp_path / "p.nii.gz", name)
    got = load_volume(tmp_path / "p.nii.gz", roi, chans, cuda)
    assert got.device.type == "cuda" and got.shape == (chans,) + tuple(roi)
    _assert_item(got, R.chain(values, zooms, roi, chans), f"{name} {roi} x {chans}")


def test_reoriented_files_give_the_item_of_their_ras_twin(cuda, tmp_path):
    roi, chans = (32, 32, 32), 3
    _write_phantom(tmp_path / "ras.nii", "thick")
    twin = load_volume(tmp_path / "ras.nii", roi, chans, cuda)
    variants = [dict(out_of=(0, 1, 2), sign=(-1, -1, 1)), dict(out_of=(1, 0, 2), sign=(1, -1, -1)), dict(out_of=(2, 1, 0), sign=(-1, 1, 1)),
                dict(out_of=(1, 2, 0), sign=(1, 1, -1), byteorder=">"), dict(out_of=(2, 0, 1), sign=(-1, -1, -1), form="qform")]
    for i, kw in enumerate(variants):
        _write_phantom(tmp_path / f"v{i}.nii.gz", "thick", **kw)
        got = load_volume(tmp_path / f"v{i}.nii.gz", roi, chans, cuda)
        if kw.get("form") == "qform":  # the quaternion round trip moves the zooms by rounding
            _assert_item(got, twin, f"variant {i}")
        else:
            assert torch.equal(got, twin), kw
    # a tilted frame: same axes, same zooms up to rounding, the tilt stays in the affine
    values, zooms = _write_phantom(tmp_path / "tilt.nii", "thick", out_of=(0, 1, 2), sign=(-1, -1, 1), tilt=15.0)
    _assert_item(load_volume(tmp_path / "tilt.nii", roi, chans, cuda), R.chain(values, zooms, roi, chans), "tilted")


def test_constant_volume_empty_foreground_and_refusals(cuda, tmp_path):
    aff = np.diag([0.6, 0.7, 2.0, 1.0])
    R.write_nifti(tmp_path / "const.nii", np.full((40, 37, 11), 50, np.uint8), aff)
    for chans in (1, 3):
        got = load_volume(tmp_path / "const.nii", (16, 24, 8), chans, cuda)
        for c, (lo, hi) in enumerate(HU_WINDOWS[chans]):
            want = torch.tensor(min(max((50.0 - lo) / (hi - lo), 0.0), 1.0)).to(torch.float16)
            assert bool((got[c].cpu() == want).all()), (chans, c)
    R.write_nifti(tmp_path / "air.nii", np.full((20, 20, 9), -1000, np.int16), aff)
    with pytest.raises(ValueError, match="empty foreground"):
        load_volume(tmp_path / "air.nii", (16, 16, 16), 1, cuda)
    R.write_nifti(tmp_path / "two.nii", np.full((20, 20, 9), 5, np.int16), aff, n_volumes=2)
    with pytest.raises(ValueError, match="two.nii"):
        load_volume(tmp_path / "two.nii", (16, 16, 16), 1, cuda)


def test_second_call_is_served_from_the_cache(cuda, tmp_path):
    _write_phantom(tmp_path / "p.nii.gz", "thick")
    cache = VolumeCache(tmp_path / "cache", (32, 32, 32), 1)
    first = cache.get(str(tmp_path / "p.nii.gz"), cuda)
    assert torch.equal(first, load_volume(tmp_path / "p.nii.gz", (32, 32, 32), 1, cuda))
    os.unlink(tmp_path / "p.nii.gz")
    again = cache.get(str(tmp_path / "p.nii.gz"), cuda)
    assert again.device.type == "cuda" and torch.equal(again, first)
    with pytest.raises(ValueError):  # another roi is another item, and the source is gone
        VolumeCache(tmp_path / "cache", (16, 16, 16), 1).get(str(tmp_path / "p.nii.gz"), cuda)


# ---- the engines --------------------------------------------------------------------------------------------------------------------
def _csvs(tmp_path, n, corrupt=None):
    rows = []
    variants = [dict(), dict(out_of=(1, 0, 2), sign=(-1, -1, 1)), dict(out_of=(0, 1, 2), sign=(1, -1, -1)), dict(out_of=(2, 1, 0), sign=(1, 1, 1))]
    for i in range(n):
        p = tmp_path / f"scan{i}.nii.gz"
        _write_phantom(p, "thick" if i % 2 else "cut", **variants[i % 4])
        if i == corrupt:
            blob = open(p, "rb").read()
            open(p, "wb").write(blob[:len(blob) // 3])
        rows.append(str(p))
    path = tmp_path / "scans.csv"
    path.write_text("img_path\n" + "\n".join(rows) + "\n")
    return ["DATA.TRAIN_CSV_PATH", str(path), "DATA.VAL_CSV_PATH", str(path), "DATA.TEST_CSV_PATH", str(path), "DATA.SYNTHETIC", "False",
            "DATA.CACHE_DIR", str(tmp_path / "cache")]


def _run(cmd):
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = str(sock.getsockname()[1])
    run = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", port]
    r = subprocess.run(run + cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600, cwd=ROOT)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    return log


def _losses(log):
    return [float(l.split("Loss:")[1].split()[0]) for l in log.splitlines() if "] " in l and "Loss:" in l and "Epoch" in l]


def test_mae_entry_point_trains_from_a_csv_with_a_corrupt_entry(cuda, tmp_path):
    """Two training steps of batch 2 (and the validation and test passes) from four phantom files, one truncated: finite losses, the
    placeholder reported, the cache filled."""
    out = ["MODEL.DIR", str(tmp_path / "ckpt"), "LOG.OUTPUT_DIR", str(tmp_path / "log"), "OUTPUT", str(tmp_path / "json")]
    log = _run([os.path.join(ROOT, "main_pretrain_mae.py"), "--local_rank", "0", "--model_name", "mae", "--batch_size", "2", "--max_epochs", "1",
                "--base_lr", "3e-4", "--cfg", os.path.join(ROOT, "configs/mae/mae_tiny_plumbing.yaml"), "--opts"] + out + _csvs(tmp_path, 4, corrupt=2))
    losses = _losses(log)
    assert len(losses) >= 2 and all(np.isfinite(l) and l > 0 for l in losses), log[-3000:]
    assert "Error loading index 2:" in log and "nan" not in log.lower().replace("nanosecond", "")
    assert len([f for f in os.listdir(tmp_path / "cache") if f.endswith(".pt")]) == 3


def test_dino_entry_point_runs_a_step_through_the_multi_crop_loader(cuda, tmp_path):
    out = ["MODEL.DIR", str(tmp_path / "ckpt"), "LOG.OUTPUT_DIR", str(tmp_path / "log"), "OUTPUT", str(tmp_path / "json")]
    log = _run([os.path.join(ROOT, "main_pretrain_dino.py"), "--local_rank", "0", "--model_name", "dino", "--batch_size", "2", "--max_epochs", "1",
                "--base_lr", "5e-3", "--cfg", os.path.join(ROOT, "configs/dino/dino_tiny_plumbing.yaml"), "--opts"] + out + _csvs(tmp_path, 2))
    assert "train completed" in log and "test completed" in log and "Error loading" not in log
    assert "nan" not in log.lower().replace("nanosecond", "")
    assert len([f for f in os.listdir(tmp_path / "cache") if f.endswith(".pt")]) == 2
