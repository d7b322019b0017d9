"""Host side of the loading chain (no GPU): the NIfTI-1 reader, the RAS assignment, the geometry of Spacingd, the FIR restatement
against scipy, the cache, the loader's sampler and placeholder rule, the config door and the exported symbols.  It also asserts, for
every case the GPU tests compare end to end, the two conditions that make those comparisons meaningful."""
import os
import re

import numpy as np
import pytest
import torch

from headct_foundation_amd import nifti
from headct_foundation_amd.data import PretrainVolumes, VolumeCache, get_pretrain_dataloaders, load_volume
from tests import loading_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _labelled(shape, dtype):
    """Every voxel its own value, within the range of the dtype."""
    n = int(np.prod(shape))
    v = np.arange(n).reshape(shape)
    info = np.iinfo(dtype) if np.dtype(dtype).kind in "iu" else None
    if info is not None:
        v = v % (int(info.max) - int(info.min) + 1) + int(info.min)
    return v.astype(dtype)


AFF = np.array([[0.5, 0.0, 0.0, -12.0], [0.0, 0.75, 0.0, 7.5], [0.0, 0.0, 2.5, 3.0], [0.0, 0.0, 0.0, 1.0]])


# ---- reader -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "int16", "int32", "float32", "float64", "int8", "uint16"])
def test_reader_every_datatype_both_byte_orders_gz_and_plain(tmp_path, dtype):
    data = _labelled((5, 7, 3), dtype)
    for bo in "<>":
        for ext in (".nii", ".nii.gz"):
            p = tmp_path / f"v_{dtype}_{'le' if bo == '<' else 'be'}{ext}"
            R.write_nifti(p, data, AFF, slope=2.0, inter=-3.0, byteorder=bo)
            raw, slope, inter, aff = nifti.read_nifti(p)
            assert raw.dtype == np.dtype(dtype) and raw.dtype.isnative and raw.shape == (3, 7, 5)
            assert np.array_equal(raw, data.transpose(2, 1, 0))  # file order: axis i contiguous
            assert (slope, inter) == (2.0, -3.0) and np.array_equal(aff, AFF)


def test_reader_scaling_follows_nibabel(tmp_path):
    data = _labelled((4, 4, 4), "int16")
    for slope, inter, want in ((0.0, 5.0, (None, None)), (float("nan"), 0.0, (None, None)), (1.0, 0.0, (1.0, 0.0)), (0.5, -1024.0, (0.5, -1024.0))):
        R.write_nifti(tmp_path / "s.nii", data, AFF, slope=slope, inter=inter)
        assert nifti.read_nifti(tmp_path / "s.nii")[1:3] == want


def test_reader_affine_sform_qform_neither(tmp_path):
    data = _labelled((6, 5, 4), "int16")
    lps = np.diag([-0.5, -0.75, 2.5, 1.0])  # a left-handed-to-RAS flip pair keeps the determinant positive
    lps[:3, 3] = [10.0, 20.0, -30.0]
    mirrored = np.diag([-0.5, 0.75, 2.5, 1.0])  # determinant < 0: qfac = -1
    for aff in (AFF, lps, mirrored, R.tilted(AFF)):
        R.write_nifti(tmp_path / "s.nii", data, aff, form="sform")
        assert np.allclose(nifti.read_nifti(tmp_path / "s.nii")[3], aff, rtol=1e-6, atol=1e-6)
        R.write_nifti(tmp_path / "q.nii", data, aff, form="qform")
        assert np.allclose(nifti.read_nifti(tmp_path / "q.nii")[3], aff, rtol=1e-5, atol=1e-5)
    R.write_nifti(tmp_path / "n.nii", data, AFF, form="none")
    want = np.diag([0.5, 0.75, 2.5, 1.0])
    want[:3, 3] = [-(6 - 1) / 2 * 0.5, -(5 - 1) / 2 * 0.75, -(4 - 1) / 2 * 2.5]  # nibabel's centre-of-volume origin
    assert np.allclose(nifti.read_nifti(tmp_path / "n.nii")[3], want)
    # both codes set: the sform wins
    R.write_nifti(tmp_path / "b.nii", data, AFF, form="sform")
    blob = bytearray(open(tmp_path / "b.nii", "rb").read())
    blob[252:254] = (1).to_bytes(2, "little")
    open(tmp_path / "b.nii", "wb").write(blob)
    assert np.array_equal(nifti.read_nifti(tmp_path / "b.nii")[3], AFF)


def test_reader_squeezes_a_single_time_point_and_refuses_the_rest(tmp_path):
    data = _labelled((4, 5, 6), "int16")
    R.write_nifti(tmp_path / "t1.nii", data, AFF, dim4=True)
    assert nifti.read_nifti(tmp_path / "t1.nii")[0].shape == (6, 5, 4)
    bad = {
        "two_volumes.nii": dict(n_volumes=2),
        "nifti2.nii": dict(sizeof_hdr=540),
        "pair.nii": dict(magic=b"ni1\0"),
        "analyze.nii": dict(magic=b"\0\0\0\0"),
        "garbage_size.nii": dict(sizeof_hdr=123),
    }
    for name, kw in bad.items():
        R.write_nifti(tmp_path / name, data, AFF, **kw)
        with pytest.raises(ValueError, match=re.escape(name)):
            nifti.read_nifti(tmp_path / name)
    R.write_nifti(tmp_path / "rgb.nii", data, AFF)
    blob = bytearray(open(tmp_path / "rgb.nii", "rb").read())
    blob[70:72] = (128).to_bytes(2, "little")  # RGB24
    open(tmp_path / "rgb.nii", "wb").write(blob)
    open(tmp_path / "cut.nii", "wb").write(bytes(blob[:400]))
    open(tmp_path / "short.nii", "wb").write(b"\0" * 100)
    open(tmp_path / "notgz.nii.gz", "wb").write(b"not a gzip stream at all" * 40)
    for name in ("rgb.nii", "cut.nii", "short.nii", "notgz.nii.gz", "missing.nii"):
        with pytest.raises(ValueError, match=re.escape(name)):
            nifti.read_nifti(tmp_path / name)


# ---- orientation and geometry -------------------------------------------------------------------------------------------------------
def _apply(stored, perm, flip):
    out = np.transpose(stored, perm)
    for o in range(3):
        if flip[o]:
            out = np.flip(out, axis=o)
    return out


def test_ras_axes_on_all_48_signed_permutations():
    data = _labelled((4, 5, 6), "int32")
    aff = AFF.copy()
    assert len(R.SIGNED_PERMUTATIONS) == 48
    for out_of, sign in R.SIGNED_PERMUTATIONS:
        stored, saff = R.stored_as(data, aff, out_of, sign)
        perm, flip, zooms, ras = nifti.ras_axes(saff, stored.shape)
        assert np.array_equal(_apply(stored, perm, flip), data), (out_of, sign)
        assert np.allclose(ras, aff, atol=1e-12) and np.allclose(zooms, [0.5, 0.75, 2.5]), (out_of, sign)


def test_ras_axes_on_a_tilted_frame():
    data = _labelled((4, 5, 6), "int32")
    for out_of, sign in (((0, 1, 2), (1, 1, 1)), ((1, 0, 2), (-1, -1, 1)), ((2, 0, 1), (1, -1, -1))):
        stored, saff = R.stored_as(data, R.tilted(AFF, 15.0), out_of, sign)
        perm, flip, zooms, ras = nifti.ras_axes(saff, stored.shape)
        assert np.array_equal(_apply(stored, perm, flip), data)
        assert np.allclose(zooms, [0.5, 0.75, 2.5]) and np.allclose(ras, R.tilted(AFF, 15.0), atol=1e-12)  # the tilt stays in the affine


def test_shape_rule_rounds_half_to_even():
    assert nifti.spacing_geometry(512, 0.47) == (int(np.round(511 * 0.47 + 1)), 1.0 / 0.47) and nifti.spacing_geometry(512, 0.47)[0] == 241
    assert nifti.spacing_geometry(4, 0.5)[0] == 2      # 2.5 -> 2
    assert nifti.spacing_geometry(6, 0.5)[0] == 4      # 3.5 -> 4
    assert nifti.spacing_geometry(2, 2.5)[0] == 4      # 3.5 -> 4
    assert nifti.spacing_geometry(160, 1.3) == (208, 1.0 / 1.3)
    assert nifti.spacing_geometry(1, 3.0) == (1, 1.0 / 3.0)
    for n, z in ((17, 5.0), (150, 0.47), (33, 1.0)):
        assert nifti.spacing_geometry(n, z)[0] == R.out_length(n, z)


def test_tables_are_the_restatements():
    for n, zoom in ((44, 1.3), (150, 0.47), (17, 5.0), (9, 0.3), (1, 2.0)):
        m, step = nifti.spacing_geometry(n, zoom)
        base, w = nifti.bspline3_tables(n, m, step)
        rbase, rw = R.fir_tables(n, m, step)
        assert base.dtype == np.int32 and w.dtype == np.float64 and w.shape == (nifti.TAPS, m) and nifti.TAPS == R.TAPS == 32
        assert np.array_equal(base, rbase) and float(np.abs(w - rw).max()) <= 2.0 ** -24  # the restatement's are these rounded to fp32: half a step of weights below 2
        assert np.allclose(w.astype(np.float64).sum(0), 1.0, atol=1e-6)  # a constant stays a constant
        assert int(base.min()) >= -1 - nifti.PREFILTER_REACH and int(base.max()) + nifti.TAPS - 1 <= n + 12 + nifti.PREFILTER_REACH


@pytest.mark.parametrize("name", sorted(R.PHANTOMS))
def test_fir_restatement_against_scipy(name):
    """Bound from the number format: a row of weights has sum |w| <= sum |h| = sqrt(3) (1 + |z|) / (1 - |z|) = 3 =: g, so after pass
    a the amplitude is at most g^a A0; a pass of T = 32 taps with weights rounded to fp32 adds at most (T + 2) u g times its input
    amplitude (u = 2^-24), and the later passes amplify that by at most g each: in all 3 (T + 2) u g^3 A0, 0.2 HU at A0 = 1200.
    The truncation of the prefilter adds 2 sqrt(3) |z|^15 / (1 - |z|) g^2 A0 < 1e-4 HU.  (Clamping coefficient indices instead
    of extending the signal is off by about 2 HU at the faces.)"""
    _, values, zooms, _ = R.phantom_ras(name)
    want, got = R.resample_f64(values, zooms), R.resample_fir_f32(values, zooms)
    assert got.dtype == np.float32 and got.shape == want.shape
    a0 = float(np.abs(values).max())
    bound = 3 * (R.TAPS + 2) * 2.0 ** -24 * 27 * a0 + 1e-4
    err = float(np.abs(got - want).max())
    face = max(float(np.abs(got - want)[sl].max()) for sl in ((0,), (-1,), (slice(None), 0), (slice(None), -1), (Ellipsis, 0), (Ellipsis, -1)))
    print(f"{name}: fp32 FIR vs scipy float64: max abs {err:.3g} HU (faces {face:.3g}), bound {bound:.3g}")
    assert err <= bound


@pytest.mark.parametrize("name,roi,chans", R.END_TO_END_CASES)
def test_conditions_that_make_the_gpu_comparisons_meaningful(name, roi, chans):
    """(1) the foreground box does not hang on a rounding: v > 0.05 and v > -0.05 give the same box on the float64 volume;
    (2) the fp32 restatement's cache item differs from the float64 chain's on at most a quarter of the share the GPU tests allow
    (0.5 % / 4) and nowhere by more than one fp16 step."""
    _, values, zooms, _ = R.phantom_ras(name)
    zooms = [float(np.float32(z)) for z in zooms]  # what a NIfTI header holds
    vol = R.resample_f64(values, zooms)
    assert R.foreground_box(vol, 0.05) == R.foreground_box(vol, -0.05) == R.foreground_box(vol)
    a = R.chain(values, zooms, roi, chans)
    b = R.chain(values, zooms, roi, chans, R.resample_fir_f32)
    steps = R.fp16_steps(a, b)
    share = float((steps > 0).float().mean())
    print(f"{name} {roi} x {chans}: fp32 restatement vs float64 chain: {share:.3%} of voxels differ, max {int(steps.max())} step")
    assert int(steps.max()) <= 1 and share <= (1 - R.EQUAL_SHARE) / 4


# ---- load_volume's refusals that need no device -------------------------------------------------------------------------------------
def test_load_volume_refuses_oversized_axes_and_bad_channels(tmp_path):
    R.write_nifti(tmp_path / "long.nii", np.zeros((1100, 3, 3), np.uint8), np.eye(4))
    with pytest.raises(ValueError, match="beyond 1024"):
        load_volume(tmp_path / "long.nii", (8, 8, 8), 1, "cpu")
    R.write_nifti(tmp_path / "coarse.nii", np.zeros((600, 3, 3), np.uint8), np.diag([2.0, 1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="beyond 1024"):
        load_volume(tmp_path / "coarse.nii", (8, 8, 8), 1, "cpu")
    with pytest.raises(NotImplementedError):
        load_volume(tmp_path / "long.nii", (8, 8, 8), 2, "cpu")
    from headct_foundation_amd import HctError
    R.write_nifti(tmp_path / "ok.nii", np.ones((4, 4, 4), np.uint8), np.eye(4))
    with pytest.raises(HctError):  # no CPU fallback
        load_volume(tmp_path / "ok.nii", (8, 8, 8), 1, "cpu")


# ---- cache --------------------------------------------------------------------------------------------------------------------------
class _CountingLoader:
    def __init__(self):
        self.calls = []

    def __call__(self, path, roi, in_channels, device):
        nifti.read_nifti(path)  # reader errors surface as they do in load_volume
        self.calls.append(str(path))
        g = torch.Generator().manual_seed(len(str(path)))
        return torch.rand((in_channels,) + tuple(roi), generator=g).to(torch.float16).to(device)


def test_cache_writes_atomically_serves_and_rebuilds(tmp_path):
    src = tmp_path / "scan.nii"
    R.write_nifti(src, np.ones((4, 4, 4), np.uint8), np.eye(4))
    loader = _CountingLoader()
    cache = VolumeCache(tmp_path / "cache", (8, 8, 8), 3, loader=loader)
    a = cache.get(str(src), "cpu")
    files = os.listdir(tmp_path / "cache")
    assert files == [cache.key(str(src)) + ".pt"] and a.dtype == torch.float16 and a.shape == (3, 8, 8, 8)  # no temporary left behind
    on_disk = torch.load(cache.file_of(str(src)), weights_only=True)
    assert isinstance(on_disk, torch.Tensor) and torch.equal(on_disk, a)  # the plain tensor
    os.unlink(src)
    assert torch.equal(cache.get(str(src), "cpu"), a) and len(loader.calls) == 1  # served without the source
    # a truncated file is rebuilt (the source is needed again)
    R.write_nifti(src, np.ones((4, 4, 4), np.uint8), np.eye(4))
    blob = open(cache.file_of(str(src)), "rb").read()
    open(cache.file_of(str(src)), "wb").write(blob[:len(blob) // 2])
    assert torch.equal(cache.get(str(src), "cpu"), a) and len(loader.calls) == 2
    assert torch.equal(torch.load(cache.file_of(str(src)), weights_only=True), a)
    # a failing loader leaves nothing behind
    with pytest.raises(ValueError):
        cache.get(str(tmp_path / "absent.nii"), "cpu")
    assert os.listdir(tmp_path / "cache") == files


def test_cache_key_changes_with_path_roi_and_channels(tmp_path):
    mk = lambda roi, c: VolumeCache(tmp_path, roi, c, loader=_CountingLoader())
    keys = {mk((8, 8, 8), 3).key("a.nii"), mk((8, 8, 8), 3).key("b.nii"), mk((8, 8, 16), 3).key("a.nii"), mk((8, 8, 8), 1).key("a.nii")}
    assert len(keys) == 4 and mk(8, 3).key("a.nii") == mk([8, 8, 8], 3).key("a.nii")
    from headct_foundation_amd import data
    old = data.PIPELINE_VERSION
    try:
        data.PIPELINE_VERSION = old + 1
        assert mk((8, 8, 8), 3).key("a.nii") not in keys
    finally:
        data.PIPELINE_VERSION = old


# ---- loader -------------------------------------------------------------------------------------------------------------------------
def _csv(path, rows, column="img_path"):
    with open(path, "w") as f:
        f.write(f"idx,{column},label\n")
        for i, r in enumerate(rows):
            f.write(f"{i},{r},0\n")
    return str(path)


def test_sampler_partition_over_world_2(tmp_path):
    paths = [f"/nowhere/{i}.nii" for i in range(5)]
    csv = _csv(tmp_path / "t.csv", paths)
    cache = VolumeCache(tmp_path / "c", 8, 1, loader=_CountingLoader())
    r0 = PretrainVolumes(csv, cache, 2, "cpu", rank=0, world_size=2)
    r1 = PretrainVolumes(csv, cache, 2, "cpu", rank=1, world_size=2)
    assert r0.paths == paths and r0.indices == [0, 2, 4] and r1.indices == [1, 3, 0]  # DistributedSampler(shuffle=False): padded by wrapping
    assert len(r0) == len(r1) == 2
    assert PretrainVolumes(csv, cache, 2, "cpu").indices == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="img_path"):
        PretrainVolumes(_csv(tmp_path / "bad.csv", paths, column="image"), cache, 2, "cpu")
    with pytest.raises(NotImplementedError):  # the loaders stay cubic, like the models
        PretrainVolumes(csv, VolumeCache(tmp_path / "c2", (8, 8, 16), 1, loader=_CountingLoader()), 2, "cpu")


def test_placeholder_on_a_corrupt_file(tmp_path, capsys):
    files = []
    for i in range(3):
        files.append(str(tmp_path / f"s{i}.nii.gz"))
        R.write_nifti(files[-1], np.ones((4, 4, 4), np.uint8), np.eye(4))
    open(files[1], "wb").write(b"\x1f\x8b broken")
    cache = VolumeCache(tmp_path / "c", 8, 3, loader=_CountingLoader())
    loader = PretrainVolumes(_csv(tmp_path / "t.csv", files), cache, 2, "cpu", num_workers=2)
    batches = list(loader)
    assert [tuple(b.shape) for b in batches] == [(2, 3, 8, 8, 8), (1, 3, 8, 8, 8)] and all(b.dtype == torch.float16 for b in batches)
    assert float(batches[0][1].abs().max()) == 0.0 and float(batches[0][0].abs().max()) > 0 and float(batches[1][0].abs().max()) > 0
    out = capsys.readouterr().out
    assert "Error loading index 1:" in out and "s1.nii.gz" in out and out.count("Error loading index") == 1
    assert sorted(os.path.basename(c) for c in cache.loader.calls) == ["s0.nii.gz", "s2.nii.gz"]
    assert [tuple(b.shape) for b in loader] == [(2, 3, 8, 8, 8), (1, 3, 8, 8, 8)]  # a second epoch, from the cache
    assert len(cache.loader.calls) == 2


# ---- the config door and the exports ------------------------------------------------------------------------------------------------
def _config(tmp_path, **csvs):
    from config import _C
    cfg = _C.clone()
    cfg.defrost()
    cfg.DATA.SYNTHETIC, cfg.DATA.BATCH_SIZE, cfg.DATA.CACHE_DIR = False, 2, str(tmp_path / "cache")
    cfg.MODEL.ROI, cfg.MODEL.IN_CHANS, cfg.MAE.INPUT_SIZE, cfg.MAE.IN_CHANS = [16, 16, 16], 1, 16, 1
    cfg.VIT.INPUT_SIZE, cfg.VIT.IN_CHANS = 16, 1
    for k, v in csvs.items():
        setattr(cfg.DATA, k, v)
    return cfg


def test_config_door(tmp_path):
    import main_pretrain_dino as M
    rows = [str(tmp_path / f"{i}.nii") for i in range(5)]
    csvs = {k: _csv(tmp_path / f"{k}.csv", rows[:n]) for k, n in (("TRAIN_CSV_PATH", 5), ("VAL_CSV_PATH", 2), ("TEST_CSV_PATH", 1))}
    for door in (lambda c: get_pretrain_dataloaders(c, "cpu", 0, 1), lambda c: M.build_loaders(c, torch.device("cpu"), 0, 1)):
        loaders = door(_config(tmp_path, **csvs))
        assert [len(l) for l in loaders] == [3, 1, 1]
        assert all(isinstance(l.base, PretrainVolumes) and l.base.cache.roi == (16, 16, 16) for l in loaders)
        for key in csvs:  # a missing CSV names its key
            with pytest.raises(FileNotFoundError, match="DATA." + key):
                door(_config(tmp_path, **dict(csvs, **{key: str(tmp_path / "absent.csv")})))
        cfg = _config(tmp_path, **csvs)
        cfg.MODEL.ROI = [16, 16, 24]
        with pytest.raises(ValueError, match="MODEL.ROI"):
            door(cfg)
    with pytest.raises(FileNotFoundError, match="DATA.TRAIN_CSV_PATH"):  # the defaults point nowhere
        get_pretrain_dataloaders(_config(tmp_path), "cpu", 0, 1)
    train, val, test = get_pretrain_dataloaders(_config(tmp_path, **csvs), "cpu", 0, 1)
    assert (train.transform.smooth_prob, val.transform.smooth_prob, test.transform.smooth_prob) == (0.2, 0.2, 0.0)
    assert (train.transform.flip_prob, train.transform.shift_prob, test.transform.flip_prob, test.transform.shift_prob) == (0.1, 0.5, 0.0, 0.0)
    # the synthetic door is where it was
    cfg = _config(tmp_path)
    cfg.DATA.SYNTHETIC = True
    assert len(M.build_loaders(cfg, torch.device("cpu"), 0, 1)) == 3


def test_exports_are_declared_in_the_header(lib):
    import headct_foundation_amd as pkg
    from headct_foundation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "headct_hip.h")).read()
    names = ("hct_volume_to_ras", "hct_bspline3_resample", "hct_bspline3_resample_workspace_bytes", "hct_foreground_bbox",
             "hct_foreground_bbox_workspace_bytes", "hct_crop_window_resize_area")
    for s in names:
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert "HCT_LOAD_EMPTY_FOREGROUND" in hdr
    assert lib.hct_bspline3_resample_workspace_bytes(512, 512, 160, 241, 241, 208) >= (241 * 512 * 160 + 241 * 241 * 160) * 8
    assert lib.hct_foreground_bbox_workspace_bytes(241, 241, 208) >= 24 and lib.hct_foreground_bbox_workspace_bytes(0, 4, 4) == 0
    for s in ("load_volume", "VolumeCache", "PretrainVolumes", "read_nifti"):
        assert hasattr(pkg, s), s
    assert os.path.exists(os.path.join(ROOT, "cache_volumes.py"))
