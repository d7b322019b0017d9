"""CPU: the native-grid reference (tests/native_ref.py) against torch's own resampling, the host tables of
headct_foundation_amd/native.py against the reference, planted faults, the geometry cache, the config keys and the volumes."""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from headct_foundation_amd import native
from tests import native_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
GEOMS = {**R.geometries(), **R.long_geometries(), **R.dyadic_geometries(), "identity": R.identity_geom()}


def _vol(K=3, seed=0):
    return R.gaussian_volume(K, seed, False)


# ---- the reference against torch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", ["full", "inner"])
def test_reference_equals_interpolate_where_steps_are_one(box):
    """1 mm RAS file: inside the box the blend is F.interpolate(trilinear, align_corners=False) of the item onto the box."""
    geom = R.make_geom((12, 9, 7), (0, 1, 2), (False, False, False), (1.0, 1.0, 1.0), box)
    assert geom.steps == (1.0, 1.0, 1.0)
    vol = _vol()
    got, inside = R.blend(vol.numpy(), R.tables(geom), geom.perm)  # [K, nk, nj, ni]
    want = F.interpolate(vol[None], size=geom.size, mode="trilinear", align_corners=False)[0].numpy()  # [K, RAS 0, 1, 2] = [K, i, j, k]
    s, z = geom.start, geom.size
    ins = np.zeros((7, 9, 12), bool)
    ins[s[2]:s[2] + z[2], s[1]:s[1] + z[1], s[0]:s[0] + z[0]] = True
    assert np.array_equal(inside, ins)
    sub = got[:, s[2]:s[2] + z[2], s[1]:s[1] + z[1], s[0]:s[0] + z[0]]
    # torch derives the source coordinate from a scale it keeps in fp32 even for float64 data: 2^-24 relative on a coordinate
    # below 6 moves a value by at most 6 * 2^-24 * (the largest difference of neighbours, below 10 for unit Gaussians) < 4e-6
    assert np.abs(sub - want.transpose(0, 3, 2, 1)).max() < 4e-6


@pytest.mark.parametrize("name", list(GEOMS))
def test_reference_equals_grid_sample(name):
    """General steps, orientation and box: grid_sample (bilinear, border padding, align_corners=False) on the grid of item
    coordinates built voxel by voxel."""
    geom = GEOMS[name]
    vol = _vol(seed=len(name))
    got, _ = R.blend(vol.numpy(), R.tables(geom), geom.perm)
    ni, nj, nk = geom.file_shape
    t = [R.axis_coordinate(geom, a, R.S)[0] for a in range(3)]  # per file axis, the coordinate on item axis o = perm.index(a)
    grid = torch.empty(1, nk, nj, ni, 3, dtype=F64)
    full = [torch.from_numpy(t[0])[None, None, :].expand(nk, nj, ni), torch.from_numpy(t[1])[None, :, None].expand(nk, nj, ni),
            torch.from_numpy(t[2])[:, None, None].expand(nk, nj, ni)]
    for a in range(3):
        o = geom.perm.index(a)
        grid[0, ..., 2 - o] = (2.0 * full[a] + 1.0) / R.S - 1.0  # grid_sample's x is the last item axis
    want = F.grid_sample(vol[None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0].numpy()
    # the tables' weights are fp32 by definition (half an ulp below 1 is 2^-25); a weight error e moves a lerp by e |b - a| <= 2 e M,
    # once per axis: 3 * 2^-25 * 2 M.  Everything else is float64.
    assert np.abs(got - want).max() <= 6 * 2.0 ** -25 * float(vol.abs().max()) + 1e-12


@pytest.mark.parametrize("name", list(R.geometries()))
def test_tables_invert_the_reorientation(name):
    """1 mm voxels, a full box and an item of the RAS volume's own shape: the item IS the reoriented file (data.py's transpose and
    flips), and both modes must give the file back exactly."""
    g0 = R.geometries()[name]
    geom = R.make_geom(g0.file_shape, g0.perm, g0.flip, (1.0, 1.0, 1.0), "full")
    ni, nj, nk = geom.file_shape
    file = np.arange(nk * nj * ni, dtype=np.float64).reshape(nk, nj, ni)
    ras = np.transpose(np.transpose(file, (2, 1, 0)), geom.perm)
    for o in range(3):
        if geom.flip[o]:
            ras = np.flip(ras, axis=o)
    for interp in native.INTERPS:
        tabs = native.native_tables(geom, geom.d, interp)
        assert R.tables_equal(tabs, R.tables(geom, geom.d, interp))
        got, inside = R.blend(ras[None], tabs, geom.perm)
        assert inside.all() and np.array_equal(got[0], file)


def test_identity_geometry():
    geom = R.identity_geom()
    for interp in native.INTERPS:
        for t in native.native_tables(geom, R.S, interp):
            assert np.array_equal(t["i0"], np.arange(R.S)) and not t["w"].any() and t["inside"].all()
            assert t["i0"].dtype == np.int32 and t["i1"].dtype == np.int32 and t["w"].dtype == np.float32 and t["inside"].dtype == np.uint8


# ---- the host tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", native.INTERPS)
@pytest.mark.parametrize("name", list(GEOMS))
def test_native_tables_equal_the_reference(name, interp):
    assert R.tables_equal(native.native_tables(GEOMS[name], R.S, interp), R.tables(GEOMS[name], R.S, interp))


def test_cases_cover_what_they_are_named_for():
    gs = R.geometries()
    assert {g.perm for g in gs.values()} == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    assert all(any(g.flip) for n, g in gs.items() if n.startswith("perm"))
    assert {g.flip for n, g in gs.items() if n.startswith("flip")} == {tuple(bool(c >> o & 1) for o in range(3)) for c in range(8)}
    assert {g.file_shape for g in gs.values()} == {(13, 9, 7), (7, 13, 9)}
    steps = {round(s, 3) for g in gs.values() for s in g.steps}
    assert {2.222, 1.0, 0.2} <= steps
    assert any(1 in g.size for g in gs.values()) and any(g.size == g.m and g.start == (0, 0, 0) for g in gs.values())
    both = 0
    for g in gs.values():  # outside voxels on both sides of every axis
        ins = [t["inside"] for t in R.tables(g)]
        both += all(i[0] == 0 and i[-1] == 0 and i.any() for i in ins)
    assert both >= 3
    for g in R.dyadic_geometries().values():  # weights that are multiples of 1/8
        assert all(np.array_equal(t["w"] * 8, np.round(t["w"] * 8)) for t in R.tables(g))


@pytest.mark.parametrize("fault", ["no_flip", "no_half", "no_start"])
def test_planted_table_faults_are_rejected(fault):
    """Each planted fault changes the tables, and changes the prediction of the reference on Gaussian logits."""
    geom = R.geometries()["flip7"]
    assert all(geom.flip) and min(geom.start) > 0
    good, bad = R.tables(geom), R.tables(geom, fault=fault)
    assert R.tables_equal(native.native_tables(geom, R.S), good) and not R.tables_equal(native.native_tables(geom, R.S), bad)
    vol = _vol(5, 3).numpy()
    pg, pb = R.predict(*R.blend(vol, good, geom.perm)), R.predict(*R.blend(vol, bad, geom.perm))
    assert (pg != pb).mean() > 0.05


def test_near_ties_of_the_reference_alone_are_rare():
    """On the Gaussian inputs of the GPU test the float64 reference leaves out far less than the cap."""
    worst = 0.0
    for name, geom, K, first, pad, bf16, seed in R.gaussian_cases():
        vol = R.gaussian_volume(K, seed, bf16).numpy()
        values, inside = R.blend(vol, R.tables(geom), geom.perm)
        share = R.near_ties(values, inside, np.abs(vol).max()).mean()
        worst = max(worst, share)
        assert share <= R.NEAR_TIE_CAP / 4, (name, share)
    print(f"worst near-tie share {worst:.2e} (cap {R.NEAR_TIE_CAP:.0e})")
    assert R.blend_error_bound(4.0) == 16 * 2.0 ** -24 * 4.0


def test_argmax_rule_and_counts():
    values = np.zeros((3, 1, 1, 4))
    values[2, 0, 0, 1] = 1.0
    values[1, 0, 0, 2] = values[2, 0, 0, 2] = 0.5
    inside = np.array([[[True, True, True, False]]])
    values[1, 0, 0, 3] = 9.0
    pred = R.predict(values, inside)
    assert pred.dtype == np.int16 and pred.tolist() == [[[0, 2, 1, 0]]]
    y = np.array([[[0, 1, 255, 0]]], np.uint8)
    assert R.counts(pred, y, 3).tolist() == [[2, 0, 0], [0, 0, 1], [0, 1, 0]]


# ---- geometry cache, config, volumes -----------------------------------------------------------------------------------------------------
def test_geometry_cache_round_trip(tmp_path):
    from headct_foundation_amd.data import PIPELINE_VERSION, VolumeCache
    geom = R.geometries()["perm120"]
    made = []

    def maker(path, roi, in_channels, device):
        made.append(path)
        return geom

    cache = native.GeometryCache(tmp_path, 96, 3, maker=maker)
    file = cache.file_of("/data/a.nii.gz")
    assert file.endswith(".json") and os.path.basename(file)[:-5] != VolumeCache(tmp_path, 96, 3).key("/data/a.nii.gz") and PIPELINE_VERSION == 1
    got = cache.get("/data/a.nii.gz", "cpu")
    assert got == geom and made == ["/data/a.nii.gz"] and os.path.exists(file)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    back = cache.get("/data/a.nii.gz", "cpu")  # from the file: float64 steps and the affine survive JSON bit for bit
    assert back == geom and made == ["/data/a.nii.gz"] and back.steps == geom.steps
    assert set(json.load(open(file))) == {"file_shape", "perm", "flip", "d", "m", "steps", "affine", "start", "size"}
    with open(file, "w") as f:
        f.write('{"file_shape": [1, 2')  # a corrupt file is rebuilt
    assert cache.get("/data/a.nii.gz", "cpu") == geom and len(made) == 2 and native.ScanGeometry.from_json(open(file).read()) == geom
    assert native.GeometryCache(tmp_path, 96, 1, maker=maker).file_of("/data/a.nii.gz") != file
    with pytest.raises(ValueError):
        native.ScanGeometry((4, 4, 4), (0, 1, 2), (0, 0, 0), (4, 4, 4), (4, 4, 4), (1.0, 1.0, 1.0), np.eye(4), (0, 0, 3), (4, 4, 2))
    assert native.confine_box([-2, 1, 9, 50, 0, 3, 0, 0], (6, 6, 6)) == ([0, 1, 5], [6, 1, 1])  # label_to_item_kernel's confinement


def _args(tmp_path, opts=None, **flags):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    return argparse.Namespace(cfg=str(cfg), opts=opts, local_rank=0, **flags)


def test_native_config_keys_and_flags(tmp_path):
    from config import check_segmentation_mode, get_config
    c = get_config(_args(tmp_path))
    assert (c.SEG.NATIVE_PREDS, c.SEG.NATIVE_INTERP) == (False, "linear")
    c = get_config(_args(tmp_path, native_preds=True, native_interp="nearest"))
    assert (c.SEG.NATIVE_PREDS, c.SEG.NATIVE_INTERP) == (True, "nearest")
    c = get_config(_args(tmp_path, opts=["SEG.NATIVE_PREDS", "True", "SEG.NATIVE_INTERP", "nearest"]))
    assert (c.SEG.NATIVE_PREDS, c.SEG.NATIVE_INTERP) == (True, "nearest")
    with pytest.raises(ValueError, match="NATIVE_INTERP"):
        get_config(_args(tmp_path, native_interp="cubic"))
    with pytest.raises(ValueError, match="NATIVE_PREDS"):
        check_segmentation_mode(get_config(_args(tmp_path, native_preds=True, opts=["DATA.SYNTHETIC", "True"])))
    check_segmentation_mode(get_config(_args(tmp_path, native_preds=True, opts=["DATA.SYNTHETIC", "False"])))
    src = open(os.path.join(ROOT, "main_segmentation.py")).read()
    assert "--native_preds" in src and "--native_interp" in src


def test_class_volumes_ml_on_a_sheared_affine():
    aff = np.array([[0.45, 0.1, 0.0, -100.0], [0.0, 0.45, 0.2, 30.0], [0.0, 0.0, -1.0, 5.0], [0.0, 0.0, 0.0, 1.0]])
    vox = torch.tensor([1000, 250, 0], dtype=torch.int64)
    want = np.array([1000, 250, 0]) * 0.45 * 0.45 * 1.0 / 1000.0  # a triangular matrix: the determinant is the diagonal's product
    assert np.allclose(native.class_volumes_ml(vox, aff), want, rtol=1e-14, atol=0)
    assert np.allclose(native.class_volumes_ml(np.array([8]), np.diag([2.0, 5.0, 10.0, 1.0])), [0.8])


def test_native_symbols_declared_and_exported(lib):
    from headct_foundation_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "headct_hip.h")).read(), flags=re.S)
    for s in ("hct_seg_to_native", "hct_seg_to_native_workspace_bytes"):
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert "native.hip" in build.SOURCES
    # one partial of 4 K int32 per workgroup, a workgroup per slice and 16 rows, at most 8192 of them
    assert lib.hct_seg_to_native_workspace_bytes(512, 512, 160, 6) == 32 * 160 * 4 * 6 * 4
    assert lib.hct_seg_to_native_workspace_bytes(7, 3, 2, 2) == 2 * 4 * 2 * 4
    assert lib.hct_seg_to_native_workspace_bytes(2, 1024, 1024, 16) == 8192 * 4 * 16 * 4
    assert lib.hct_seg_to_native_workspace_bytes(7, 3, 2, 17) == 0 and lib.hct_seg_to_native_workspace_bytes(1025, 3, 2, 2) == 0


def test_seg_to_native_refuses_the_cpu():
    from headct_foundation_amd import _lib
    with pytest.raises(_lib.HctError, match="cuda"):
        native.seg_to_native(torch.zeros(27, 16), 2, 2, 0, R.identity_geom())
