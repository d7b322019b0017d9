"""CPU: the surface-distance oracle (tests/surface_ref.py) against closed forms, the numpy restatement of hct_edt3d's arithmetic
against scipy, planted faults, the host helpers of headct_foundation_amd/surface.py, SurfaceMetrics, the config keys and the ABI."""
import argparse
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from headct_foundation_amd import surface
from headct_foundation_amd.metrics import SurfaceMetrics
from tests import surface_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
SPACING = (2.5, 0.75, 0.5)  # (s_k, s_j, s_i)


def _cuboid(shape, lo, hi, value=1, dtype=np.int16):
    v = np.zeros(shape, dtype)
    v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = value
    return v


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("s", [1, 3])
def test_shifted_cuboid_has_the_shift_as_hausdorff_distance(axis, s):
    """A solid cuboid against itself shifted by s voxels along one axis: every surface voxel of one has a surface voxel of the other
    exactly s voxels away along the axis (or nearer), so HD = s * spacing[axis] exactly, and NSD reaches 1 at that tolerance."""
    shape, lo, hi = (14, 16, 18), [3, 4, 5], [8, 10, 12]
    labels = _cuboid(shape, lo, hi, dtype=np.uint8)
    lo2, hi2 = list(lo), list(hi)
    lo2[axis] += s
    hi2[axis] += s
    pred = _cuboid(shape, lo2, hi2)
    want = s * SPACING[axis]
    m = R.class_metrics(pred, labels, 1, SPACING, want)
    assert m["HD"] == want and m["NSD"] == 1.0 and m["HD95"] <= want and 0 < m["ASSD"] < want
    below = R.class_metrics(pred, labels, 1, SPACING, np.nextafter(want, 0.0))
    assert below["NSD"] < 1.0 and below["HD"] == want
    same = R.class_metrics(labels.astype(np.int16), labels, 1, SPACING, 0.0)
    assert same["HD"] == 0.0 and same["ASSD"] == 0.0 and same["NSD"] == 1.0


def test_two_single_voxels():
    pred, labels = np.zeros((5, 6, 7), np.int16), np.zeros((5, 6, 7), np.uint8)
    pred[1, 2, 3], labels[3, 5, 1] = 1, 1
    d = float(np.sqrt(((2 * 2.5) ** 2 + (3 * 0.75) ** 2) + (2 * 0.5) ** 2))
    m = R.class_metrics(pred, labels, 1, SPACING, 1.0)
    assert (m["n_pred"], m["n_gt"]) == (1, 1) and m["HD"] == d and m["HD95"] == d and m["ASSD"] == d and m["NSD"] == 0.0


@pytest.mark.parametrize("n", [1, 2, 21, 22])
def test_percentile_ranks_and_interpolation(n):
    """n = 1 and 2, n = 21 (r = 19 is an integer) and n = 22 (r = 19.95): the two ranks and the lerp are numpy's."""
    d = np.sort(np.random.default_rng(n).uniform(0.0, 9.0, n))
    lo, hi, r = surface.percentile_ranks(n)
    assert lo == int(np.floor(0.95 * (n - 1))) and hi == min(lo + 1, n - 1) and abs(r - 0.95 * (n - 1)) < 1e-12
    if n == 21:
        assert r == lo == 19 or abs(r - 19) < 1e-12
    want = float(np.percentile(d, 95))
    got = surface.lerp_percentile(float(d[lo]), float(d[hi]), r)
    assert abs(got - want) <= 4 * EPS * want
    assert abs(got - (d[lo] + (r - lo) * (d[hi] - d[lo]))) <= 4 * EPS * max(want, 1e-300)


def test_empty_rules():
    shape = (6, 6, 6)
    z16, z8 = np.zeros(shape, np.int16), np.zeros(shape, np.uint8)
    one = _cuboid(shape, (1, 1, 1), (3, 3, 3))
    m = R.surface_metrics(z16, z8, 2, SPACING)
    assert all(np.isnan(m[k][1]) for k in ("HD", "HD95", "ASSD", "NSD"))
    for pred, labels in ((one, z8), (z16, one.astype(np.uint8))):
        m = R.surface_metrics(pred, labels, 2, SPACING)
        assert m["NSD"][1] == 0.0 and all(np.isnan(m[k][1]) for k in ("HD", "HD95", "ASSD"))
    assert np.isnan(m["NSD"][0]) and m["n_gt"][1] == 8
    # a prediction that lies on ignore voxels only is empty
    ign = np.where(one > 0, 255, 0).astype(np.uint8)
    m = R.surface_metrics(one, ign, 2, SPACING)
    assert m["n_pred"][1] == 0 and np.isnan(m["NSD"][1])


# ---- the kernel's arithmetic against scipy -------------------------------------------------------------------------------------------------
def _edt_cases():
    gen = np.random.default_rng(5)
    shapes = [(7, 33, 70)] * 4 + [(1, 1, 1), (3, 5, 70), (2, 3, 40)]
    return [(shape, gen.random(shape) < (0.003 if n % 2 else 0.02)) for n, shape in enumerate(shapes)]


@pytest.mark.parametrize("spacing,ulps", [((1.0, 1.0, 1.0), 0), ((1.0, 2.0, 3.0), 0), ((1.0, 0.45, 0.47), 8), ((5.0, 0.488281, 0.488281), 8)])
def test_direct_minimum_restatement_against_scipy(spacing, ulps):
    """The separable direct minimum in float64 (what hct_edt3d computes): bit-equal to scipy after the square root on integer spacings,
    where every term is exact; within 8 * 2^-53 relative otherwise -- three rounded products, three rounded squares, two rounded adds
    and a square root on each side, about 2 * 2^-53 at worst in practice."""
    worst = 0.0
    for shape, feat in _edt_cases():
        if not feat.any():
            feat[tuple(s // 2 for s in shape)] = True
        got = np.sqrt(R.edt_direct(feat, spacing))
        want = ndimage.distance_transform_edt(~feat, sampling=spacing)
        if ulps == 0:
            assert np.array_equal(got, want)
        else:
            err = np.abs(got - want) / np.maximum(want, 1e-300)
            worst = max(worst, float(err.max()))
            assert float(err.max()) <= ulps * EPS
    print(f"spacing {spacing}: worst relative error {worst / EPS:.2f} * 2^-53")


def test_direct_minimum_without_features_is_infinite():
    assert np.isinf(R.edt_direct(np.zeros((3, 4, 5), bool), (1.0, 0.5, 2.0))).all()
    assert (R.edt_direct(np.ones((3, 4, 5), bool), (1.0, 0.5, 2.0)) == 0).all()


# ---- planted faults -----------------------------------------------------------------------------------------------------------------------
def _fault_inputs():
    """Inputs that tell every planted fault from the oracle: the end-to-end scan (anisotropic spacing, a blob on the volume's face,
    ignore voxels on the rim), and a thick L-shaped pair whose directed percentiles differ."""
    pred, labels, K = R.scan_case("both")
    shape = (20, 24, 28)
    p2, l2 = np.zeros(shape, np.int16), np.zeros(shape, np.uint8)
    l2[4:14, 4:16, 4:20] = 1
    p2[4:14, 4:16, 4:20] = 1
    p2[6:9, 6:9, 20:27] = 1  # a spur on the prediction only: d(p -> G) has a long tail, d(g -> P) has none
    p3, l3 = np.zeros((3, 3, 8), np.int16), np.zeros((3, 3, 8), np.uint8)
    p3[1, 1, 1], p3[1, 1, 5], l3[1, 1, 0] = 1, 1, 1  # n_p = 2 with distances 0.5 and 2.5: the linear percentile lies between them
    return [(pred, labels, K, (2.5, 0.8, 0.45), 1.0), (p2, l2, 2, (1.0, 1.0, 1.0), 1.0), (p2, l2, 2, SPACING, 1.0), (p3, l3, 2, SPACING, 1.0)]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_inputs_reject_each_planted_fault(fault):
    differs = False
    for pred, labels, K, spacing, tau in _fault_inputs():
        good, bad = R.surface_metrics(pred, labels, K, spacing, tau), R.surface_metrics(pred, labels, K, spacing, tau, faults=(fault,))
        for k in ("HD", "HD95", "ASSD", "NSD", "n_pred", "n_gt"):
            a, b = np.asarray(good[k], np.float64)[1:], np.asarray(bad[k], np.float64)[1:]
            if not np.allclose(a, b, rtol=1e-9, atol=0, equal_nan=True):
                differs = True
    assert differs, fault


# ---- host helpers -------------------------------------------------------------------------------------------------------------------------
def test_voxel_spacing_reads_the_columns():
    aligned = np.diag([0.45, 0.47, 5.0, 1.0])
    assert surface.voxel_spacing(aligned) == (5.0, 0.47, 0.45)
    flipped = np.diag([-0.45, 0.47, -5.0, 1.0])
    flipped[:3, 3] = (100.0, -20.0, 3.0)
    assert surface.voxel_spacing(flipped) == (5.0, 0.47, 0.45)
    permuted = np.array([[0.0, 1.5, 0.0, -10.0], [-0.8, 0.0, 0.0, 12.0], [0.0, 0.0, 2.0, 5.0], [0.0, 0.0, 0.0, 1.0]])  # i -> -y, j -> +x
    assert surface.voxel_spacing(permuted) == (2.0, 1.5, 0.8)
    rot = np.eye(4)
    rot[:2, :2] = 0.5 * np.array([[np.cos(0.3), -np.sin(0.3)], [np.sin(0.3), np.cos(0.3)]])
    assert np.allclose(surface.voxel_spacing(rot), (1.0, 0.5, 0.5), rtol=1e-15)
    zero = np.diag([0.45, 0.0, 5.0, 1.0])
    with pytest.raises(ValueError, match="> 0"):
        surface.voxel_spacing(zero)
    bad = np.diag([0.45, np.nan, 5.0, 1.0])
    with pytest.raises(ValueError):
        surface.voxel_spacing(bad)
    assert "hear" in surface.voxel_spacing.__doc__  # the docstring says that shear is ignored


def test_surface_metrics_refuses_the_cpu_before_any_launch():
    from headct_foundation_amd import _lib
    pred, labels = torch.zeros(3, 4, 5, dtype=torch.int16), torch.zeros(3, 4, 5, dtype=torch.uint8)
    with pytest.raises(_lib.HctError, match="cuda"):
        surface.surface_metrics(pred, labels, 2, (1.0, 1.0, 1.0))
    with pytest.raises(_lib.HctError, match="cuda"):
        surface.distance_transform(labels, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        surface.surface_metrics(pred, labels, 2, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="tolerance"):
        surface.surface_metrics(pred, labels, 2, (1.0, 1.0, 1.0), tolerance_mm=-1.0)


# ---- SurfaceMetrics -----------------------------------------------------------------------------------------------------------------------
def _scan(hd95, assd, nsd, hd):
    return {"HD95": np.array(hd95), "ASSD": np.array(assd), "NSD": np.array(nsd), "HD": np.array(hd)}


def test_surface_metrics_accumulator():
    nan = np.nan
    m = SurfaceMetrics(3)
    m(_scan([nan, 2.0, nan], [nan, 1.0, nan], [nan, 0.5, 0.0], [nan, 4.0, nan]))    # class 2: one mask empty
    m(_scan([nan, 4.0, nan], [nan, 2.0, nan], [nan, 1.0, nan], [nan, 8.0, nan]))    # class 2: both empty, not scored
    m(_scan([nan, nan, 3.0], [nan, nan, 1.5], [nan, nan, 0.25], [nan, nan, 6.0]))   # class 1: both empty
    out = m.compute()
    assert out["ScansScored"] == [0, 2, 2] and out["OneEmpty"] == [0, 0, 1]
    assert np.isnan(out["HD95"][0]) and np.isnan(out["NSD"][0])
    assert (out["HD95"][1], out["ASSD"][1], out["NSD"][1], out["HD"][1]) == (3.0, 1.5, 0.75, 6.0)
    assert (out["HD95"][2], out["ASSD"][2], out["NSD"][2], out["HD"][2]) == (3.0, 1.5, 0.125, 6.0)  # NSD over two scans, distances over one
    m.all_reduce()  # a world of one: nothing changes
    assert m.compute()["ScansScored"] == [0, 2, 2]
    with pytest.raises(ValueError):
        m(_scan([nan, 1.0], [nan, 1.0], [nan, 1.0], [nan, 1.0]))
    m.reset()
    assert m.compute()["ScansScored"] == [0, 0, 0] and np.isnan(m.compute()["NSD"]).all()


# ---- config and ABI -----------------------------------------------------------------------------------------------------------------------
def _args(tmp_path, opts=None, **flags):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    return argparse.Namespace(cfg=str(cfg), opts=opts, local_rank=0, **flags)


def test_surface_config_keys_and_flags(tmp_path):
    from config import get_config
    c = get_config(_args(tmp_path))
    assert c.SEG.SURFACE_METRICS is False and c.SEG.SURFACE_TOLERANCE_MM == 2.0
    c = get_config(_args(tmp_path, native_preds=True, surface_metrics=True, surface_tolerance_mm=1.5))
    assert c.SEG.SURFACE_METRICS is True and c.SEG.SURFACE_TOLERANCE_MM == 1.5
    c = get_config(_args(tmp_path, opts=["SEG.NATIVE_PREDS", "True", "SEG.SURFACE_METRICS", "True", "SEG.SURFACE_TOLERANCE_MM", "0.0"]))
    assert c.SEG.SURFACE_METRICS is True and c.SEG.SURFACE_TOLERANCE_MM == 0.0
    with pytest.raises(ValueError, match="NATIVE_PREDS"):
        get_config(_args(tmp_path, surface_metrics=True))
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="SURFACE_TOLERANCE_MM"):
            get_config(_args(tmp_path, native_preds=True, surface_metrics=True, surface_tolerance_mm=bad))
    src = open(os.path.join(ROOT, "main_segmentation.py")).read()
    assert "--surface_metrics" in src and "--surface_tolerance_mm" in src


def test_surface_symbols_declared_and_exported(lib):
    from headct_foundation_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "headct_hip.h")).read(), flags=re.S)
    for s in ("hct_surface_edges", "hct_surface_edges_workspace_bytes", "hct_edt3d", "hct_surface_stats", "hct_surface_stats_workspace_bytes",
              "hct_surface_select", "hct_surface_select_workspace_bytes"):
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert "surface.hip" in build.SOURCES
    # one partial per workgroup, a workgroup per row (k, j) up to 2048: 8 int64 for the edges, 4 int64 + 4 float64 for the statistics
    assert lib.hct_surface_edges_workspace_bytes(160, 512, 512) == 2048 * 8 * 8
    assert lib.hct_surface_edges_workspace_bytes(3, 5, 70) == 15 * 8 * 8
    assert lib.hct_surface_stats_workspace_bytes(3, 5, 70) == 15 * 4 * 16
    assert lib.hct_surface_edges_workspace_bytes(0, 5, 70) == 0 and lib.hct_surface_stats_workspace_bytes(3, 5, 32769) == 0
    # the select's state (4 prefixes, 4 ranks) and 8 passes x 4 ranks x 256 bins of uint64
    assert lib.hct_surface_select_workspace_bytes() == 64 + 8 * 4 * 256 * 8
