"""CPU: the oracle of the connected-component kernels (tests/components_ref.py) against scipy and against its own planted faults, the
host arithmetic of headct_foundation_amd/components.py (min_voxels_for, workspace queries, hct_cc_tile_dims), LesionMetrics, the config
keys and flags, the ABI, and the refusal of host tensors before any launch."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib, components
from headct_foundation_amd.metrics import LesionMetrics
from tests import components_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = (4, 8, 16)  # a tile small enough that the seam cases of the numpy labeller have seams: shape 2 T + (3, 5, 7) = (11, 21, 39)
CONNS = (6, 18, 26)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_reference_counts_of_the_case_list():
    cases = R.small_cases(TILE)
    assert cases["empty"].shape == (11, 21, 39) and R.seam_corner(TILE) == TILE
    assert R.seam_shape((R.AXIS_LIMIT,) * 3) == R.SEAM_CAP and R.seam_corner((R.AXIS_LIMIT,) * 3) == (17, 34, 67)
    for conn in (6, 26):
        got = tuple(R.label_ref(cases[f"bernoulli_{p}"], conn)[1] for p in (0.08, 0.2, 0.31, 0.5))
        assert got == R.BERNOULLI_COUNTS[conn]
    assert [R.label_ref(cases["checkerboard"], c)[1] for c in CONNS] == [6912, 1, 1]
    assert [R.label_ref(cases["face_diagonal"], c)[1] for c in CONNS] == [40, 1, 1]
    assert [R.label_ref(cases["body_diagonal"], c)[1] for c in CONNS] == [40, 40, 1]
    assert R.label_ref(R.lattice(), 26)[1] == 73728
    for tile in (TILE, (R.AXIS_LIMIT,) * 3):
        big = R.small_cases(tile)
        assert R.label_ref(big["serpentine"], 6)[1] == 1 and R.label_ref(big["comb"], 26)[1] == 1
        assert R.label_ref(big["comb"][:-1], 26)[1] == big["comb"][0].sum() > 50  # the teeth meet in the last plane only
        for d in R.DIRECTIONS:
            name = "".join("-0+"[x + 1] for x in d)
            for conn in CONNS:
                want = 1 if R.allowed(d, conn) else 2
                assert R.label_ref(big["seam_" + name], conn)[1] == want
                if "blobs_" + name in big:
                    assert R.label_ref(big["blobs_" + name], conn)[1] == want
        for name in ("wrap_j", "wrap_k"):
            assert [R.label_ref(big[name], c)[1] for c in CONNS] == [2, 2, 2]
    assert len(R.DIRECTIONS) == 13 and [sum(R.allowed(d, c) for d in R.DIRECTIONS) for c in CONNS] == [3, 9, 13]


def test_numpy_labeller_restates_scipy_and_root_form():
    for name, mask in R.small_cases(TILE).items():
        for conn in CONNS:
            want, n = R.label_ref(mask, conn)
            got, m = R.label_uf(mask, conn, TILE)
            assert m == n and np.array_equal(got, want), (name, conn)
            root = R.root_form(mask, conn)
            flat, idx = want.reshape(-1), np.arange(want.size)
            for c in range(1, min(n, 50) + 1):
                assert (root.reshape(-1)[flat == c] == idx[flat == c].min() + 1).all()
            assert (root[~mask] == 0).all()
    got, m = R.label_uf(R.lattice(), 26)
    assert m == 73728 and np.array_equal(got, R.label_ref(R.lattice(), 26)[0])


@pytest.mark.parametrize("fault", R.FAULTS)
def test_case_list_rejects_every_planted_fault(fault):
    """Each fault a kernel could have changes the labels of at least one case of the list at some connectivity."""
    cases = dict(R.small_cases(TILE))
    if fault == "counter16":
        cases = {"lattice": R.lattice()}
    caught = []
    for name, mask in cases.items():
        for conn in CONNS:
            got, m = R.label_uf(mask, conn, TILE, fault=fault)
            want, n = R.label_ref(mask, conn)
            if m != n or not np.array_equal(got, want):
                caught.append((name, conn))
    assert caught, fault
    names = {n for n, _ in caught}
    if fault.startswith("skip_seam_"):
        assert any(n.startswith("seam_") for n in names) and any(n.startswith("blobs_") for n in names)
    if fault == "row_wrap":
        assert {"wrap_j", "wrap_k"} <= names
    if fault == "conn18_for_26":
        assert "body_diagonal" in names and all(c == 26 for _, c in caught)


def test_restatements_agree_with_scipy():
    from scipy import ndimage
    mask, other = R.bernoulli((9, 20, 31), 0.3, 1), R.bernoulli((9, 20, 31), 0.5, 2)
    lab, n = R.label_ref(mask, 18)
    idx = np.arange(1, n + 1)
    assert np.array_equal(R.sizes_ref(lab, n)[1:], ndimage.sum(mask, lab, idx).astype(np.int64)) and R.sizes_ref(lab, n)[0] == 0
    assert np.array_equal(R.overlap_ref(lab, n, other)[1:], ndimage.sum(other, lab, idx).astype(np.int64))
    pred, labels = R.removal_case()
    for conn in CONNS:
        out = R.remove_small_ref(pred, 3, 12, conn, labels)
        assert out["removed"].tolist() == [0, 4, 4] and out["class_voxels"].sum() == pred.size
        assert out["class_voxels"][1] == 12 + 13 + 12 and (out["counts"][:, 0] + out["counts"][:, 2]).sum() == (labels < 3).sum()
        same = R.remove_small_ref(pred, 3, 1, conn, labels)
        assert np.array_equal(same["pred"], pred) and same["removed"].tolist() == [0, 0, 0]
    p2, l2 = R.lesion_scene()
    for conn in CONNS:
        m = R.lesion_metrics_ref(p2, l2, 2, conn)
        assert (m["n_gt"][1], m["gt_detected"][1], m["n_pred"][1], m["pred_matched"][1]) == (3, 2, 5, 3)
        assert [r[4] for r in m["lesions"] if r[1] == "gt"] == [0, 1, 2 * 4 * 6 + 2 * 4 * 8]
        assert sum(1 for r in m["lesions"] if r[1] == "pred" and r[4] == 0) == 2


# ---- host arithmetic ------------------------------------------------------------------------------------------------------------------------
def test_min_voxels_for_at_exact_boundaries():
    aff = np.diag([0.45, 0.45, 1.0, 1.0])
    assert components.min_voxels_for(0.2025, aff) == 1000  # 0.45 * 0.45 * 1 mm^3 = 0.2025 uL: exactly 1000 voxels
    from headct_foundation_amd.native import class_volumes_ml
    for n in (1, 2, 7, 999, 1000, 1001, 123457):
        v = float(class_volumes_ml(np.array([n]), aff)[0])  # the volume native_volumes.csv would report for n voxels
        assert components.min_voxels_for(v, aff) == n
        assert components.min_voxels_for(v * (1 + 2.0 ** -40), aff) == n + 1  # beyond the 2^-48 a rounded determinant is forgiven
        assert components.min_voxels_for(np.nextafter(v, 0.0), aff) == n and components.min_voxels_for(np.nextafter(v, np.inf), aff) == n
    assert components.min_voxels_for(0.0, aff) == 0 and components.min_voxels_for(1e-12, aff) == 1
    rot = np.array([[0.0, 1.5, 0.0, -10.0], [-0.8, 0.0, 0.0, 12.0], [0.0, 0.0, 2.0, 5.0], [0.0, 0.0, 0.0, 1.0]])
    assert components.min_voxels_for(0.024, rot) == 10 and components.min_voxels_for(0.0241, rot) == 11
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            components.min_voxels_for(bad, aff)
    with pytest.raises(ValueError):
        components.min_voxels_for(1.0, np.zeros((4, 4)))


def _scan(n_gt, n_pred, det, mat):
    return {"n_gt": np.array(n_gt), "n_pred": np.array(n_pred), "gt_detected": np.array(det), "pred_matched": np.array(mat), "lesions": []}


def test_lesion_metrics_accumulator():
    m = LesionMetrics(3)
    m(_scan([0, 3, 0], [0, 5, 2], [0, 2, 0], [0, 3, 0]))
    m(_scan([0, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]))
    out = m.compute()
    assert out["n_gt"] == [0, 4, 0] and out["n_pred"] == [0, 5, 2] and out["gt_detected"] == [0, 2, 0] and out["pred_matched"] == [0, 3, 0]
    assert out["LesionRecall"][1] == 0.5 and out["LesionPrecision"][1] == 0.6 and abs(out["LesionF1"][1] - 2 * 0.5 * 0.6 / 1.1) < 1e-15
    assert np.isnan(out["LesionRecall"][2]) and out["LesionPrecision"][2] == 0.0 and np.isnan(out["LesionF1"][2])  # no truth lesion: recall undefined
    assert all(np.isnan(out[k][0]) for k in ("LesionRecall", "LesionPrecision", "LesionF1"))
    m.all_reduce()  # a world of one: nothing changes
    assert m.compute()["n_gt"] == [0, 4, 0]
    a, b = LesionMetrics(3), LesionMetrics(3)
    a(_scan([0, 3, 0], [0, 5, 2], [0, 2, 0], [0, 3, 0]))
    b(_scan([0, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]))
    a.merge(b)
    x = a.compute()
    assert all(np.array_equal(np.asarray(x[k]), np.asarray(out[k]), equal_nan=True) for k in out)
    z = LesionMetrics(2)
    z(_scan([0, 2], [0, 2], [0, 0], [0, 0]))
    assert z.compute()["LesionRecall"][1] == 0.0 and np.isnan(z.compute()["LesionF1"][1])  # P + R = 0
    for bad in (_scan([0, 1], [0, 1], [0, 0], [0, 0]), _scan([0, 1, 0], [0, 1, 0], [0, 2, 0], [0, 0, 0]), _scan([1, 1, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0]),
                _scan([0.0, 1.0, 0.0], [0, 1, 0], [0, 0, 0], [0, 0, 0])):
        with pytest.raises(ValueError):
            m(bad)
    m.reset()
    assert m.compute()["n_pred"] == [0, 0, 0] and np.isnan(m.compute()["LesionF1"]).all()


# ---- config and ABI -----------------------------------------------------------------------------------------------------------------------
def _args(tmp_path, opts=None, **flags):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    return argparse.Namespace(cfg=str(cfg), opts=opts, local_rank=0, **flags)


def test_component_config_keys_and_flags(tmp_path):
    from config import get_config
    c = get_config(_args(tmp_path))
    assert c.SEG.MIN_COMPONENT_ML == 0.0 and c.SEG.LESION_METRICS is False and c.SEG.COMPONENT_CONNECTIVITY == 26
    c = get_config(_args(tmp_path, native_preds=True, lesion_metrics=True, min_component_ml=0.25, component_connectivity=18))
    assert c.SEG.MIN_COMPONENT_ML == 0.25 and c.SEG.LESION_METRICS is True and c.SEG.COMPONENT_CONNECTIVITY == 18
    c = get_config(_args(tmp_path, opts=["SEG.NATIVE_PREDS", "True", "SEG.LESION_METRICS", "True", "SEG.MIN_COMPONENT_ML", "0.5",
                                         "SEG.COMPONENT_CONNECTIVITY", "6"]))
    assert c.SEG.MIN_COMPONENT_ML == 0.5 and c.SEG.LESION_METRICS is True and c.SEG.COMPONENT_CONNECTIVITY == 6
    c = get_config(_args(tmp_path, min_component_ml=0.0, component_connectivity=6))  # the filter off: no native pass needed
    assert c.SEG.MIN_COMPONENT_ML == 0.0 and c.SEG.COMPONENT_CONNECTIVITY == 6
    with pytest.raises(ValueError, match="NATIVE_PREDS"):
        get_config(_args(tmp_path, lesion_metrics=True))
    with pytest.raises(ValueError, match="NATIVE_PREDS"):
        get_config(_args(tmp_path, min_component_ml=0.1))
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="MIN_COMPONENT_ML"):
            get_config(_args(tmp_path, native_preds=True, min_component_ml=bad))
    for bad in (4, 0, 27, 8):
        with pytest.raises(ValueError, match="COMPONENT_CONNECTIVITY"):
            get_config(_args(tmp_path, native_preds=True, component_connectivity=bad))
    src = open(os.path.join(ROOT, "main_segmentation.py")).read()
    assert all(flag in src for flag in ("--min_component_ml", "--lesion_metrics", "--component_connectivity"))


SYMBOLS = ("hct_cc_masks", "hct_cc_label", "hct_cc_label_workspace_bytes", "hct_cc_compact", "hct_cc_compact_workspace_bytes", "hct_cc_sizes",
           "hct_cc_overlap", "hct_cc_remove_small", "hct_cc_count_small", "hct_seg_recount", "hct_seg_recount_workspace_bytes", "hct_cc_tile_dims")


def test_component_symbols_declared_bound_and_exported(lib):
    from headct_foundation_amd import build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "headct_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert "components.hip" in build.SOURCES


def test_workspace_queries_and_tile_dims_are_host_arithmetic(lib):
    tk, tj, ti = components.tile_dims()
    assert all(1 <= t <= R.AXIS_LIMIT for t in (tk, tj, ti))
    # the numbering: one int32 per chunk of 4096 voxels and one per 1024 chunks, each array rounded up to 8 bytes
    assert lib.hct_cc_compact_workspace_bytes(2, 3, 4) == 8 + 8
    assert lib.hct_cc_compact_workspace_bytes(160, 512, 512) == 10240 * 4 + 10 * 4
    assert lib.hct_cc_compact_workspace_bytes(1, 1, 4097) == 8 + 8 and lib.hct_cc_compact_workspace_bytes(3, 4096, 1) == 16 + 8
    assert lib.hct_cc_compact_workspace_bytes(32767, 32768, 2) == 524272 * 4 + 512 * 4  # 2^31 - 65536 voxels: the top level still fits one workgroup
    # the recount: 4 K int32 per workgroup of 256 voxels, 8192 workgroups at the most
    assert lib.hct_seg_recount_workspace_bytes(2, 3, 4, 2) == 4 * 2 * 4 and lib.hct_seg_recount_workspace_bytes(160, 512, 512, 6) == 8192 * 4 * 6 * 4
    for shape in ((0, 3, 4), (2, 3, 32769), (32768, 32768, 2), (2048, 1024, 1024)):
        assert lib.hct_cc_compact_workspace_bytes(*shape) == 0 and lib.hct_seg_recount_workspace_bytes(*shape, 2) == 0, shape
    assert lib.hct_seg_recount_workspace_bytes(2, 3, 4, 1) == 0 and lib.hct_seg_recount_workspace_bytes(2, 3, 4, 17) == 0
    assert lib.hct_cc_label_workspace_bytes(160, 512, 512) <= 4 * 160 * 512 * 512  # at most a second array of parents


def test_host_tensors_are_refused_before_any_launch():
    u8, i16, i32 = (torch.zeros(2, 3, 4, dtype=d) for d in (torch.uint8, torch.int16, torch.int32))
    for call in (lambda: components.connected_components(u8), lambda: components.component_sizes(i32, 1),
                 lambda: components.remove_small_components(i16, 2, 5), lambda: components.lesion_metrics(i16, u8, 2)):
        with pytest.raises(_lib.HctError, match="cuda"):
            call()
    with pytest.raises(ValueError, match="connectivity"):
        components.connected_components(u8, connectivity=4)
    with pytest.raises(ValueError, match="num_classes"):
        components.lesion_metrics(i16, u8, 1)
