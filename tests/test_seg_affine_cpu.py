"""No GPU: tests/seg_affine_ref.py against torch's grid_sample, planted faults against the case list the GPU file runs the kernel
on (tests/seg_affine_cases.py), the excused share of the general maps, the config keys and flags, the ABI."""
import argparse
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import affine_ref
from tests import seg_affine_cases as C
from tests import seg_affine_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against torch ---------------------------------------------------------------------------------------------------------
def _grid_sample_nearest(labels, mat, S):
    """labels [B, S, S, S] -> grid_sample(mode='nearest', align_corners=True, padding zeros) at the reference's own coordinates,
    normalised: x_norm = 2 q / (S - 1) - 1, grid[..., 0] the contiguous axis."""
    q, _ = R.coords(mat, S)
    grid = torch.from_numpy(2.0 * q[..., ::-1].copy() / (S - 1) - 1.0)
    x = torch.from_numpy(labels.astype(np.float64)).unsqueeze(1)
    return F.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=True)[:, 0].numpy()


def test_reference_equals_grid_sample_away_from_ties():
    """grid_sample rounds half to even and takes its own inside test, so the two are compared where no axis is within 1e-6 of a tie
    or of the volume's border; label values are kept above 0 so that torch's zero padding is told from a voxel."""
    for case in C.lattice_cases():
        S, lab = case["S"], np.maximum(C.gathered(case), 1)
        got = R.affine_labels_ref(lab, case["mat"].numpy(), None, None, 0)
        assert np.array_equal(got, _grid_sample_nearest(lab, case["mat"].numpy(), S).astype(np.uint8)), case["name"]
    compared = 0
    for case in C.general_cases():
        S, lab, mat = case["S"], np.maximum(C.gathered(case), 1), case["mat"].numpy()
        got = R.affine_labels_ref(lab, mat, None, None, 0)
        want = _grid_sample_nearest(lab, mat, S).astype(np.uint8)
        away = ~R.near_tie(mat, S, 1e-6)
        assert np.array_equal(got[away], want[away]), case["name"]
        assert away.mean() > 0.99
        compared += int(away.sum())
        assert 0.05 < (got == 0).mean() < 0.9, "the general maps must push part of the volume out, not all of it"
    assert compared > 3 * 4 * 16 ** 3 * 0.99


def test_lattice_and_tie_cases_are_index_arithmetic():
    """The reference on the exact cases equals integer indexing (what the GPU file compares the kernel to as well)."""
    for case in list(C.lattice_cases()) + list(C.tie_cases()):
        want, lab = C.expected(case), C.gathered(case)
        for b, (perm, sign, t, flip) in enumerate(case["maps"]):
            if case["name"].startswith("ties"):
                idx = C.tie_index(lab[b], t, flip, case["outside"])
            else:
                idx = C.lattice_index(lab[b], perm, sign, t, flip, case["outside"])
            assert np.array_equal(want[b], idx), (case["name"], b)
    # the tie rule in so many words: +1/2 on axis 0 reads the next voxel and leaves the volume at the last one; -1/2 reads the voxel itself
    case = next(C.tie_cases())
    want, lab = C.expected(case), C.gathered(case)
    assert np.array_equal(want[0][:-1], lab[0][1:]) and bool((want[0][-1] == case["outside"]).all())
    assert np.array_equal(want[1], lab[1])


# ---- planted faults ------------------------------------------------------------------------------------------------------------------------
def _faulty(fault):
    """A copy of seg_affine_ref.affine_labels_ref with one fault planted."""
    def ref(labels, mat, fire=None, flip=None, outside=0):
        labels = np.asarray(labels, dtype=np.uint8)
        B, S = labels.shape[0], labels.shape[1]
        out = R.flip_plain(labels, flip)
        if mat is None:
            return out
        mat = np.asarray(mat, dtype=np.float64).reshape(B, 3, 4).copy()
        c = (S - 1) / 2
        r = np.arange(S, dtype=np.float64) - (0.0 if fault == "centre dropped" else c)
        p = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1)
        for b in range(B):
            if fire is not None and not int(fire[b]):
                continue
            A, t = mat[b, :, :3], mat[b, :, 3]
            if fault == "A transposed":
                A = A.T
            if fault == "flip not folded" and flip is not None:  # the fold undone: column k times -1 once more
                A = A * np.array([-1.0 if (int(flip[b]) >> k) & 1 else 1.0 for k in range(3)])
            with np.errstate(invalid="ignore", over="ignore"):
                q = np.einsum("ak,xyzk->xyza", A, p) + (t if fault == "centre dropped" else t + c)
                if fault == "inside test (-1, S)":
                    ok = (q > -1) & (q < S)
                else:
                    ok = (q >= -0.5) & (q < S - 0.5)
            qs = np.where(ok, q, 0.0)
            n = (np.rint(qs) if fault == "round half even" else np.floor(qs + 0.5)).astype(np.int64)
            n = np.clip(n, 0, S - 1)
            inside = ok.all(axis=-1)
            v = labels[b][n[..., 0], n[..., 1], n[..., 2]]
            if fault == "clamp instead of outside":
                qc = np.clip(np.nan_to_num(q), 0, S - 1)
                nc = np.floor(qc + 0.5).astype(np.int64).clip(0, S - 1)
                out[b] = labels[b][nc[..., 0], nc[..., 1], nc[..., 2]]
            else:
                out[b] = np.where(inside, v, np.uint8(0 if fault == "outside hard-wired to 0" else outside))
        return out
    return ref


FAULTS = ["A transposed", "centre dropped", "round half even", "flip not folded", "clamp instead of outside", "inside test (-1, S)",
          "outside hard-wired to 0"]


def test_the_case_list_accepts_the_reference():
    for case in C.small_cases():
        ok, what = C.verify(case, C.expected(case, _faulty(None)))  # the copy without a fault is the reference
        assert ok, what
        assert np.array_equal(C.expected(case, _faulty(None)), C.expected(case))


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_rejected(fault):
    rejected = [case["name"] for case in C.small_cases() if not C.verify(case, C.expected(case, _faulty(fault)))[0]]
    print(f"{fault}: rejected by {rejected}")
    assert rejected, f"no case of the list notices: {fault}"
    if fault == "round half even":  # only the exact half-voxel translations can tell
        assert all(name.startswith("ties") for name in rejected), rejected


# ---- near-tie share ------------------------------------------------------------------------------------------------------------------------
def test_near_tie_share_of_the_general_maps():
    """Computed here in float64 under each case's derived delta: at most 1 % of the firing samples' voxels, and in fact near 1e-3 or
    below (S <= 24: delta is a few 1e-6, the band around the 3 S tie planes of a voxel row is thin)."""
    for case in list(C.general_cases()) + [C.multi_trip_case()]:
        fire = C.firing(case)
        d = R.delta(case["mat"].numpy(), case["S"])[fire]
        share = C.tie_share(case)
        print(f"{case['name']}: delta up to {d.max():.2e}, near-tie share {share:.2e}")
        assert 0 < d.max() < 1e-4
        assert share <= C.CAP
        assert share <= 2e-3


def test_delta_counts_the_roundings_of_the_header():
    assert (affine_ref.KQ, affine_ref.U) == (5, 2.0 ** -24)
    S, mat = 8, np.array([[1.0, 0, 0, 0.25, 0, -2.0, 0, 0, 0, 0, 0.5, -1.0]])
    d = R.delta(mat, S)
    c = 3.5
    assert d.shape == (1, S, S, S, 3)
    assert d[0, 0, 0, 0, 0] == 5 * 2.0 ** -24 * (1.0 * c + 0.25 + c) and d[0, 7, 0, 2, 1] == 5 * 2.0 ** -24 * (2.0 * c + 0.0 + c)
    assert d[0, 1, 2, 7, 2] == 5 * 2.0 ** -24 * (0.5 * c + 1.0 + c)
    tie = R.near_tie(np.array([[1.0, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, 0]]), S, 1e-9)
    assert tie.all()  # a half-voxel translation puts every voxel on a tie
    assert not R.near_tie(np.array([[1.0, 0, 0, 0.25, 0, 1, 0, 0, 0, 0, 1, 0]]), S, 1e-9).any()


# ---- config keys and flags -----------------------------------------------------------------------------------------------------------------
def _args(tmp_path, opts=None, **flags):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    return argparse.Namespace(cfg=str(cfg), opts=opts, local_rank=0, **flags)


def test_seg_affine_keys_and_flags(tmp_path):
    from config import check_segmentation_mode, get_config
    c = get_config(_args(tmp_path))
    assert (c.SEG.AFFINE_PROB, c.SEG.AFFINE_OUTSIDE) == (0.0, "background")
    c = get_config(_args(tmp_path, seg_affine_prob=0.5, seg_affine_outside="ignore", affine_rotate=[10.0], affine_scale=0.2, affine_translate=0.1))
    assert (c.SEG.AFFINE_PROB, c.SEG.AFFINE_OUTSIDE, list(c.TRAIN.AFFINE_ROTATE), c.TRAIN.AFFINE_SCALE, c.TRAIN.AFFINE_TRANSLATE) == \
        (0.5, "ignore", [10.0], 0.2, 0.1)
    assert c.TRAIN.AFFINE_PROB == 0.0
    check_segmentation_mode(c)  # the segmentation node's own switch passes
    c = get_config(_args(tmp_path, seg_affine_prob=0.0, opts=["SEG.AFFINE_PROB", "0.7"]))  # --seg_affine_prob 0 reaches the config
    assert c.SEG.AFFINE_PROB == 0.0
    for flags, key in ((dict(seg_affine_prob=1.5), "SEG.AFFINE_PROB"), (dict(seg_affine_prob=-0.1), "SEG.AFFINE_PROB"),
                       (dict(seg_affine_prob=float("nan")), "SEG.AFFINE_PROB"), (dict(seg_affine_outside="zero"), "SEG.AFFINE_OUTSIDE")):
        with pytest.raises(ValueError, match=key):
            get_config(_args(tmp_path, **flags))
    for opts, key in ((["SEG.AFFINE_OUTSIDE", "edge"], "SEG.AFFINE_OUTSIDE"), (["SEG.AFFINE_PROB", "2.0"], "SEG.AFFINE_PROB")):
        with pytest.raises(ValueError, match=key):
            get_config(_args(tmp_path, opts=opts))
    with pytest.raises(ValueError, match=r"TRAIN\.AFFINE_PROB.*SEG\.AFFINE_PROB"):  # still refused, and says where to go
        check_segmentation_mode(get_config(_args(tmp_path, affine_prob=0.5, seg_affine_prob=0.5)))


def test_segmentation_affine_builds_the_draws_from_the_config(tmp_path):
    from config import get_config
    from headct_foundation_amd.data import AFFINE_OUTSIDE, RandAffine3D, segmentation_affine
    assert AFFINE_OUTSIDE == {"background": 0, "ignore": 255}
    assert segmentation_affine(get_config(_args(tmp_path, seg_affine_outside="ignore")), 7) == (None, 255)
    c = get_config(_args(tmp_path, seg_affine_prob=0.25, affine_rotate=[20.0, 10.0, 5.0], affine_scale=0.2, opts=["TRAIN.AFFINE_ISOTROPIC", "False"]))
    aff, outside = segmentation_affine(c, 7)
    assert isinstance(aff, RandAffine3D) and outside == 0
    assert (aff.rotate_deg, aff.scale, aff.translate, aff.prob, aff.isotropic_scale) == ((20.0, 10.0, 5.0), 0.2, (0.05,) * 3, 0.25, False)
    assert aff.gen.initial_seed() == 7


def test_flags_are_in_main_segmentation():
    src = open(os.path.join(ROOT, "main_segmentation.py")).read()
    for flag in ("--seg_affine_prob", "--seg_affine_outside", "--affine_rotate", "--affine_scale", "--affine_translate"):
        assert f'"{flag}"' in src, flag
    assert "--affine_prob" not in src.replace("--seg_affine_prob", "")  # TRAIN.AFFINE_PROB has no flag here


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_affine_labels_symbol_declared_and_exported(lib):
    from headct_foundation_amd import _lib, affine_labels  # noqa: F401
    hdr = open(os.path.join(ROOT, "include", "headct_hip.h")).read()
    assert re.search(r"\bint\s+hct_affine_labels\s*\(const uint8_t\* pool, const int32_t\* slot, int64_t n_slots, uint8_t\* out, int B, int S,", hdr)
    assert "hct_affine_labels" in _lib._PROTOS and hasattr(lib, "hct_affine_labels")
    assert len(_lib._PROTOS["hct_affine_labels"][1]) == 11
    src = open(os.path.join(ROOT, "headct_foundation_amd", "csrc", "affine.hip")).read()
    # one device function for the coordinates, used by the image kernel and by the label kernel
    assert len(re.findall(r"\baffine_coord\(M, [012], row\[[012]\], p2\)", src)) == 6 and src.count("affine_labels_kernel") >= 2
