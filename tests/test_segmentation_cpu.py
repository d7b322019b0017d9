"""CPU: the segmentation reference (tests/seg_ref.py) checked against autograd, its bounds against an fp32 evaluation and planted
faults, SegmentationMetrics against scikit-learn, the synthetic set's contract, config keys and refusals, the ABI."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import seg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
W_CE, W_DICE = 1.0, 0.5


def _case(name, dtype=F64):
    c = R.LOSS_CASES[name]
    tok, y = R.make_case(c["B"], c["G"], c["P"], c["K"], c["first"], seed=len(name), pad=c["pad"], dtype=dtype)
    return c, tok, y


def _cw(K):
    return torch.linspace(0.5, 2.0, K, dtype=F32)


# ---- layout --------------------------------------------------------------------------------------------------------------------------
def test_layout_maps():
    B, G, P, K, first = 2, 2, 4, 3, 2
    T, S = first + G ** 3, G * P
    tok = torch.arange(B * T * K * P ** 3, dtype=F64).reshape(B, T, K * P ** 3)
    vol = R.unpatchify(tok, first, G, P, K)
    flat = tok.reshape(B * T, -1)
    for (b, c, z, y, x) in [(0, 0, 0, 0, 0), (1, 2, 7, 3, 4), (0, 1, 4, 5, 6), (1, 0, 3, 7, 1)]:
        assert float(vol[b, c, z, y, x]) == float(flat[R.row_of(b, z, y, x, T, first, G, P), R.column_of(c, z % P, y % P, x % P, P)])
    back = R.patchify(vol, first, T, G, P)
    assert torch.equal(back[:, first:], tok[:, first:]) and bool((back[:, :first] == 0).all())


def test_cases_cover_the_kernel_paths():
    """The shapes of the GPU loss test reach what they are named for (restated work split of the kernels)."""
    C = R.LOSS_CASES
    split = lambda c: R.work_split(c["G"] * c["P"], 4 if (c["P"] % 4 == 0 and (c["K"] * c["P"] ** 3 + c["pad"]) % 4 == 0) else 1)
    assert C["odd_K_first2"]["K"] % 2 == 1 and C["odd_K_first2"]["first"] == 2
    assert C["P12_vector_tail"]["P"] ** 3 == 1728 and split(C["P12_vector_tail"])[0] % 256 != 0
    assert split(C["two_partials"])[2] == 2 and C["two_partials"]["B"] == 5
    assert C["no_leading_rows"]["first"] == 0
    assert C["second_finalize_trip"]["B"] * C["second_finalize_trip"]["K"] > 256
    assert (C["one_voxel_access"]["K"] * C["one_voxel_access"]["P"] ** 3 + C["one_voxel_access"]["pad"]) % 4 != 0 and split(C["one_voxel_access"])[2] == 2
    assert C["K_below_bound"]["K"] == 5 and C["K16"]["K"] == 16
    assert R.work_split(96, 4) == (221184, 14, 62)  # ViT-B / 12^3 at 96^3: at most 64 blocks per sample


# ---- the closed form against autograd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["no_leading_rows", "odd_K_first2", "two_partials"])
@pytest.mark.parametrize("weighted", [False, True])
def test_closed_form_gradient_equals_autograd(name, weighted):
    """K = 2 and 3, ignore voxels, an absent class (sample 0) and an all-ignored sample (the last), against float64 autograd of the
    plain torch composition."""
    c, tok, y = _case(name)
    K = c["K"]
    assert not bool((y[0] == K - 1).any()) and bool((y[-1] == 255).all()) and bool((y[:-1] == 255).any())
    x = R.unpatchify(tok, c["first"], c["G"], c["P"], K).clone().requires_grad_(True)
    cw = _cw(K).to(F64) if weighted else None
    loss = R.loss_composed(x, y, W_CE, W_DICE, cw)
    loss.backward()
    r = R.loss_parts(x.detach(), y, W_CE, W_DICE, cw)
    assert abs(float(loss.detach()) - float(r["loss"])) < 1e-12
    assert float((x.grad - r["grad"]).abs().max()) < 1e-14
    assert bool((r["grad"][-1] == 0).all()) and bool((r["dice_bc"][-1] == 1).all())
    ign = (y == 255).unsqueeze(1).expand_as(x)
    assert bool((r["grad"][ign] == 0).all())
    # against torch's own cross-entropy
    ce = torch.nn.functional.cross_entropy(x.detach(), y.to(torch.int64), weight=cw, ignore_index=255)
    assert abs(float(ce) - float(r["ce"])) < 1e-12


def test_no_valid_voxel_convention():
    c, tok, y = _case("no_leading_rows")
    x = R.unpatchify(tok, c["first"], c["G"], c["P"], c["K"])
    r = R.loss_parts(x, torch.full_like(y, 255), W_CE, W_DICE)
    assert float(r["loss"]) == 0.0 and float(r["ce"]) == 0.0 and float(r["dice"]) == 0.0 and bool((r["grad"] == 0).all())


# ---- bounds: an fp32 evaluation in another order holds them, planted faults do not -----------------------------------------------------
def _fp32_eval(tok, y, c, cw, fault=None):
    """The loss in fp32 torch ops on the token layout (a summation order of torch's choosing), with optional planted faults."""
    K, P, G, first = c["K"], c["P"], c["G"], c["first"]
    B = tok.shape[0]
    y = y.clone()
    if fault == "label":
        v = (y[0] < K).nonzero()[0]
        y[0, v[0], v[1], v[2]] = (int(y[0, v[0], v[1], v[2]]) + 1) % K
    if fault == "first_rows":   # the leading rows counted as voxels: the patches are read one row early
        x = R.unpatchify(torch.nan_to_num(tok.to(F32), nan=0.0), first - 1, G, P, K)
    elif fault == "swapped":    # voxel-major columns read as class-major
        t = tok[:, first:, :K * P ** 3].to(F32).reshape(B, G ** 3, P ** 3, K).transpose(2, 3).reshape(B, G ** 3, K * P ** 3)
        x = R.unpatchify(t, 0, G, P, K)
    else:
        x = R.unpatchify(tok.to(F32), first, G, P, K)
    yl = y.to(torch.int64)
    valid = yl < K
    oh = torch.nn.functional.one_hot(torch.where(valid, yl, torch.zeros_like(yl)), K).movedim(-1, 1).to(F32) * valid.unsqueeze(1)
    p = torch.softmax(x, dim=1)
    wy = (oh * cw.view(1, K, 1, 1, 1)).sum(1)
    nll = -(torch.log_softmax(x, dim=1) * oh).sum(1)
    ce = (wy * nll).sum() / wy.sum()
    vm = valid.unsqueeze(1).to(F32)
    I, Pc, Y = (p * oh).flatten(2).sum(2), (p * vm).flatten(2).sum(2), oh.flatten(2).sum(2)
    eps = 0.0 if fault == "no_eps" else R.EPS
    d = (2 * I + eps) / (Pc + Y + eps)
    d = torch.nan_to_num(d, nan=1.0)
    terms = 1 - d
    if fault == "dropped_sample":
        terms = terms[1:]
        dice = terms.sum() / (B * K)
    else:
        dice = terms.mean()
    return dict(loss=W_CE * ce + W_DICE * dice, ce=ce, dice=dice, dice_bc=d)


def _inside(got, r, bd):
    ok = all(abs(float(got[k]) - float(r[k])) <= float(bd[k]) for k in ("loss", "ce", "dice"))
    return ok and bool(((got["dice_bc"].to(F64) - r["dice_bc"]).abs() <= bd["dice_bc"]).all())


@pytest.mark.parametrize("name", ["odd_K_first2", "two_partials"])
def test_bounds_hold_fp32_and_reject_planted_faults(name):
    c, tok, y = _case(name, F32)
    K = c["K"]
    cw = _cw(K)
    r = R.loss_parts(R.unpatchify(tok.to(F64), c["first"], c["G"], c["P"], K), y, W_CE, W_DICE, cw)
    # torch's fp32 sums are pairwise over the whole sample: no deeper than the kernel's thread run + block tree
    bd = R.loss_bounds(r, K, W_CE, W_DICE, run=4)
    assert _inside(_fp32_eval(tok, y, c, cw), r, bd)
    for fault in ("label", "dropped_sample", "no_eps", "first_rows", "swapped"):
        assert not _inside(_fp32_eval(tok, y, c, cw, fault), r, bd), fault
    # the gradient's bound: the float64 closed form rounded to fp32 lies inside, a gradient with one voxel's label wrong does not
    g32 = r["grad"].to(F32).to(F64)
    assert bool(((g32 - r["grad"]).abs() <= bd["grad"]).all())
    y2 = y.clone()
    v = (y2[0] < K).nonzero()[0]
    y2[0, v[0], v[1], v[2]] = (int(y2[0, v[0], v[1], v[2]]) + 1) % K
    r2 = R.loss_parts(R.unpatchify(tok.to(F64), c["first"], c["G"], c["P"], K), y2, W_CE, W_DICE, cw)
    assert not bool(((r2["grad"] - r["grad"]).abs() <= bd["grad"]).all())
    # relative size: the bounds are a few ulps of the quantities, not a loose tolerance
    assert float(bd["loss"]) < 1e-5 * float(r["loss"]) and float(bd["dice_bc"].max()) < 1e-5


# ---- prediction, counts, metrics -------------------------------------------------------------------------------------------------------
def test_predict_ties_and_counts():
    x = torch.zeros(1, 3, 2, 2, 2, dtype=F64)
    x[0, 2, 0, 0, 0] = 1.0
    x[0, 1, 0, 0, 1] = x[0, 2, 0, 0, 1] = 2.0
    pred = R.predict(x)
    assert int(pred[0, 0, 0, 0]) == 2 and int(pred[0, 0, 0, 1]) == 1 and int(pred[0, 1, 1, 1]) == 0
    y = torch.zeros(1, 2, 2, 2, dtype=torch.uint8)
    y[0, 0, 0, 0], y[0, 0, 0, 1], y[0, 1, 1, 1] = 2, 2, 255
    cnt = R.counts(pred, y, 3)
    assert cnt[0].tolist() == [[5, 0, 0], [0, 1, 0], [1, 0, 1]]


def test_segmentation_metrics_against_sklearn():
    from sklearn.metrics import f1_score, jaccard_score
    from headct_foundation_amd.metrics import SegmentationMetrics
    gen = torch.Generator().manual_seed(0)
    K, B, S = 4, 6, 6
    y = torch.randint(0, K, (B, S, S, S), generator=gen).to(torch.uint8)
    pred = torch.where(torch.rand(B, S, S, S, generator=gen) < 0.6, y, torch.randint(0, K, (B, S, S, S), generator=gen).to(torch.uint8))
    y[torch.rand(B, S, S, S, generator=gen) < 0.1] = 255
    y[0][y[0] == 3] = 0   # class 3 absent from scan 0
    m = SegmentationMetrics(K)
    m(R.counts(pred[:4], y[:4], K))
    m(torch.from_numpy(R.counts(pred[4:], y[4:], K)))
    out = m.compute()
    valid = (y != 255).numpy().reshape(-1)
    yt, yp = y.numpy().reshape(-1)[valid], pred.numpy().reshape(-1)[valid]
    assert np.allclose(out["DiceGlobal"], f1_score(yt, yp, labels=list(range(K)), average=None), atol=1e-12)
    assert np.allclose(out["IoUGlobal"], jaccard_score(yt, yp, labels=list(range(K)), average=None), atol=1e-12)
    per = []
    for b in range(B):
        v = (y[b] != 255).numpy().reshape(-1)
        per.append(f1_score(y[b].numpy().reshape(-1)[v], pred[b].numpy().reshape(-1)[v], labels=list(range(K)), average=None, zero_division=0.0))
    per = np.array(per)
    present = np.array([[bool((y[b] == c).any()) for c in range(K)] for b in range(B)])
    want = np.array([per[present[:, c], c].mean() for c in range(K)])
    assert np.allclose(out["DiceScan"], want, atol=1e-12) and out["ScansPresent"].tolist() == present.sum(0).tolist()
    assert out["ScansPresent"][3] == B - 1
    ref = R.metrics(R.counts(pred, y, K))
    assert np.allclose(ref["dice_global"], out["DiceGlobal"]) and np.allclose(ref["dice_scan"], out["DiceScan"])
    m.reset()
    assert np.isnan(m.compute()["DiceGlobal"]).all()
    with pytest.raises(ValueError):
        m(np.zeros((2, K + 1, 3)))


def test_flip_labels_reference():
    pool = torch.arange(2 * 4 * 4 * 4, dtype=torch.int64).reshape(2, 4, 4, 4).to(torch.uint8)
    out = R.flip_labels(pool, [1, 0, -1], [5, 2, 7])
    assert torch.equal(out[0], pool[1].flip(0).flip(2)) and torch.equal(out[1], pool[0].flip(1)) and bool((out[2] == 255).all())


def test_constant_prediction_is_the_prior():
    y = torch.zeros(2, 4, 4, 4, dtype=torch.uint8)
    y[:, :2, :2, :2] = 1
    y[0, 3] = 255
    c = R.constant_prediction(y, 2)
    valid = y != 255
    prior = torch.tensor([float((y[valid] == k).sum()) for k in range(2)], dtype=F64) / float(valid.sum())
    ce = -float((prior * prior.log()).sum())
    assert c["fg_dice"] == 0.0 and c["loss"] > ce  # cross-entropy at the prior is its entropy; the Dice term adds to it


# ---- the nearest-neighbour label item -----------------------------------------------------------------------------------------------
def test_label_item_identity():
    """A 1 mm RAS file whose foreground box is the whole volume and whose roi equals its size: the item is the mask."""
    gen = np.random.default_rng(0)
    mask = gen.integers(0, 4, (5, 7, 6)).astype(np.float32)
    got = R.label_item(mask, m=mask.shape, steps=(1.0, 1.0, 1.0), box_start=(0, 0, 0), box_size=mask.shape, roi=mask.shape)
    assert got.dtype == np.uint8 and np.array_equal(got, mask.astype(np.uint8))


def test_label_item_anisotropic_against_plain_loops():
    """Anisotropic spacing, a box at a non-zero offset, a roi that neither divides nor is divided by the box: against the integer
    arithmetic written out as plain loops; the loader's tables are the reference's."""
    from headct_foundation_amd import nifti
    from headct_foundation_amd.data import nearest_tables
    gen = np.random.default_rng(1)
    d, zooms, roi = (9, 14, 11), (2.5, 0.7, 1.3), (8, 6, 10)
    mask = gen.integers(0, 3, d).astype(np.float32)
    geom = [nifti.spacing_geometry(d[a], zooms[a]) for a in range(3)]
    m, steps = [g[0] for g in geom], [g[1] for g in geom]
    start, size = (3, 1, 2), (m[0] - 5, m[1] - 2, m[2] - 4)
    got = R.label_item(mask, m, steps, start, size, roi)
    want = np.zeros(roi, np.uint8)
    src = []
    for a in range(3):
        row = []
        for o in range(roi[a]):
            c = start[a] + min(size[a] - 1, ((2 * o + 1) * size[a]) // (2 * roi[a]))
            row.append(min(max(int(np.floor(c * steps[a] + 0.5)), 0), d[a] - 1))
        src.append(row)
    for i in range(roi[0]):
        for j in range(roi[1]):
            for k in range(roi[2]):
                want[i, j, k] = mask[src[0][i], src[1][j], src[2][k]]
    assert np.array_equal(got, want)
    assert np.array_equal(nearest_tables(d, m, steps), np.concatenate([R.nearest_axis(d[a], m[a], steps[a]) for a in range(3)]).astype(np.int32))
    assert all(0 <= min(r) and max(r) < d[a] for a, r in enumerate(src))
    bad = mask.copy()
    bad[src[0][0], src[1][0], src[2][0]] = 300.0
    with pytest.raises(ValueError):
        R.label_item(bad, m, steps, start, size, roi)
    bad[src[0][0], src[1][0], src[2][0]] = 1.5
    with pytest.raises(ValueError):
        R.label_item(bad, m, steps, start, size, roi)


def test_read_segmentation_paths(tmp_path):
    from headct_foundation_amd.data import LabelCache, VolumeCache, read_segmentation_paths
    f = tmp_path / "seg.csv"
    f.write_text("img_path,seg_path,site\n/a/1.nii.gz,/a/1_seg.nii.gz,x\n/a/2.nii,/a/2_seg.nii,y\n")
    assert read_segmentation_paths(f) == [("/a/1.nii.gz", "/a/1_seg.nii.gz"), ("/a/2.nii", "/a/2_seg.nii")]
    g = tmp_path / "bad.csv"
    g.write_text("img_path,label\n/a/1.nii.gz,0\n")
    with pytest.raises(ValueError, match="seg_path"):
        read_segmentation_paths(g)
    lc, vc = LabelCache(tmp_path / "c", 16, 3), VolumeCache(tmp_path / "c", 16, 3)
    assert lc.key("/a/1.nii", "/a/1_seg.nii") != vc.key("/a/1.nii") and lc.key("/a/1.nii", "/a/1_seg.nii") != lc.key("/a/1.nii", "/a/other.nii")
    assert os.path.dirname(lc.file_of("/a/1.nii", "/s")) == os.path.dirname(vc.file_of("/a/1.nii"))


# ---- the synthetic set ----------------------------------------------------------------------------------------------------------------
def test_synthetic_segmented_contract():
    from headct_foundation_amd.data import SyntheticSegmented
    K, S, P, bs = 3, 24, 12, 8
    d = SyntheticSegmented(3, bs, 2, S, K, "cpu", seed=1)
    assert d.reuses_batches and len(d) == 3
    straddle = inside = 0
    for i, (v, y, names) in enumerate(d):
        assert tuple(v.shape) == (bs, 2, S, S, S) and v.dtype == F32 and y.dtype == torch.uint8 and tuple(y.shape) == (bs, S, S, S)
        assert len(names) == bs and len(set(names)) == bs
        for b in range(bs):
            r = i * bs + b
            assert bool((y[b] == K - 1).any()) == (r % 3 != 2), r      # class K - 1 absent from every third sample
            assert bool((y[b] == 255).any()) == (r % 4 == 3), r        # a shell of ignore voxels in every fourth
            assert bool((y[b] == 1).any())
            for (c, z0, z1, y0, y1, x0, x1) in d.boxes[i][b]:
                cross = any(lo // P != (hi - 1) // P for lo, hi in ((z0, z1), (y0, y1), (x0, x1)))
                straddle += cross
                inside += not cross
            c, z0, z1, y0, y1, x0, x1 = d.boxes[i][b][-1]  # the last box is painted over by none
            assert bool((y[b, z0:z1, y0:y1, x0:x1] == c).all())
            assert float(v[b, :, z0:z1, y0:y1, x0:x1].min()) >= 0.5 * c and float(v[b].max()) < 1.0 + 0.5 * (K - 1)
            if r % 4 == 3 and z0 > 0:
                assert bool((y[b, z0 - 1, y0:y1, x0:x1] == 255).all())
    assert straddle > 0 and inside > 0
    d2 = SyntheticSegmented(3, bs, 2, S, K, "cpu", seed=1)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(d, d2))


# ---- config ----------------------------------------------------------------------------------------------------------------------------
def _args(tmp_path, opts=None, **flags):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    return argparse.Namespace(cfg=str(cfg), opts=opts, local_rank=0, **flags)


def test_seg_config_keys_and_flags(tmp_path):
    from config import get_config
    c = get_config(_args(tmp_path))
    assert (c.SEG.NUM_CLASSES, c.SEG.CE_WEIGHT, c.SEG.DICE_WEIGHT, list(c.SEG.CLASS_WEIGHT), c.SEG.IGNORE_INDEX, c.SEG.SAVE_PREDS) == \
        (2, 1.0, 1.0, [], 255, False)
    c = get_config(_args(tmp_path, seg_classes=4, dice_weight=0.0, ce_weight=2.0, save_preds=True))
    assert (c.SEG.NUM_CLASSES, c.SEG.CE_WEIGHT, c.SEG.DICE_WEIGHT, c.SEG.SAVE_PREDS) == (4, 2.0, 0.0, True)
    c = get_config(_args(tmp_path, opts=["SEG.NUM_CLASSES", "3", "SEG.CLASS_WEIGHT", "[1.0, 2.0, 4.0]"]))
    assert list(c.SEG.CLASS_WEIGHT) == [1.0, 2.0, 4.0]
    for bad in (dict(seg_classes=1), dict(seg_classes=17), dict(dice_weight=-1.0), dict(dice_weight=0.0, ce_weight=0.0)):
        with pytest.raises(ValueError, match="SEG"):
            get_config(_args(tmp_path, **bad))
    for opts in (["SEG.IGNORE_INDEX", "0"], ["SEG.CLASS_WEIGHT", "[1.0, 2.0, 3.0]"], ["SEG.CLASS_WEIGHT", "[0.0, 0.0]"]):
        with pytest.raises(ValueError, match="SEG"):
            get_config(_args(tmp_path, opts=opts))


def test_segmentation_mode_refusals(tmp_path):
    from config import check_segmentation_mode, get_config
    check_segmentation_mode(get_config(_args(tmp_path)))
    # what lives in the backbone or the optimizer passes
    check_segmentation_mode(get_config(_args(tmp_path, lock=True, layer_decay=0.75, drop_path=0.1, wd_exclude_1d=True,
                                             opts=["TRAIN.LORA", "True", "VIT.NUM_REGISTER_TOKENS", "4", "MAE.NORM_LAYER", "rmsnorm", "VIT.DROPOUT_RATE", "0.1"])))
    for flags, word in ((dict(affine_prob=0.5), "AFFINE_PROB"), (dict(mixup=0.2), "MIXUP"), (dict(cutmix=1.0), "CUTMIX"),
                        (dict(patch_dropout=0.25), "PATCH_DROPOUT")):
        with pytest.raises(ValueError, match=word):
            check_segmentation_mode(get_config(_args(tmp_path, **flags)))


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
SEG_SYMBOLS = ["hct_seg_loss_workspace_bytes", "hct_seg_loss", "hct_seg_predict_workspace_bytes", "hct_seg_predict", "hct_gather_flip_labels",
               "hct_label_to_item"]


def test_seg_symbols_declared_and_exported(lib):
    from headct_foundation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "headct_hip.h")).read()
    for name in SEG_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib._PROTOS and hasattr(lib, name), name
    assert lib.hct_seg_loss_workspace_bytes(2, 2, 4, 3) > 0 and lib.hct_seg_predict_workspace_bytes(2, 2, 4, 3) > 0
    assert "segmentation.hip" in __import__("headct_foundation_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "PROF_SEG" in open(os.path.join(ROOT, "headct_foundation_amd", "csrc", "prof.h")).read()


def test_head_layout_and_cpu_refusal():
    from headct_foundation_amd import _lib
    from headct_foundation_amd.segmentation import SegmentationHead, seg_loss
    h = SegmentationHead(64, 4, 3)
    assert tuple(h.linear.weight.shape) == (3 * 64, 64) and tuple(h.linear.bias.shape) == (3 * 64,)
    assert set(h.state_dict()) == {"linear.weight", "linear.bias"}
    with pytest.raises(_lib.HctError):
        h(torch.zeros(1, 9, 64))
    with pytest.raises(_lib.HctError):
        seg_loss(torch.zeros(1, 8, 3 * 64), torch.zeros(1, 8, 8, 8, dtype=torch.uint8), 4, 3)
    with pytest.raises(ValueError):
        SegmentationHead(64, 4, 17)
