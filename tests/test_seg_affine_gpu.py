"""GPU: hct_affine_labels through the C ABI on the cases of tests/seg_affine_cases.py against tests/seg_affine_ref.py (float64), then
the loaders that carry it, training under it and main_segmentation.py end to end.

Every kernel call writes into an output between sentinel margins (99) that must come back untouched, reads a pool that sits between
sentinel regions (253, a value no label volume holds: a load outside the pool would show in the output), and is made twice on fresh
outputs that must agree bit for bit.  Exact cases -- the plain path, lattice maps, half-voxel translations -- are held to equality,
against hct_gather_flip_labels itself and against integer indexing; general maps are bit-equal to the reference outside
`seg_affine_ref.near_tie` (whose delta is derived from the header's order of operations) and one of the two candidates inside it.

Measured on an MI355X: the general maps excuse at most 7e-5 of their voxels (cap 1e-2); training under the affine goes from a loss
of 2.007 to 0.874 in 30 steps, the best constant prediction being 0.907."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd.data import (AugmentedSegmented, DeviceAugment, LabelCache, RandAffine3D, SegmentedVolumes, SyntheticSegmented, VolumeCache,
                                        affine_augment, affine_matrices, get_segmentation_dataloaders, read_segmentation_paths)
from headct_foundation_amd.segmentation import affine_labels
from tests import affine_ref
from tests import seg_affine_cases as C
from tests import seg_affine_ref as R
from tests import seg_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HCT_E_BADARG = -1
POOL_SENTINEL, OUT_SENTINEL, GUARD = 253, 99, 256


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Guarded:
    """uint8 data of `shape` between two sentinel regions of GUARD bytes (a multiple of 4: the body keeps the buffer's alignment)."""

    def __init__(self, shape, dev, fill, data=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
        self.fill, self.n = fill, n
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if data is not None:
            self.t.copy_(torch.as_tensor(data))
        self.ptr = self.t.data_ptr()

    def result(self):
        assert bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all()), "sentinel margin written"
        return self.t.cpu().numpy()


class _Launch:
    """The device side of a case: the pool between sentinels and the tables, kept alive; `run` makes one call into a fresh output."""

    def __init__(self, case, dev):
        self.case, self.dev = case, dev
        self.B, self.S = len(case["slots"]), case["S"]
        self.pool = _Guarded(case["pool"].shape, dev, POOL_SENTINEL, case["pool"])
        up = lambda v, dt: None if v is None else torch.as_tensor(v).to(device=dev, dtype=dt).contiguous()
        self.slot = up(case["slots"], torch.int32)
        self.mat, self.fire, self.flip = up(case["mat"], torch.float32), up(case["fire"], torch.uint8), up(case["flip"], torch.uint8)

    def run(self, lib, mat="case", outside=None):
        out = _Guarded((self.B, self.S, self.S, self.S), self.dev, OUT_SENTINEL)
        m = self.mat if isinstance(mat, str) else mat
        rc = lib.hct_affine_labels(self.pool.ptr, self.slot.data_ptr(), self.case["pool"].shape[0], out.ptr, self.B, self.S, _ptr(m), _ptr(self.fire),
                                   _ptr(self.flip), self.case["outside"] if outside is None else outside, _st())
        assert rc == 0, lib.hct_last_error_string()
        return out

    def twice(self, lib, **kw):
        a, b = self.run(lib, **kw), self.run(lib, **kw)
        torch.cuda.synchronize()
        x, y = a.result(), b.result()
        assert np.array_equal(x, y), "a second identical call differs"
        assert not (x == POOL_SENTINEL).any(), "a byte from outside the pool reached the output"
        self.pool.result()
        return x


SMALL = C.small_cases()


# ---- 1. the case list -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_case_list(lib, cuda, case):
    launch = _Launch(case, cuda)
    got = launch.twice(lib)
    ok, what = C.verify(case, got)
    print(what)
    assert ok, what
    lab = C.gathered(case)
    if case["name"].startswith("plain"):
        # the plain path IS hct_gather_flip_labels: bit-equal to that entry point's own output
        ref = _Guarded(got.shape, cuda, OUT_SENTINEL)
        _lib.check(lib.hct_gather_flip_labels(launch.pool.ptr, launch.slot.data_ptr(), ref.ptr, launch.B, launch.S, C.N_SLOTS, _ptr(launch.flip), _st()),
                   "hct_gather_flip_labels")
        torch.cuda.synchronize()
        assert np.array_equal(got, ref.result())
        assert bool((got[case["slots"].index(-1)] == 255).all())
    for b, m in enumerate(case.get("maps", [])):
        perm, sign, t, flip = m
        want = C.tie_index(lab[b], t, flip, case["outside"]) if case["name"].startswith("ties") else C.lattice_index(lab[b], perm, sign, t, flip, case["outside"])
        assert np.array_equal(got[b], want), (case["name"], b, m)
    if case["name"].startswith("ties"):  # q = n + 1/2 takes n + 1; q = S - 1/2 is outside; q = -1/2 is voxel 0
        assert np.array_equal(got[0][:-1], lab[0][1:]) and bool((got[0][-1] == case["outside"]).all()) and np.array_equal(got[1], lab[1])


def test_more_than_one_trip(lib, cuda):
    """B = 64, S = 44: the smallest shape at which a workgroup takes a second trip of its grid-stride loop with a partial last trip
    (21296 threads' work per sample for 64 blocks = 16384 threads; S = 40 fits in one trip) -- seg_affine_cases.multi_trip_case."""
    case = C.multi_trip_case()
    S, B = case["S"], len(case["slots"])
    work, blocks = S * S * (S // 4), min(math.ceil(S * S * (S // 4) / 256), math.ceil(4096 / B))
    assert blocks * 256 < work < 2 * blocks * 256 and 40 * 40 * 10 <= blocks * 256
    got = _Launch(case, cuda).twice(lib)
    ok, what = C.verify(case, got)
    print(what)
    assert ok, what
    assert bool((got[17] == 255).all())  # the placeholder


# ---- 2. degenerate matrices ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_matrices_are_all_outside_and_the_neighbours_do_not_notice(lib, cuda):
    case = dict(next(c for c in C.general_cases() if c["name"] == "general S16 fire NULL"))
    launch = _Launch(case, cuda)
    base = launch.twice(lib)
    B = len(case["slots"])
    for b in range(B):
        for col, bad in ((3, 1e30), (7, -1e30), (11, 1e30), (0, 1e30), (5, -3e38), (2, float("nan")), (3, float("nan")), (9, float("inf"))):
            mat = case["mat"].clone()
            mat[b, col] = bad
            got = launch.twice(lib, mat=mat.to(cuda))
            assert bool((got[b] == case["outside"]).all()), (b, col, bad)
            others = [o for o in range(B) if o != b]
            assert np.array_equal(got[others], base[others]), (b, col, bad)


# ---- 3. image and labels share coordinates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [16, 20])
def test_image_and_labels_share_coordinates(lib, cuda, S):
    """Channels holding i, j, k through hct_affine_augment give q (the interpolant of a linear function is the function); label
    volumes holding i, j, k through hct_affine_labels give n.  Wherever all eight taps are inside, |n_a - q_a| <= 1/2 + bound."""
    B = 4
    mat = C.general_mats(B, S, 20 + S, [3, 0, 6, 5])
    r = torch.arange(S, dtype=torch.float32)
    x = torch.stack(torch.meshgrid(r, r, r, indexing="ij")).unsqueeze(0).expand(B, 3, S, S, S).contiguous()
    qhat = affine_augment(x.to(cuda), mat).cpu().double()
    bound = affine_ref.bound(x, mat)
    q, _ = affine_ref._coords(mat, S)
    inside, f, _ = affine_ref._cells(q, S)
    eight = (inside & (f >= 0) & (f + 1 < S)).all(dim=-1)
    assert 0.2 < float(eight.double().mean()) < 1.0
    pool = x[0].to(torch.uint8).to(cuda)  # slot a holds the index along axis a
    worst = -math.inf
    for a in range(3):
        n = affine_labels(pool, torch.full((B,), a, dtype=torch.int32), mat, outside=255).cpu()
        assert bool((n[eight] < S).all()), "a voxel with all eight taps inside was called outside"
        err = (n.double() - qhat[:, a]).abs()[eight]
        lim = 0.5 + bound[:, a][eight]
        worst = max(worst, float((err - lim).max()))
        assert bool((err <= lim).all()), (a, float((err - lim).max()))
    print(f"S {S}: worst |n - q| - (1/2 + bound) = {worst:.3e}")


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(lib, cuda):
    B, S, n = 2, 8, 3
    pool = torch.as_tensor(C.volumes(n, S)).to(cuda)
    out = _Guarded((B, S, S, S), cuda, OUT_SENTINEL)
    slot = torch.zeros(B, dtype=torch.int32, device=cuda)
    mat = affine_matrices(torch.zeros(B, 3), torch.ones(B, 3), torch.zeros(B, 3)).to(cuda)
    fire = torch.ones(B, dtype=torch.uint8, device=cuda)
    ok = dict(pool=pool.data_ptr(), slot=slot.data_ptr(), n=n, out=out.ptr, B=B, S=S, mat=mat.data_ptr(), fire=fire.data_ptr(), flip=None, outside=0)
    call = lambda **kw: lib.hct_affine_labels(*[{**ok, **kw}[k] for k in ("pool", "slot", "n", "out", "B", "S", "mat", "fire", "flip", "outside")], _st())
    for kw, word in ((dict(S=10), "multiple of 4"), (dict(S=0), "multiple of 4"), (dict(S=1028), "at most 1024"), (dict(B=0), "bad arguments"),
                     (dict(B=65536), "65535"), (dict(pool=None), "bad arguments"), (dict(slot=None), "needs a slot"), (dict(out=None), "bad arguments"),
                     (dict(n=0), "bad arguments"), (dict(out=pool.data_ptr()), "out must not be the pool"), (dict(out=out.ptr + 2), "4-byte aligned"),
                     (dict(pool=pool.data_ptr() + 1), "4-byte aligned"), (dict(mat=None), "fire without mat")):
        assert call(**kw) == HCT_E_BADARG, kw
        msg = lib.hct_last_error_string().decode()
        assert "hct_affine_labels" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert bool((out.result() == OUT_SENTINEL).all()), "a refused call wrote"
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.result(), pool[:1].expand(B, S, S, S).cpu().numpy())  # the identity
    # the Python door: _checked_mat's refusals and gather_flip_labels'
    slots = torch.tensor([0, 1], dtype=torch.int32)
    for bad in (float("nan"), float("inf")):
        m = mat.cpu().clone()
        m[1, 5] = bad
        with pytest.raises(ValueError, match="non-finite"):
            affine_labels(pool, slots, m)
    with pytest.raises(ValueError, match="fire without mat"):
        affine_labels(pool, slots, None, fire)
    with pytest.raises(ValueError, match="12"):
        affine_labels(pool, slots, mat.cpu()[:1])
    with pytest.raises(ValueError, match="outside"):
        affine_labels(pool, slots, mat, outside=256)
    with pytest.raises(_lib.HctError, match="flip"):
        affine_labels(pool, slots, mat, flip=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(_lib.HctError, match="pool uint8"):
        affine_labels(pool.cpu(), slots, mat)
    assert torch.equal(affine_labels(pool, slots, None), pool[:2])  # mat None: the plain gather


# ---- 5. loaders -----------------------------------------------------------------------------------------------------------------------------------
def _write_pair(tmp_path, tag, shape_ijk, affine, seed):
    """An image (HU-like values, positive inside a box, air outside) and a mask of blocks 0 .. 2 on the same grid (the helper of
    tests/test_segmentation_gpu.py)."""
    from headct_foundation_amd.nifti import write_nifti
    gen = np.random.default_rng(seed)
    ni, nj, nk = shape_ijk
    img = np.full((nk, nj, ni), -1000.0, np.float32)
    img[2:nk - 2, 3:nj - 2, 2:ni - 3] = gen.uniform(20.0, 80.0, (nk - 4, nj - 5, ni - 5)).astype(np.float32)
    mask = np.zeros((nk, nj, ni), np.int16)
    mask[3:nk // 2, 4:nj - 4, 3:ni // 2] = 1
    mask[nk // 2:nk - 3, 5:nj // 2, ni // 2:ni - 4] = 2
    ip, sp = tmp_path / f"{tag}.nii.gz", tmp_path / f"{tag}_seg.nii.gz"
    write_nifti(ip, img, affine, dtype="f4")
    write_nifti(sp, mask, affine, dtype="i2")
    return str(ip), str(sp)


AFF_B = np.array([[0.0, 1.5, 0.0, -10.0], [-0.8, 0.0, 0.0, 12.0], [0.0, 0.0, 2.0, 5.0], [0.0, 0.0, 0.0, 1.0]])  # not RAS, anisotropic


def _pairs_csv(tmp_path, n, missing=False):
    rows = [_write_pair(tmp_path, f"s{k}", (20, 18, 14) if k % 2 else (24, 14, 10), np.eye(4) if k % 2 else AFF_B, k) for k in range(n)]
    if missing:
        rows.append((f"{tmp_path}/missing.nii.gz", f"{tmp_path}/missing_seg.nii.gz"))
    csv = tmp_path / "pairs.csv"
    csv.write_text("img_path,seg_path\n" + "".join(f"{i},{s}\n" for i, s in rows))
    return str(csv)


@pytest.mark.parametrize("outside", [0, 255])
def test_loader_with_the_affine(lib, cuda, tmp_path, outside, capsys):
    """SegmentedVolumes with a RandAffine3D at prob 1: volumes are affine_augment of the cache items and labels affine_labels of the
    label items under last_mat / last_fire / last_flip; the scan that fails to load stays zero / all-255 and does not fire."""
    roi = (16, 16, 16)
    pairs = read_segmentation_paths(_pairs_csv(tmp_path, 3, missing=True))
    vc, lc = VolumeCache(tmp_path / "cache", roi, 3), LabelCache(tmp_path / "cache", roi, 3)
    aug = DeviceAugment(flip_prob=0.5, shift_offsets=0.1, shift_prob=0.5, seed=3, affine=RandAffine3D(20.0, 0.15, 0.1, 1.0, seed=5))
    order = [1, 3, 0, 2, 2, 3, 1, 0]
    loader = SegmentedVolumes(pairs, order, vc, lc, 4, cuda, aug, 2, affine_outside=outside)
    seen = 0
    for k, (vol, lab, names) in enumerate(loader):
        idxs = order[4 * k:4 * k + 4]
        flip, mat, fire = loader.last_flip, loader.last_mat, loader.last_fire
        shift = aug.last_draw[1]
        failed = [i == 3 for i in idxs]
        assert names == ["None" if f else pairs[i][0] for i, f in zip(idxs, failed)]
        assert fire.tolist() == [0 if f else 1 for f in failed] and bool(aug.affine.last_draw["fire"].all())
        assert torch.equal(mat, aug.affine.matrices(aug.affine.last_draw, flip)) and torch.equal(flip, aug.last_draw[0])
        x = torch.stack([torch.zeros((3,) + roi, dtype=torch.float16, device=cuda) if f else vc.get(pairs[i][0], cuda) for i, f in zip(idxs, failed)])
        y = torch.stack([torch.full(roi, 255, dtype=torch.uint8, device=cuda) if f else lc.get(*pairs[i], cuda) for i, f in zip(idxs, failed)])
        assert torch.equal(vol, affine_augment(x, mat, fire, flip, shift))
        assert torch.equal(lab, affine_labels(y, torch.arange(4, dtype=torch.int32), mat, fire, flip, outside))
        # and the labels against the float64 reference, under the same judgement as the kernel's own cases
        case = dict(name=f"loader batch {k}", kind="general", S=16, pool=y.cpu().numpy(), slots=[0, 1, 2, 3], mat=mat, fire=fire.numpy(), flip=flip.numpy(),
                    outside=outside)
        ok, what = C.verify(case, lab.cpu().numpy())
        assert ok, what
        for b, f in enumerate(failed):
            if f:
                assert bool((lab[b] == 255).all()) and bool((vol[b] == shift[b].to(cuda)).all())
            else:
                assert not torch.equal(lab[b], y[b]) and set(lab[b].unique().tolist()) <= {0, 1, 2, outside}
                seen += int((lab[b] == outside).sum()) if outside == 255 else 0
    assert outside == 0 or seen > 0  # part of some volume was pushed out and reads as ignore
    capsys.readouterr()


def _seg_config(tmp_path, csv, **seg):
    from config import _C
    cfg = _C.clone()
    cfg.defrost()
    cfg.DATA.SYNTHETIC, cfg.DATA.BATCH_SIZE, cfg.DATA.CACHE_DIR, cfg.DATA.NUM_WORKERS = False, 2, str(tmp_path / "cache"), 2
    cfg.MODEL.ROI, cfg.MODEL.IN_CHANS, cfg.VIT.INPUT_SIZE, cfg.VIT.IN_CHANS = [16, 16, 16], 3, 16, 3
    cfg.DATA.TRAIN_CSV_PATH = cfg.DATA.VAL_CSV_PATH = cfg.DATA.TEST_CSV_PATH = csv
    cfg.TRAIN.AFFINE_ROTATE, cfg.TRAIN.AFFINE_SCALE = [30.0], 0.2
    for k, v in seg.items():
        setattr(cfg.SEG, k, v)
    return cfg


def _two_epochs(loader):
    out = [[(v, y, names) for v, y, names in loader] for _ in range(2)]
    torch.cuda.synchronize()
    return [(v.cpu(), y.cpu(), names) for epoch in out for v, y, names in epoch]


def test_switch_off_is_the_loader_without_the_feature(lib, cuda, tmp_path):
    csv = _pairs_csv(tmp_path, 4)
    cfg = _seg_config(tmp_path, csv)
    off = get_segmentation_dataloaders(cfg, cuda, 0, 1)
    assert off[0].augment.affine is None and off[1].augment is None and off[2].augment is None
    got = _two_epochs(off[0])
    assert off[0].last_mat is None and off[0].last_fire is None and off[0].last_flip is not None
    # a loader built as before this switch existed, same seed
    pairs = read_segmentation_paths(csv)
    vc, lc = VolumeCache(cfg.DATA.CACHE_DIR, [16, 16, 16], 3), LabelCache(cfg.DATA.CACHE_DIR, [16, 16, 16], 3)
    bare = SegmentedVolumes(pairs, off[0].order, vc, lc, 2, cuda, DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=cfg.SEED), 2)
    want = _two_epochs(bare)
    assert len(got) == len(want) == 4
    for (v, y, names), (w, z, others) in zip(got, want):
        assert torch.equal(v.view(torch.int32), w.view(torch.int32)) and torch.equal(y, z) and names == others
    # switch on: the train loader alone carries the affine, seeded SEED + rank; the same scans in the same order, moved
    on = get_segmentation_dataloaders(_seg_config(tmp_path, csv, AFFINE_PROB=1.0, AFFINE_OUTSIDE="ignore"), cuda, 0, 1)
    aff = on[0].augment.affine
    assert isinstance(aff, RandAffine3D) and (aff.rotate_deg, aff.scale, aff.prob) == ((30.0,) * 3, 0.2, 1.0) and aff.gen.initial_seed() == cfg.SEED
    assert on[0].affine_outside == 255 and on[1].augment is None and on[2].augment is None
    for (v, y, names), (w, z, others) in zip(_two_epochs(on[0]), want):
        assert names == others and not torch.equal(v, w) and not torch.equal(y, z) and bool((y == 255).any())
    for k in (1, 2):
        for (v, y, names), (w, z, others) in zip(_two_epochs(on[k]), _two_epochs(off[k])):
            assert torch.equal(v, w) and torch.equal(y, z) and names == others
    bad = _seg_config(tmp_path, csv)
    bad.TRAIN.AFFINE_PROB = 0.5
    with pytest.raises(ValueError, match="SEG.AFFINE_PROB"):
        get_segmentation_dataloaders(bad, cuda, 0, 1)


# ---- 6. training ----------------------------------------------------------------------------------------------------------------------------------
def test_training_under_the_affine_beats_the_constant_prediction(lib, cuda):
    """tests/test_segmentation_gpu.py's test of 30 steps on one fixed synthetic batch, with the batch resampled anew at every step
    (the wrapper at prob 1, ignore outside): the same step count, optimizers and bar -- the loss ends below its first value and below
    the loss of the best constant prediction on the batch's labels."""
    from headct_foundation_amd.dino_model import ViTBackbone
    from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_
    from headct_foundation_amd.segmentation import SegmentationHead, seg_loss
    torch.manual_seed(7)
    K, P, S = 3, 12, 24
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=1,
                      compute_dtype="fp32").to(cuda)
    head = SegmentationHead(48, P, K).to(cuda)
    first = 1 + vit.num_register_tokens
    fixed = SyntheticSegmented(1, 8, 3, S, K, cuda, seed=0)
    y0 = fixed.batches[0][1].clone()
    const = seg_ref.constant_prediction(y0.cpu(), K)
    loader = AugmentedSegmented(fixed, DeviceAugment(flip_prob=0.0, shift_offsets=0.0, shift_prob=0.0, affine=RandAffine3D(prob=1.0, seed=1)), 255)
    opts = [HipAdamW(head, lr=1e-2, weight_decay=0.0), HipAdamW(vit, lr=1e-4, weight_decay=0.0)]
    losses = []
    vit.train()
    head.train()
    for _ in range(30):
        (v, y, _), = list(loader)
        assert bool(loader.last_draws["fire"].all()) and not torch.equal(y, y0)
        for o in opts:
            o.zero_grad()
        loss = seg_loss(head(vit(v)[0]), y, P, K, first, inplace_grad=True)
        loss.backward()
        clip_grad_norm_(head, 1.0)
        clip_grad_norm_(vit, 1.0)
        for o in opts:
            o.step()
        losses.append(float(loss.detach()))
    assert torch.equal(fixed.batches[0][1], y0)  # the fixed batch is not written
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f}, constant prediction {const['loss']:.4f}")
    assert all(math.isfinite(x) for x in losses)
    assert losses[-1] < losses[0] and losses[-1] < const["loss"], (losses, const)


# ---- 7. main_segmentation.py end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["nifti", "synthetic"])
def test_main_segmentation_with_the_affine(lib, cuda, tmp_path, data):
    from headct_foundation_amd.dino_model import ViTBackbone
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=0, compute_dtype="fp32")
    torch.save({"state_dict": {"module." + k: t for k, t in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    opts = ["VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3",
            "MODEL.ROI", "[24, 24, 24]", "TRAIN.VAL_EVERY", "1", "MODEL.DIR", str(tmp_path / "out"), "MODEL.SAVE_NAME", "seg.pt", "LOG.OUTPUT_DIR",
            str(tmp_path / "log"), "PREDS_SAVE_NAME", "run", "MAE.COMPUTE_DTYPE", "fp32", "DATA.CACHE_DIR", str(tmp_path / "cache"), "DATA.NUM_WORKERS", "2"]
    extra = []
    if data == "nifti":
        csv = _pairs_csv(tmp_path, 4)
        extra = ["--train_csv_path", csv, "--val_csv_path", csv, "--test_csv_path", csv]
    else:
        opts += ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "8"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", "29631" if data == "nifti" else "29633",
           os.path.join(ROOT, "main_segmentation.py"), "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"),
           "--seg_classes", "3", "--batch_size", "2", "--max_epochs", "1", "--grad_clip", "1.0", "--base_lr", "1e-4", "--seg_affine_prob", "0.5",
           "--affine_rotate", "10", "--seg_affine_outside", "ignore"] + extra + ["--opts"] + opts
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "Random affine of scans and masks: SEG.AFFINE_PROB 0.5, SEG.AFFINE_OUTSIDE ignore, TRAIN.AFFINE_ROTATE [10.0] degrees" in log, log[-4000:]
    # training steps log "Loss: x  CE: ..", the validation and test passes "Loss: x" alone: every one of them finite
    train = [float(x) for x in re.findall(r"Epoch 1/1 \[\d+/\d+\]  Loss: (\S+)  CE:", log)]
    losses = [float(x) for x in re.findall(r"Epoch \d+/1 \[\d+/\d+\]  Loss: (\S+)", log)]
    assert len(train) == (2 if data == "nifti" else 4) and len(losses) > len(train) and all(math.isfinite(x) for x in losses), log[-4000:]
    assert "SegDiceGlobal" in log and "Final test loss" in log and "Error loading" not in log, log[-4000:]
