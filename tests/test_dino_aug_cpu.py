"""Host side of the DINO multi-crop augmentation (no GPU): the draws of DeviceAugmentDINO3D, the restatement's own area windows,
the new config keys and the exported symbols."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import dino_aug_ref as R


def _aug(**kw):
    from headct_foundation_amd.data import DeviceAugmentDINO3D
    args = dict(final_size=(96, 96, 96), global_crops_size=112, local_crops_size=64, local_crops_number=8, seed=0)
    args.update(kw)
    return DeviceAugmentDINO3D(**args)


def test_draw_ranges_rates_and_independence():
    """A few thousand draws (S = 96: the volume sits at [64, 160) of the 224^3 field, the local field is [16, 208) of it)."""
    aug = _aug(seed=1)
    B, N = 64, 8
    draws = [aug.draw(B, 96) for _ in range(N)]
    boxes = torch.cat([d["boxes"] for d in draws], dim=1).long()  # [V, N B, 6]
    assert boxes.shape == (10, N * B, 6) and draws[0]["boxes"].dtype == torch.int32
    gs, gn = boxes[:2, :, :3] + 64, boxes[:2, :, 3:]       # global views in field coordinates: input + pad
    ls, ln = boxes[2:, :, :3] + 64 - 16, boxes[2:, :, 3:]  # local views in coordinates of the 192 field
    assert int(gn.min()) == 112 and int(gn.max()) == 224  # both extremes occur
    assert bool((gs >= 0).all()) and bool((gs + gn <= 224).all())
    assert int(gs.min()) == 0 and bool((gs + gn == 224).any())
    assert int(ln.min()) == 64 and int(ln.max()) == 112
    assert bool((ls >= 0).all()) and bool((ls + ln <= 192).all())
    assert int(ls.min()) == 0 and bool((ls + ln == 192).any())
    # axes are drawn independently: some box has three different sizes, and sizes of two axes are uncorrelated
    assert bool(((gn[..., 0] != gn[..., 1]) & (gn[..., 1] != gn[..., 2]) & (gn[..., 0] != gn[..., 2])).any())
    assert abs(float(torch.corrcoef(torch.stack([gn[..., 0].flatten().double(), gn[..., 1].flatten().double()]))[0, 1])) < 0.1
    flip = torch.cat([d["flip"] for d in draws], dim=1)
    shift = torch.cat([d["shift"] for d in draws], dim=1)
    assert flip.dtype == torch.uint8 and shift.dtype == torch.float32
    assert int(flip[2:].max()) == 0 and float(shift[2:].abs().max()) == 0.0  # local views carry no flip / shift
    assert int(flip.max()) <= 7 and float(shift.abs().max()) <= 0.2 and float(shift.abs().max()) > 0.19

    def within(count, n, p):
        return abs(count - n * p) <= 4 * math.sqrt(n * p * (1 - p))

    n2 = 2 * N * B
    for a in range(3):
        assert within(int(((flip[:2] >> a) & 1).sum()), n2, 0.2), a
    assert within(int((shift[:2] != 0).sum()), n2, 0.5)
    # more draws for the per-sample transforms
    more = [aug.draw(B, 96) for _ in range(24)]
    sf = torch.cat([d["smooth_fire"] for d in more])
    gf = torch.cat([d["gamma_fire"] for d in more])
    assert within(int(sf.sum()), sf.numel(), 0.2) and within(int(gf.sum()), gf.numel(), 0.2)
    assert abs(int((sf & gf).sum()) - sf.numel() * 0.04) <= 4 * math.sqrt(sf.numel() * 0.04)  # the two fire independently
    sigma = torch.cat([d["sigma"] for d in more])
    gamma = torch.cat([d["gamma"] for d in more])
    assert sigma.shape == (24 * B, 3) and 0.5 <= float(sigma.min()) < 0.51 and 0.99 < float(sigma.max()) <= 1.0
    assert gamma.shape == (24 * B,) and 0.2 <= float(gamma.min()) < 0.21 and 0.99 < float(gamma.max()) <= 1.0


def test_draw_is_seeded():
    a, b, c = _aug(seed=5).draw(4, 96), _aug(seed=5).draw(4, 96), _aug(seed=6).draw(4, 96)
    assert sorted(a) == ["boxes", "flip", "gamma", "gamma_fire", "shift", "sigma", "smooth_fire"]
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["boxes"], c["boxes"])


@pytest.mark.parametrize("S,pad", [(96, 64), (224, 0), (240, -8), (97, 63), (225, 0)])
def test_draw_input_coordinates_are_field_coordinates_minus_the_pad(S, pad):
    """Field voxel p is input voxel p - pad: pad = (224 - S) // 2 of zero padding in front for S <= 224, and for S > 224 the centre
    crop starts at input voxel S // 2 - 112 (pad negative).  Checked by cutting the same boxes from the materialised field."""
    aug = _aug(seed=2, local_crops_number=2)
    assert aug.origins(S) == (-pad, -pad + 16)
    d = aug.draw(3, S)
    vol = torch.arange(S ** 3, dtype=torch.float32).reshape(1, S, S, S) + 1.0  # every voxel its own non-zero value
    gfield = R.pad_or_crop(vol, 224)
    lfield = R.center_crop(gfield, 192)
    big = F.pad(vol, (300,) * 6)  # input coordinates + 300, zero outside
    for v in range(4):
        field = gfield if v < 2 else lfield
        for b in range(3):
            x, y, z, nx, ny, nz = [int(t) for t in d["boxes"][v, b]]
            fx, fy, fz = (t + pad - (0 if v < 2 else 16) for t in (x, y, z))
            assert 0 <= min(fx, fy, fz) and max(fx + nx, fy + ny, fz + nz) <= field.shape[-1]
            assert torch.equal(field[:, fx:fx + nx, fy:fy + ny, fz:fz + nz],
                               big[:, x + 300:x + 300 + nx, y + 300:y + 300 + ny, z + 300:z + 300 + nz])


def test_constructor_follows_the_reference_and_rejects_non_cubic():
    from headct_foundation_amd.data import DeviceAugmentDINO3D, MultiCropLoader
    aug = DeviceAugmentDINO3D([96, 96, 96], [112, 112, 112], [64, 64, 64], 8)  # the yaml's lists, the reference's argument order
    assert (aug.final_size, aug.global_crops_size, aug.local_crops_size, aug.n_views, aug.field, aug.local_field) == (96, 112, 64, 10, 224, 192)
    with pytest.raises(NotImplementedError):
        DeviceAugmentDINO3D((96, 96, 64), 112, 64, 8)
    with pytest.raises(NotImplementedError):
        DeviceAugmentDINO3D(98, 112, 64, 8)
    with pytest.raises(ValueError):
        DeviceAugmentDINO3D(96, 112, 64, 8, field=100)
    from headct_foundation_amd._lib import HctError
    with pytest.raises(HctError):
        aug(torch.zeros(1, 1, 8, 8, 8))  # CPU tensors: no fallback
    assert len(MultiCropLoader([0, 1, 2], aug)) == 3


def test_area_windows_agree_with_interpolate():
    """The window bounds [floor(i n / F), ceil((i + 1) n / F)) written out as per-axis averaging matrices are what
    F.interpolate(mode="area") computes: 3 x 96^3 fp16 data in the padded field, boxes of 64 ... 224 resized to 96."""
    g = torch.Generator().manual_seed(0)
    vol = torch.rand(3, 96, 96, 96, generator=g).to(torch.float16)
    field = R.pad_or_crop(vol.float(), 224)
    worst, taps = 0.0, 0
    for box in ((0, 0, 0, 224, 224, 224), (40, 50, 60, 64, 64, 64), (30, 64, 10, 112, 96, 171), (60, 20, 50, 97, 150, 64)):
        x, y, z, nx, ny, nz = box
        got = R.crop_resize(vol, box, 96)
        mats = [R.area_matrix(n, 96) for n in (nx, ny, nz)]
        taps = max(taps, max(int((m > 0).sum(1).max()) for m in mats))
        crop = field[:, x:x + nx, y:y + ny, z:z + nz].double()
        want = torch.einsum("kc,dijc->dijk", mats[2], torch.einsum("jb,dibc->dijc", mats[1], torch.einsum("ia,dabc->dibc", mats[0], crop)))
        worst = max(worst, float((got.double() - want).abs().max()))
        for n in (nx, ny, nz):
            assert R.area_windows(n, 96, 0) == [(int(torch.nonzero(r)[0]), int(torch.nonzero(r)[-1]) + 1) for r in R.area_matrix(n, 96)]
    print(f"area resize vs averaging matrices: max abs {worst:.3g}, at most {taps} taps per axis")
    assert worst <= 2e-6 and taps <= 4


def test_contrast_restatement_constant_crop_and_identity():
    c = torch.full((3, 4, 4, 4), 0.37)
    assert torch.equal(R.adjust_contrast(c, 0.5), c)  # range 0: the formula returns the constant
    x = torch.rand(3, 4, 4, 4, generator=torch.Generator().manual_seed(1)) * 1.4 - 0.2
    assert float((R.adjust_contrast(x, 1.0) - x).abs().max()) <= 2e-7
    assert float((R.adjust_contrast_fp32(x, 0.37) - R.adjust_contrast(x, 0.37)).abs().max()) <= 2e-6


def test_config_keys_and_exports(lib):
    from config import _C
    from headct_foundation_amd import _lib
    assert _C.DATA.DEVICE_AUGMENT is False and _C.DINO.CROP_FIELD == 224 and _C.DINO.LOCAL_CROP_FIELD == 192
    names = _lib.exported_symbols()
    for s in ("hct_crop_resize_area", "hct_adjust_contrast", "hct_adjust_contrast_workspace_bytes"):
        assert s in names and hasattr(lib, s)
    n = 3 * 96 ** 3
    assert lib.hct_adjust_contrast_workspace_bytes(64, n) >= 64 * 2 * 4 and lib.hct_adjust_contrast_workspace_bytes(0, n) == 0


def test_entry_point_refuses_roi_other_than_the_backbone_size():
    import main_pretrain_dino as M
    from config import _C
    cfg = _C.clone()
    cfg.defrost()
    cfg.DATA.DEVICE_AUGMENT, cfg.DATA.SYNTHETIC = True, True
    cfg.MODEL.ROI = [64, 64, 64]
    with pytest.raises(ValueError, match="VIT.INPUT_SIZE"):
        M.build_loaders(cfg, torch.device("cpu"), 0, 1)
