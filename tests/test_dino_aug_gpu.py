"""GPU: the DINO multi-crop augmentation on the device (hct_crop_resize_area, hct_adjust_contrast, DeviceAugmentDINO3D,
MultiCropLoader, main_pretrain_dino.py with DATA.DEVICE_AUGMENT) against the CPU restatement tests/dino_aug_ref.py, which cuts
its boxes from a really materialised zero-padded field.  Bound everywhere: abs <= 2e-6, the bound of the project's other fp32
resampling kernels (sums of <= 64 values in [0, 1] in another order, one divide, one add)."""
import os

import pytest
import torch

from tests import dino_aug_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-6
S0, FIELD, LFIELD, FINAL = 96, 224, 192, 96
PAD = (FIELD - S0) // 2  # 64: field voxel p is input voxel p - PAD

# boxes in coordinates of the 224^3 field; the volume is [64, 160) of it
CASES = {
    "whole field": (0, 0, 0, 224, 224, 224),
    "inside": (66, 70, 75, 80, 72, 85),
    "one face": (30, 70, 70, 80, 70, 70),
    "two faces": (30, 120, 70, 80, 80, 70),
    "three faces": (20, 100, 130, 112, 120, 90),
    "up-sampling": (80, 90, 70, 64, 64, 64),
    "copy": (64, 64, 64, 96, 96, 96),
    "anisotropic": (10, 40, 0, 200, 150, 224),
}
IN_PADDING = (0, 0, 0, 60, 60, 60)


def _resample(lib, x, boxes, F, flip=None, shift=None):
    """hct_crop_resize_area on x [B, C, S, S, S] (device) with CPU tables boxes [V, B, 6] (input coordinates), flip / shift [V, B]."""
    from headct_foundation_amd import _lib
    V, B = boxes.shape[0], boxes.shape[1]
    dev = x.device
    bx = boxes.to(torch.int32).contiguous().to(dev)
    fl = None if flip is None else flip.to(torch.uint8).contiguous().to(dev)
    sh = None if shift is None else shift.to(torch.float32).contiguous().to(dev)
    out = torch.empty(V, B, x.shape[1], F, F, F, dtype=torch.float32, device=dev)
    _lib.check(lib.hct_crop_resize_area(x.data_ptr(), _lib.dtype_code(x), B, x.shape[1], x.shape[2], out.data_ptr(), F, V, bx.data_ptr(),
                                        _lib.ptr(fl), _lib.ptr(sh), _lib.stream_ptr()), "hct_crop_resize_area")
    torch.cuda.synchronize()
    return out.cpu()


def _volumes(B, C, S, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, C, S, S, S, generator=g).to(dtype)


def _compare(got, want, what):
    nz = float((want != 0).float().mean())
    err = float((got - want).abs().max())
    print(f"{what}: max abs err {err:.3g}, non-zero outputs {100 * nz:.1f} %")
    assert nz > 0.05, (what, nz)  # zeros must not carry the comparison
    assert err <= TOL, (what, err)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_resample_explicit_boxes_vs_restatement(lib, cuda, dtype):
    """Full geometry (S 96 in the 224 field, F 96, C 3, B 2): the whole field, a box inside the volume, boxes straddling one, two
    and three faces, a 64-wide box (up-sampling), size == F (a pure copy: bit-equal), anisotropic sizes, and one box wholly in the
    padding (exactly zero).  Sample 1 takes the cases in another order than sample 0."""
    x = _volumes(2, 3, S0, dtype, 11)
    names = list(CASES)
    per_sample = [names, names[3:] + names[:3]]
    field_boxes = [[CASES[per_sample[b][v]] for b in range(2)] for v in range(len(names))] + [[IN_PADDING, IN_PADDING]]
    boxes = torch.tensor(field_boxes)
    boxes[..., :3] -= PAD
    got = _resample(lib, x.to(cuda), boxes, FINAL)
    again = _resample(lib, x.to(cuda), boxes, FINAL)
    assert torch.equal(got, again)  # fixed summation order: two calls are bit-identical
    for v in range(len(names)):
        for b in range(2):
            want = R.crop_resize(x[b], field_boxes[v][b], FINAL, FIELD)
            _compare(got[v, b], want, f"{dtype} {per_sample[b][v]} (sample {b})")
            if per_sample[b][v] == "copy":
                assert torch.equal(got[v, b], x[b].float())
    assert float(got[-1].abs().max()) == 0.0


@pytest.mark.parametrize("S,offset", [(240, 8), (224, 0)])
def test_resample_larger_volumes(lib, cuda, S, offset):
    """S = 240: the field is a centre crop, input coordinates = field coordinates + 8; S = 224: no padding at all."""
    x = _volumes(1, 3, S, torch.float16, 12)
    field_boxes = [[CASES["whole field"]], [CASES["anisotropic"]], [CASES["three faces"]]]
    boxes = torch.tensor(field_boxes)
    boxes[..., :3] += offset
    got = _resample(lib, x.to(cuda), boxes, FINAL)
    for v in range(3):
        _compare(got[v, 0], R.crop_resize(x[0], field_boxes[v][0], FINAL, FIELD), f"S {S} box {field_boxes[v][0]}")


def test_resample_flips_and_shift(lib, cuda):
    """All 8 flip codes: equal to torch.flip of the unflipped result bit for bit (the window sums keep their order).  The shift is
    one fp32 add after the divide, in the same place as the restatement's: bit-equal to the unshifted result plus the offset."""
    x = _volumes(2, 3, S0, torch.float16, 13)
    fb = [CASES["three faces"], CASES["anisotropic"]]
    boxes = torch.tensor([fb] * 8)
    boxes[..., :3] -= PAD
    flip = torch.arange(8, dtype=torch.uint8).view(8, 1).repeat(1, 2)
    shift = torch.tensor([[0.0, 0.0], [0.2, -0.2], [0.1337, -0.0421], [0.0, 0.05], [-0.11, 0.0], [0.07, 0.07], [-0.2, 0.2], [0.01, -0.19]])
    plain = _resample(lib, x.to(cuda), boxes, FINAL)
    flipped = _resample(lib, x.to(cuda), boxes, FINAL, flip=flip)
    both = _resample(lib, x.to(cuda), boxes, FINAL, flip=flip, shift=shift)
    for code in range(8):
        dims = [1 + a for a in range(3) if code & (1 << a)]  # spatial axis a of a crop [C, F, F, F]
        for b in range(2):
            want = torch.flip(plain[0, b], dims) if dims else plain[0, b]
            assert torch.equal(flipped[code, b], want), (code, b)
            assert torch.equal(both[code, b], want + shift[code, b]), (code, b)
            _compare(both[code, b], R.crop_resize(x[b], fb[b], FINAL, FIELD, None, code, float(shift[code, b])), f"flip {code} shift {float(shift[code, b]):+.4f}")


def test_adjust_contrast_vs_fp64_formula(lib, cuda):
    """gammas 0.2, 0.37, 1.0; a sample that does not fire (bit-identical); a crop with negative values (after a shift); a constant
    crop (range 0: the formula returns the constant, no NaN).  abs <= 2e-6 against the formula evaluated in fp64 (values in
    [-0.2, 1.2]: fp32 spacing 1.2e-7, five roundings and a powf of at most 2 ulp); the fp32 CPU formula's own distance is printed."""
    from headct_foundation_amd import _lib
    C, F = 3, 32
    n = C * F ** 3
    g = torch.Generator().manual_seed(21)
    x = torch.rand(6, C, F, F, F, generator=g)
    x[4] = x[4] * 1.2 - 0.2  # negative values
    x[5] = 0.4321            # constant
    gamma = torch.tensor([0.2, 0.37, 1.0, 0.5, 0.61, 0.3])
    apply = torch.tensor([1, 1, 1, 0, 1, 1], dtype=torch.uint8)
    d = x.to(cuda)
    need = lib.hct_adjust_contrast_workspace_bytes(6, n)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    gd, ad = gamma.to(cuda), apply.to(cuda)
    _lib.check(lib.hct_adjust_contrast(d.data_ptr(), 6, n, gd.data_ptr(), ad.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), "hct_adjust_contrast")
    torch.cuda.synchronize()
    got = d.cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got[3], x[3])
    assert torch.equal(got[5], x[5])
    for b in (0, 1, 2, 4, 5):
        want = R.adjust_contrast(x[b], float(gamma[b]))
        err, cpu32 = float((got[b] - want).abs().max()), float((R.adjust_contrast_fp32(x[b], float(gamma[b])) - want).abs().max())
        print(f"contrast sample {b} gamma {float(gamma[b]):.2f}: kernel err {err:.3g}, fp32 CPU formula err {cpu32:.3g}")
        assert err <= TOL, (b, err)
    with pytest.raises(_lib.HctError):
        _lib.check(lib.hct_adjust_contrast(d.data_ptr(), 6, n, gd.data_ptr(), ad.data_ptr(), ws.data_ptr(), need - 1, _lib.stream_ptr()), "hct_adjust_contrast")


def _field_boxes(aug, d, S):
    """The draw's boxes back in field coordinates, by the test's own arithmetic (S <= field here): global views + pad, local
    views + pad - (field - local_field) / 2."""
    pad = (aug.field - S) // 2
    fb = d["boxes"].clone().long()
    fb[:2, :, :3] += pad
    fb[2:, :, :3] += pad - (aug.field // 2 - aug.local_field // 2)
    return fb.tolist()


def test_device_augment_end_to_end(lib, cuda):
    """DeviceAugmentDINO3D with its own draws against the restatement chain on `last_draw`, 2e-6 per view.  View 1 in two stages:
    t ** gamma has slope gamma t ** (gamma - 1), unbounded towards t = 0, so a 2e-7 difference in the resampled crop may exceed
    2e-6 after the contrast step.  Stage one: the same draw with gamma_fire cleared against the restatement; stage two: the
    reference contrast applied to the DEVICE's pre-contrast crop against the device's result."""
    from headct_foundation_amd.data import DeviceAugmentDINO3D
    from headct_foundation_amd.dino_model import ViTBackbone
    B, C, L = 4, 3, 3
    aug = DeviceAugmentDINO3D((FINAL,) * 3, 112, 64, L, seed=3)
    x = _volumes(B, C, S0, torch.float16, 31)
    views = aug(x.to(cuda))
    d = aug.last_draw
    assert 0 < int(d["smooth_fire"].sum()) < B and 0 < int(d["gamma_fire"].sum()) < B, (d["smooth_fire"], d["gamma_fire"])
    assert len(views) == 2 + L
    for v in views:
        assert tuple(v.shape) == (B, C, FINAL, FINAL, FINAL) and v.dtype == torch.float32 and v.is_contiguous()
    assert views[2].data_ptr() - views[1].data_ptr() == views[1].numel() * 4  # views of one [V, B, C, F, F, F] buffer
    fb = _field_boxes(aug, d, S0)
    no_gamma = dict(d, gamma_fire=torch.zeros(B, dtype=torch.bool))
    pre = aug(x.to(cuda), draw=no_gamma)
    assert aug.last_draw is no_gamma
    torch.cuda.synchronize()
    want = R.views(x, fb, no_gamma, FINAL, FIELD, LFIELD)
    for v in range(2 + L):
        err = float((pre[v].cpu() - want[v]).abs().max())
        print(f"view {v}: max abs err {err:.3g}")
        assert err <= TOL, (v, err)
        if v != 1:
            assert torch.equal(views[v], pre[v])  # the same draw: the same crops
    pre1, got1 = pre[1].cpu(), views[1].cpu()
    for b in range(B):
        if bool(d["gamma_fire"][b]):
            err = float((got1[b] - R.adjust_contrast(pre1[b], float(d["gamma"][b]))).abs().max())
            print(f"view 1 sample {b} contrast on the device's crop: max abs err {err:.3g}")
            assert err <= TOL and not torch.equal(got1[b], pre1[b])
        else:
            assert torch.equal(got1[b], pre1[b])
    # the native backbone takes the list as it is: contiguous fp32 parts are read in place, bit-identical to the concatenation
    torch.manual_seed(3)
    bb = ViTBackbone(img_size=FINAL, patch_size=16, in_chans=C, hidden_size=192, mlp_dim=384, num_layers=2, num_heads=3,
                     num_register_tokens=2, compute_dtype="bf16").to(cuda)
    assert all(v.contiguous().float().data_ptr() == v.data_ptr() for v in views)
    with torch.no_grad():
        assert torch.equal(bb(views)[0], bb(torch.cat(views))[0])


def _check_constant_volumes(views, d, vals, S, F):
    """views: list of V CPU tensors [B, C, F, F, F] made from volumes that are vals[b] everywhere; d: the draw (input coordinates)."""
    for v, crops in enumerate(views):
        for b, val in enumerate(vals):
            box = [int(t) for t in d["boxes"][v, b]]
            sh = d["shift"][v, b]
            inside, outside = [], []
            for a in range(3):
                w = R.area_windows(box[3 + a], F, box[a], bool(int(d["flip"][v, b]) & (1 << a)))
                inside.append(torch.tensor([0 <= lo and hi <= S for lo, hi in w]))
                outside.append(torch.tensor([hi <= 0 or lo >= S for lo, hi in w]))
            m_in = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
            m_out = outside[0][:, None, None] | outside[1][None, :, None] | outside[2][None, None, :]
            c = crops[b]
            full = torch.tensor(val, dtype=torch.float32) + sh
            assert float((c[:, m_in] - full).abs().max() if m_in.any() else 0.0) <= TOL, (v, b)
            assert bool((c[:, m_out] == sh).all()), (v, b)
            # the counts are what the box predicts: nothing else of the crop shows the sample in full, nothing else is empty
            n_in = int(inside[0].sum()) * int(inside[1].sum()) * int(inside[2].sum())
            n_out = F ** 3 - int((~outside[0]).sum()) * int((~outside[1]).sum()) * int((~outside[2]).sum())
            assert int(m_in.sum()) == n_in and int(m_out.sum()) == n_out
            assert int(((c - full).abs() <= TOL).sum()) == n_in * c.shape[0], (v, b)
            assert int((c == sh).sum()) == n_out * c.shape[0], (v, b)


def test_views_of_a_sample_show_that_sample(lib, cuda):
    """What noise crops cannot have.  Volumes constant per sample (v_b, fp16-exact, different per sample), gamma and smoothing off:
    every output voxel of every view of sample b whose window lies wholly inside the volume is v_b (+ the view's shift), every
    voxel whose window lies wholly in the padding is exactly the shift, and the count of each kind is what the drawn box
    predicts (per axis, mirrored under a flip)."""
    from headct_foundation_amd.data import DeviceAugmentDINO3D
    B, C, L = 4, 3, 4
    vals = [0.25, 0.375, 0.5, 0.625]
    x = torch.tensor(vals, dtype=torch.float16).view(B, 1, 1, 1, 1).expand(B, C, S0, S0, S0).contiguous()
    aug = DeviceAugmentDINO3D(FINAL, 112, 64, L, seed=7)
    d = aug.draw(B, S0)
    d["smooth_fire"], d["gamma_fire"] = torch.zeros(B, dtype=torch.bool), torch.zeros(B, dtype=torch.bool)
    assert int((d["flip"] != 0).sum()) > 0 and int((d["shift"] != 0).sum()) > 0
    views = aug(x.to(cuda), draw=d)
    torch.cuda.synchronize()
    _check_constant_volumes([v.cpu() for v in views], d, vals, S0, FINAL)


def test_multi_crop_loader_feeds_the_engine_format(lib, cuda):
    from headct_foundation_amd.data import DeviceAugmentDINO3D, MultiCropLoader, SyntheticVolumes
    base = SyntheticVolumes(3, 2, 3, 24, cuda, seed=1, dtype=torch.float16)
    loader = MultiCropLoader(base, DeviceAugmentDINO3D([24] * 3, [28] * 3, [16] * 3, 2, seed=1, field=56, local_field=48))
    assert len(loader) == 3 and base.batches[0].dtype == torch.float16
    batches = list(loader)
    assert len(batches) == 3
    for crops in batches:
        assert len(crops) == 4 and all(tuple(c.shape) == (2, 3, 24, 24, 24) and c.dtype == torch.float32 and c.is_cuda for c in crops)
        assert all(bool(torch.isfinite(c).all()) for c in crops)
    assert not torch.equal(batches[0][0], batches[1][0])


def test_main_pretrain_dino_device_augment_run(cuda, tmp_path):
    """test_main_pretrain_dino_plumbing_run's command with DATA.DEVICE_AUGMENT True: crops cut on the device from fp16 volumes of
    24^3 (field 56, local field 48, global 28, local 16); completes, finite losses, checkpoint keys as before."""
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", "29541",
           os.path.join(root, "main_pretrain_dino.py"), "--local_rank", "0", "--model_name", "dino", "--batch_size", "2", "--max_epochs", "2",
           "--base_lr", "5e-4", "--cfg", os.path.join(root, "configs/dino/dino_tiny_plumbing.yaml"), "--optimizer", "AdamW", "--scheduler", "cosine",
           "--opts", "MODEL.DIR", str(tmp_path / "ckpt"), "LOG.OUTPUT_DIR", str(tmp_path / "log"), "OUTPUT", str(tmp_path / "json"),
           "DATA.DEVICE_AUGMENT", "True", "MODEL.ROI", "[24,24,24]", "DINO.CROP_FIELD", "56", "DINO.LOCAL_CROP_FIELD", "48",
           "DINO.GLOBAL_CROP_SIZE", "[28,28,28]", "DINO.LOCAL_CROP_SIZE", "[16,16,16]"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "train completed" in r.stdout and "test completed" in r.stdout
    assert "DEVICE_AUGMENT: true" in r.stdout.replace("True", "true")  # the dumped config: the flag reached the entry point
    finals = [float(m) for m in re.findall(r"best (?:train|test) dino loss: ([-+0-9.eE]+|nan|inf)", r.stdout)]
    assert len(finals) == 2 and all(f == f and abs(f) != float("inf") for f in finals), finals
    ck = torch.load(tmp_path / "ckpt" / "last_dino_tiny.pt", map_location="cpu", weights_only=True)
    assert sorted(ck.keys()) == ["best_loss", "epoch", "momentum_model_state_dict", "optimizer", "scheduler", "state_dict"]
    assert all(bool(torch.isfinite(t).all()) for t in ck["state_dict"].values() if t.is_floating_point())
    assert (tmp_path / "ckpt" / "best_dino_tiny.pt").exists()
