"""GPU: hct_seg_to_native (csrc/native.hip) through the C ABI against tests/native_ref.py (float64, fed the stored logits): outputs
in guarded buffers, logits as strided views inside NaN-filled allocations; then the host layer on real files and the entry point.
The bound on the blend's error is derived in tests/native_ref.py; none comes from the kernel's output."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib, native
from tests import native_ref as R
from tests import seg_ref
from tests.test_assembly_kernels_gpu import _code, _st
from tests.test_segmentation_gpu import _Bytes, _vit, _write_pair, _ws

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
P, G, S = R.P, R.G, R.S


def _logits(vol, first, pad, dtype, dev):
    """The volume in token layout as a strided view [T, N] (row stride N + pad) in the middle of a NaN-filled allocation."""
    tok = R.token_rows(vol, first, pad, dtype)
    T, ld = tok.shape
    guard = 4 * ld
    buf = torch.full((T * ld + 2 * guard,), float("nan"), dtype=dtype, device=dev)
    view = buf[guard:guard + T * ld].view(T, ld)
    view.copy_(tok)
    return view, buf


def _run(lib, dev, view, first, K, geom, interp="linear", labels=None, tabs=None, want_counts=True):
    """One hct_seg_to_native call -> (pred int16 [nk, nj, ni], class_voxels [K], counts [K, 3] or None), guards checked."""
    ni, nj, nk = geom.file_shape
    t = native.upload_tables(native.native_tables(geom, S, interp) if tabs is None else tabs, dev)
    pred, cv = _Bytes((nk, nj, ni), torch.int16, dev, 77), _Bytes((K,), torch.int64, dev, -5)
    cnt = _Bytes((K, 3), torch.int64, dev, -5) if labels is not None and want_counts else None
    lab_d = None if labels is None else torch.from_numpy(labels).to(dev)
    ws = _ws(lib.hct_seg_to_native_workspace_bytes(ni, nj, nk, K), dev)
    rc = lib.hct_seg_to_native(view.data_ptr(), _code(view.dtype), view.stride(0), view.shape[0], first, G, P, K, t["i0"].data_ptr(), t["i1"].data_ptr(),
                               t["w"].data_ptr(), t["inside"].data_ptr(), *geom.perm, ni, nj, nk, None if lab_d is None else lab_d.data_ptr(), pred.ptr,
                               cv.ptr, None if cnt is None else cnt.ptr, ws.data_ptr(), ws.numel(), _st())
    _lib.check(rc, "hct_seg_to_native")
    torch.cuda.synchronize()
    return pred.result().numpy(), cv.result().numpy(), None if cnt is None else cnt.result().numpy()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", R.CLASSES)
@pytest.mark.parametrize("name", list(R.dyadic_geometries()))
def test_integer_logits_are_exact(lib, cuda, name, K, dtype):
    """Small integers under dyadic weights: every blend is exact in fp32, so pred equals the reference voxel for voxel, the planted
    ties included, and the lowest class wins them."""
    geom = R.dyadic_geometries()[name]
    first = (0, 2)[K % 2]
    vol = R.integer_volume(K, K)
    view, _ = _logits(vol, first, 5, dtype, cuda)
    pred, cv, _ = _run(lib, cuda, view, first, K, geom)
    values, inside = R.blend(vol.numpy(), R.tables(geom), geom.perm)
    want = R.predict(values, inside)
    top = np.sort(values, axis=0)
    assert (top[-1] == top[-2])[inside].sum() >= 10  # exact ties of blended values are among the voxels
    assert np.array_equal(pred, want)
    assert np.array_equal(cv, np.bincount(pred.reshape(-1), minlength=K))


@pytest.mark.parametrize("interp", native.INTERPS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", R.CLASSES)
def test_identity_geometry_equals_seg_predict(lib, cuda, K, dtype, interp):
    """The identity geometry in both modes: the arg-max hct_seg_predict writes for the same logits (file axis i is item axis 0)."""
    first = (2, 0)[K % 2]
    vol = R.gaussian_volume(K, 40 + K, dtype == BF16)
    vol[:, 1, 2, :] = vol[0, 1, 2, :]  # a row of ties
    view, _ = _logits(vol, first, 8, dtype, cuda)
    pred, _, _ = _run(lib, cuda, view, first, K, R.identity_geom(), interp)
    ref = _Bytes((1, S, S, S), torch.uint8, cuda)
    _lib.check(lib.hct_seg_predict(view.data_ptr(), _code(dtype), view.stride(0), None, 1, view.shape[0], first, G, P, K, 0, ref.ptr, None, None,
                                   None, 0, _st()), "hct_seg_predict")
    torch.cuda.synchronize()
    want = ref.result()[0].numpy().astype(np.int16)
    assert np.array_equal(pred, want.transpose(2, 1, 0)) and (want[1, 2] == 0).all()


@pytest.mark.parametrize("case", R.gaussian_cases(), ids=[c[0] for c in R.gaussian_cases()])
def test_gaussian_logits_against_the_reference(lib, cuda, case):
    """Every geometry, fp32 and bf16: pred equals the float64 reference outside its near-ties (top-2 margin <= 2 E), whose share stays
    under the cap; class_voxels is bincount(pred), counts numpy's TP / FP / FN on labels with 255 planted; a second call is bit-equal."""
    name, geom, K, first, pad, bf16, seed = case
    dtype = BF16 if bf16 else F32
    vol = R.gaussian_volume(K, seed, bf16)
    view, _ = _logits(vol, first, pad, dtype, cuda)
    ni, nj, nk = geom.file_shape
    y = R.planted_labels((nk, nj, ni), K, seed)
    pred, cv, cnt = _run(lib, cuda, view, first, K, geom, labels=y)
    values, inside = R.blend(vol.numpy(), R.tables(geom), geom.perm)
    want = R.predict(values, inside)
    skip = R.near_ties(values, inside, float(vol.abs().max()))
    share = float(skip.mean())
    print(f"{name}: K {K} first {first} ld {view.stride(0)}: near-ties left out {int(skip.sum())} of {skip.size} ({share:.2e}), "
          f"differing inside them {int((pred != want)[skip].sum())}")
    assert share <= R.NEAR_TIE_CAP
    assert np.array_equal(pred[~skip], want[~skip])
    assert (pred[~inside] == 0).all() and 0 <= pred.min() and pred.max() < K
    assert np.array_equal(cv, np.bincount(pred.reshape(-1), minlength=K))
    assert np.array_equal(cnt, R.counts(pred, y, K))
    pred2, cv2, cnt2 = _run(lib, cuda, view, first, K, geom, labels=y)
    assert np.array_equal(pred, pred2) and np.array_equal(cv, cv2) and np.array_equal(cnt, cnt2)


def test_nearest_mode_on_a_general_geometry(lib, cuda):
    geom = R.geometries()["flip5"]
    vol = R.gaussian_volume(3, 9, False)
    view, _ = _logits(vol, 2, 3, F32, cuda)
    pred, _, _ = _run(lib, cuda, view, 2, 3, geom, "nearest")
    assert np.array_equal(pred, R.predict(*R.blend(vol.numpy(), R.tables(geom, S, "nearest"), geom.perm)))  # w = 0: no arithmetic, no near-tie


def test_argument_checks_launch_nothing(lib, cuda):
    """K 17, an axis of 1025, a null table and a too-small workspace: an error code each, and no output is touched."""
    K, first, geom = 3, 0, R.identity_geom()
    vol = R.gaussian_volume(K, 1, False)
    view, _ = _logits(vol, first, 3, F32, cuda)
    t = native.upload_tables(native.native_tables(geom, S), cuda)
    pred, cv = _Bytes((S, S, S), torch.int16, cuda, 77), _Bytes((K,), torch.int64, cuda, -5)
    ws = _ws(lib.hct_seg_to_native_workspace_bytes(S, S, S, K), cuda)

    def call(K_=K, ni=S, i0=t["i0"].data_ptr(), wsb=ws.numel(), perm=(0, 1, 2)):
        return lib.hct_seg_to_native(view.data_ptr(), _code(F32), view.stride(0), view.shape[0], first, G, P, K_, i0, t["i1"].data_ptr(),
                                     t["w"].data_ptr(), t["inside"].data_ptr(), *perm, ni, S, S, None, pred.ptr, cv.ptr, None, ws.data_ptr(), wsb, _st())

    for kw, word in ((dict(K_=17), "K 17"), (dict(ni=1025), "1024"), (dict(i0=None), "null table"), (dict(perm=(0, 1, 1)), "permutation")):
        rc = call(**kw)
        assert rc == -1 and word in lib.hct_last_error_string().decode(), (rc, lib.hct_last_error_string())
    assert call(wsb=8) == -3 and "workspace" in lib.hct_last_error_string().decode()
    # K * G * P above 8192: two item rows no longer fit the LDS a workgroup may ask for (refused before the logits are looked at)
    rc = lib.hct_seg_to_native(view.data_ptr(), _code(F32), 16 * 8, 300 ** 3, 0, 300, 2, 16, t["i0"].data_ptr(), t["i1"].data_ptr(), t["w"].data_ptr(),
                               t["inside"].data_ptr(), 0, 1, 2, S, S, S, None, pred.ptr, cv.ptr, None, ws.data_ptr(), ws.numel(), _st())
    assert rc == -1 and "8192" in lib.hct_last_error_string().decode()
    assert lib.hct_seg_to_native_workspace_bytes(S, S, S, 17) == 0 and lib.hct_seg_to_native_workspace_bytes(1025, S, S, K) == 0
    torch.cuda.synchronize()
    assert bool((pred.result() == 77).all()) and bool((cv.result() == -5).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((pred.result() != 77).all())


# ---- real files -------------------------------------------------------------------------------------------------------------------------
AFF_B = np.array([[0.0, 1.5, 0.0, -10.0], [-0.8, 0.0, 0.0, 12.0], [0.0, 0.0, 2.0, 5.0], [0.0, 0.0, 0.0, 1.0]])  # i -> -y, j -> +x: not RAS, anisotropic


def test_planted_box_through_the_label_loader(lib, cuda, tmp_path):
    """A box mask in file space -> load_label_volume (the nearest-neighbour label item) -> one-hot logits (x 10) -> seg_to_native in
    nearest mode: equal to the reference's prediction.  The Dice against the original box is printed, not thresholded: it is what
    the model-space metric hides."""
    from headct_foundation_amd.data import DecodedVolume, load_label_volume, run_loading_chain
    from headct_foundation_amd.nifti import write_nifti
    p, g = 4, 4
    roi = (p * g,) * 3
    ip, sp, _ = _write_pair(tmp_path, "box", (24, 14, 10), AFF_B, 5)
    mask = np.zeros((10, 14, 24), np.int16)
    mask[3:8, 4:11, 6:17] = 1
    write_nifti(sp, mask, AFF_B, dtype="i2")
    geom = native.scan_geometry(ip, roi, 3, cuda)
    dec = DecodedVolume(ip)
    assert geom.file_shape == tuple(dec.file_shape) and geom.perm == tuple(dec.perm) and geom.steps == tuple(dec.steps)
    with torch.cuda.device(cuda):
        _, box = run_loading_chain(dec, dec.host.to(cuda), roi, 3)
    assert native.confine_box(box.cpu().tolist(), dec.m) == (list(geom.start), list(geom.size))
    item = load_label_volume(sp, dec, box, roi, cuda).cpu()
    vol = 10.0 * torch.nn.functional.one_hot(item.to(torch.int64), 2).permute(3, 0, 1, 2).to(F64)
    tok = seg_ref.patchify(vol[None], 1, 1 + g ** 3, g, p)[0].to(F32).to(cuda)
    labels = native.read_native_labels(sp, geom, ip)
    assert np.array_equal(labels, mask.astype(np.uint8))
    out = native.seg_to_native(tok, p, 2, 1, geom, "nearest", labels=labels)
    pred = out["pred"].cpu().numpy()
    want = R.predict(*R.blend(vol.numpy(), R.tables(geom, p * g, "nearest"), geom.perm))
    assert np.array_equal(pred, want)
    cnt = out["counts"].cpu().numpy()
    assert np.array_equal(cnt, R.counts(pred, labels, 2)) and np.array_equal(out["class_voxels"].cpu().numpy(), np.bincount(pred.reshape(-1), minlength=2))
    tp, fp, fn = cnt[1]
    ml = native.class_volumes_ml(out["class_voxels"], geom.affine)
    print(f"planted box: Dice on the file grid {2 * tp / max(2 * tp + fp + fn, 1):.4f}; box {int(mask.sum())} voxels = {mask.sum() * 2.4 / 1000:.3f} mL, "
          f"predicted {ml[1]:.3f} mL")
    assert np.isclose(ml.sum(), mask.size * 1.5 * 0.8 * 2.0 / 1000.0)


def test_main_segmentation_native_preds_end_to_end(lib, cuda, tmp_path):
    """main_segmentation.py --native_preds on four tiny anisotropic, non-RAS NIfTI pairs: every <name>_native.nii.gz lies on its
    image's grid, every row of native_volumes.csv sums to the scan's volume, NativeDiceGlobal is reported; without the flag no
    such file appears."""
    from headct_foundation_amd.nifti import read_nifti
    vit = _vit("fp32", 0)
    torch.save({"state_dict": {"module." + k: t for k, t in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    shape = (24, 14, 10)
    pairs = [_write_pair(tmp_path, f"s{n}", shape, AFF_B, n)[:2] for n in range(4)]
    pairs_csv = tmp_path / "pairs.csv"
    pairs_csv.write_text("img_path,seg_path\n" + "".join(f"{i},{s}\n" for i, s in pairs))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")

    def run(tag, epochs, extra):
        opts = ["VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3",
                "MODEL.ROI", "[24, 24, 24]", "TRAIN.VAL_EVERY", "1", "MODEL.DIR", str(tmp_path / tag), "MODEL.SAVE_NAME", "seg.pt", "LOG.OUTPUT_DIR",
                str(tmp_path / (tag + "_log")), "PREDS_SAVE_NAME", "run", "MAE.COMPUTE_DTYPE", "fp32", "DATA.CACHE_DIR", str(tmp_path / "cache"),
                "DATA.NUM_WORKERS", "2"]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", "29619", os.path.join(ROOT, "main_segmentation.py"),
               "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"), "--seg_classes", "3", "--batch_size", "2",
               "--max_epochs", str(epochs), "--grad_clip", "1.0", "--base_lr", "1e-4", "--train_csv_path", str(pairs_csv), "--val_csv_path",
               str(pairs_csv), "--test_csv_path", str(pairs_csv)] + extra + ["--opts"] + opts
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        log = r.stdout + r.stderr
        assert r.returncode == 0, log[-4000:]
        return log, tmp_path / tag / "run_preds"

    log, out = run("on", 2, ["--native_preds"])
    assert "NativeDiceGlobal" in log and "NativeIoUGlobal" in log and "NativeDiceScan" in log and "SegDiceGlobal" in log, log[-4000:]
    voxel_ml = 1.5 * 0.8 * 2.0 / 1000.0
    for ip, _ in pairs:
        raw, slope, _, aff = read_nifti(str(out / (os.path.basename(ip)[:-7] + "_native.nii.gz")))
        iraw, _, _, iaff = read_nifti(ip)
        assert raw.shape == iraw.shape == (10, 14, 24) and raw.dtype == np.int16 and slope is None
        assert np.abs(aff - iaff).max() < 1e-6 and np.abs(aff - AFF_B).max() < 1e-6
        assert raw.min() >= 0 and raw.max() < 3
    with open(out / "native_volumes.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["name", "class_0_ml", "class_1_ml", "class_2_ml"] and [r[0] for r in rows[1:]] == [ip for ip, _ in pairs]
    for r in rows[1:]:
        assert abs(sum(float(v) for v in r[1:]) - 24 * 14 * 10 * voxel_ml) < 1e-4
    assert len([f for f in os.listdir(tmp_path / "cache") if f.endswith(".json")]) == 4  # one geometry file per scan
    log, out = run("off", 1, ["--save_preds"])
    assert "NativeDiceGlobal" not in log
    files = sorted(os.listdir(out))
    assert len(files) == 4 and all(f.endswith("_pred.nii.gz") for f in files), files
