"""The fine-tuning loader on the device: hct_gather_augment against index_select + hct_augment_volume (bit-equal: the same
arithmetic), LabelledVolumes with and without the device pool, eviction under a pool smaller than the shard, and
main_downstream.py fed from label CSVs of phantom NIfTI files (class-balanced and few-shot)."""
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd.data import DeviceAugment, DevicePool, LabelledVolumes, VolumeCache, gather_augment
from tests import loading_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RSNA = ["img_path", "epidural", "intraparenchymal", "intraventricular", "subarachnoid", "subdural", "any", "study_id"]


def _augment_volume(lib, x, flip, shift):
    """hct_augment_volume on an fp16 batch (the route the loaders took before the pool)."""
    B, C, S = x.shape[0], x.shape[1], x.shape[2]
    out = torch.full((B, C, S, S, S), float("nan"), device=x.device)
    _lib.check(lib.hct_augment_volume(x.data_ptr(), _lib.HCT_F16, out.data_ptr(), B, C, S, _lib.ptr(flip), _lib.ptr(shift), _lib.stream_ptr()),
               "hct_augment_volume")
    return out


def _gathered(pool, slot):
    """pool.index_select(0, slot) with the all-zero volume for slot -1."""
    x = pool.index_select(0, slot.clamp(min=0).long())
    x[slot < 0] = 0
    return x


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("S", [16, 12, 24])  # 16: the existing augment test's; 12: rows that are only 8-byte aligned
def test_gather_augment_is_bit_equal_to_gather_then_augment(lib, cuda, C, S):
    g = torch.Generator(device=cuda).manual_seed(100 * C + S)
    n = 7
    pool = (torch.rand(n, C, S, S, S, device=cuda, generator=g) * 2 - 0.5).to(torch.float16)
    before = pool.clone()
    slot = torch.tensor([3, 0, 6, 3, -1, 5, 1, 3, -1, 2, 6], dtype=torch.int32, device=cuda)  # repeats, placeholders
    B = slot.numel()
    flip = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 5, 7, 0], dtype=torch.uint8, device=cuda)  # all eight codes
    shift = torch.tensor([0.0, 0.05, -0.1, 0.0, 0.0999, -0.03, 0.0, 0.07, 0.01, -0.0625, 0.1], device=cuda)
    out = torch.full((B, C, S, S, S), float("nan"), device=cuda)
    call = lambda f, s: _lib.check(lib.hct_gather_augment(pool.data_ptr(), slot.data_ptr(), out.data_ptr(), B, C, S, n, _lib.ptr(f), _lib.ptr(s),
                                                          _lib.stream_ptr()), "hct_gather_augment")
    call(flip, shift)
    want = _augment_volume(lib, _gathered(pool, slot), flip, shift)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))  # bit patterns, signed zeros included
    assert float(out[4].abs().max()) == float(abs(shift[4]))  # the placeholder went through the arithmetic
    for f, s in ((None, None), (flip, None), (None, shift)):
        out.fill_(float("nan"))
        call(f, s)
        want = _augment_volume(lib, _gathered(pool, slot), f, s)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    call(None, None)
    torch.cuda.synchronize()
    assert torch.equal(out[0], pool[3].float()) and torch.equal(pool, before)  # the plain widening gather; the pool is only read
    # the Python door: the same launch; host-side slots are checked, device-side ones are clamped to the placeholder in the kernel
    assert torch.equal(gather_augment(pool, slot, flip, shift), _augment_volume(lib, _gathered(pool, slot), flip, shift))
    for bad in ([0, n], [-2, 1]):
        with pytest.raises(ValueError, match="slots"):
            gather_augment(pool, torch.tensor(bad, dtype=torch.int32))
    far = gather_augment(pool, torch.tensor([n, -5, 2 ** 31 - 1, 1], dtype=torch.int32, device=cuda), None, shift[:4].contiguous())
    torch.cuda.synchronize()
    assert all(bool((far[b] == shift[b]).all()) for b in range(3)) and torch.equal(far[3], pool[1].float() + shift[3])
    assert lib.hct_gather_augment(pool.data_ptr(), slot.data_ptr(), out.data_ptr(), B, C, 10, n, None, None, _lib.stream_ptr()) != 0  # S % 4


class _DeviceLoader:
    """Stands in for load_volume: an item that depends on the path alone; paths with 'bad' in them fail."""

    def __init__(self):
        self.calls = []

    def __call__(self, path, roi, in_channels, device):
        if "bad" in path:
            raise ValueError(f"{path}: not a NIfTI file")
        self.calls.append(path)
        g = torch.Generator().manual_seed(sum(path.encode()))
        return torch.rand((in_channels,) + tuple(roi), generator=g).to(torch.float16).to(device)


def _epochs(loader, n):
    out = [[(v, t, names) for v, t, names in loader] for _ in range(n)]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)) and torch.equal(x[1], y[1]) and x[2] == y[2]
                                    for x, y in zip(a, b))


def test_labelled_volumes_pool_on_equals_pool_off(lib, cuda, tmp_path, capsys):
    paths = [f"/scans/{'bad' if i == 5 else 'ok'}_{i}.nii.gz" for i in range(11)]
    label_of = {p: i % 2 for i, p in enumerate(paths)}
    order = [0, 5, 3, 3, 10, 7, 5, 1, 2, 9, 4, 8, 6]

    def run(pooled, train, sub):
        cache = VolumeCache(tmp_path / sub, 16, 3, loader=_DeviceLoader())
        pool = DevicePool(cache, 11, cuda, 4, num_workers=3) if pooled else None
        aug = DeviceAugment(flip_prob=0.3, shift_offsets=0.1, shift_prob=0.5, seed=17) if train else None
        return _epochs(LabelledVolumes(paths, label_of, order, cache, 4, cuda, aug, pool, num_workers=3), 2), cache
    for train in (True, False):
        (on, c_on), (off, _) = run(True, train, f"on{train}"), run(False, train, f"off{train}")
        assert len(on[0]) == 4 and _same(on[0], off[0]) and _same(on[1], off[1])
        assert sorted(c_on.loader.calls) == sorted(set(paths[i] for i in order if i != 5))  # once per scan over both epochs
        v, t, names = on[0][0]
        assert v.dtype == torch.float32 and v.is_cuda and t.dtype == torch.int64 and t.is_cuda and tuple(v.shape) == (4, 3, 16, 16, 16)
        assert names == [paths[0], "None", paths[3], paths[3]] and t.tolist() == [0, 0, 1, 1]
        if train:
            assert not _same(on[0], on[1])  # a new draw of flips and shifts
        else:
            assert _same(on[0], on[1]) and float(v[1].abs().max()) == 0.0 and torch.equal(v[2], c_on.get(paths[3], cuda).float())
    assert capsys.readouterr().out.count("Error loading index 5:") == 2 * 2 * 2 * 2  # twice an epoch, two epochs, on and off, train and val


def test_pool_smaller_than_the_shard_serves_the_same_items(lib, cuda, tmp_path):
    paths = [f"/scans/ok_{i}.nii.gz" for i in range(10)]
    label_of = {p: i % 2 for i, p in enumerate(paths)}
    order = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 4, 8, 1]
    cache = VolumeCache(tmp_path / "c", 16, 1, loader=_DeviceLoader())

    def loader(capacity):
        return LabelledVolumes(paths, label_of, order, cache, 4, cuda, None, DevicePool(cache, capacity, cuda, 4, num_workers=2))
    small = loader(4)
    first, second = _epochs(small, 2)  # every batch of both epochs is kept, and compared only after the stream has drained
    assert small.pool.evictions > 0 and len(small.pool.slot_of) == 4
    fresh = _epochs(loader(4), 1)[0]
    whole = _epochs(loader(10), 1)[0]
    assert _same(first, second) and _same(second, fresh) and _same(first, whole)
    want = torch.stack([cache.get(paths[i], cuda).float() for i in order])
    assert torch.equal(torch.cat([v for v, _, _ in first]), want) and torch.equal(torch.cat([v for v, _, _ in second]), want)


# ---- the entry point ----------------------------------------------------------------------------------------------------------------
def _label_csvs(tmp_path):
    """16 phantom scans (8 train, 4 val, 4 test), class 1 with a bright blob; CSVs with the RSNA header, `any` = the class."""
    csvs, rows_of = [], {}
    k = 0
    for split, n in (("train", 8), ("val", 4), ("test", 4)):
        rows = []
        for i in range(n):
            label = i % 2
            hu = R.phantom((28, 30, 26), seed=k)
            if label:
                hu[8:18, 9:19, 7:17] = 900.0
            p = str(tmp_path / f"{split}{i}.nii.gz")
            R.write_nifti(p, R.to_int16(hu, R.INT16_SLOPE, R.INT16_INTER), np.eye(4), slope=R.INT16_SLOPE, inter=R.INT16_INTER)
            rows.append((p, label))
            k += 1
        path = tmp_path / f"{split}.csv"
        path.write_text(",".join(RSNA) + "\n" + "".join(f"{p},0,0,{(i + 1) % 2},0,0,{y},ID_{i}\n" for i, (p, y) in enumerate(rows)))
        csvs.append(str(path))
        rows_of[split] = rows
    return csvs, rows_of


@pytest.mark.parametrize("few_shots", [-1, 2])
def test_main_downstream_trains_from_label_csvs(lib, cuda, tmp_path, few_shots):
    """main_downstream.py through torch.distributed.run on label CSVs: tiny ViT, 2 epochs, validation every epoch; both
    checkpoints, the predictions pickle with the test CSV's paths and labels, the cache directory filled."""
    from headct_foundation_amd.dino_model import ViTBackbone
    (train_csv, val_csv, test_csv), rows_of = _label_csvs(tmp_path)
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3)
    torch.save({"state_dict": {"module." + k: v for k, v in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n  ROI: [24, 24, 24]\n")
    opts = ["DATA.SYNTHETIC", "False", "DATA.TRAIN_SAMPLES_PER_RANK", "16", "DATA.CACHE_DIR", str(tmp_path / "cache"), "VIT.INPUT_SIZE", "24",
            "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3",
            "TRAIN.VAL_EVERY", "1", "MODEL.DIR", str(tmp_path / "out"), "MODEL.SAVE_NAME", "ft.pt", "LOG.OUTPUT_DIR", str(tmp_path / "log"),
            "PREDS_SAVE_NAME", "run"]
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = str(sock.getsockname()[1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", port,
           os.path.join(ROOT, "main_downstream.py"), "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"),
           "--classifier", "linear", "--batch_size", "4", "--max_epochs", "2", "--grad_clip", "1.0", "--base_lr", "1e-4", "--dataset", "rsna",
           "--label_name", "any", "--train_csv_path", train_csv, "--val_csv_path", val_csv, "--test_csv_path", test_csv]
    if few_shots != -1:
        cmd += ["--few_shots", str(few_shots)]
    r = subprocess.run(cmd + ["--opts"] + opts, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "MulticlassAUROC" in log and "Final test loss" in log and "Error loading" not in log, log[-4000:]
    steps = 4 if few_shots == -1 else 1  # 16 draws, or 2 rows x 2 classes, in batches of 4
    assert f"Total Steps: {2 * steps}" in log and f"Epoch 2/2 [{steps}/{steps}]" in log, log[-4000:]
    assert ("Class weights: [2.0, 2.0]" in log) == (few_shots == -1) and ("Class weights: None" in log) == (few_shots != -1)
    for name in ("ft.pt", "ft_classifier.pt"):
        assert os.path.isfile(tmp_path / "out" / name), name
    vit.load_state_dict(torch.load(tmp_path / "out" / "ft.pt", weights_only=True)["state_dict"], strict=True)
    with open(tmp_path / "out" / "run_preds.pkl", "rb") as f:
        preds = pickle.load(f)
    assert list(preds["fnames"]) == [p for p, _ in rows_of["test"]] and preds["targets"].tolist() == [y for _, y in rows_of["test"]]
    assert len(preds["preds"]) == 4 and np.isfinite(preds["preds"]).all()
    cached = [f for f in os.listdir(tmp_path / "cache") if f.endswith(".pt")]
    assert 8 + 1 <= len(cached) <= 16  # every val and test scan, and what the train draws touched
