"""The host side of the fine-tuning loader (headct_foundation_amd/data.py): label columns and class weights against pandas, the
class-balanced shard sampler against torch's DistributedSampler, the few-shot table's properties, the device pool's bookkeeping
on CPU tensors, LabelledVolumes' placeholder rule and lengths, the two loader doors and the config keys.  The CSVs are written
here with the headers of the reference's RSNA and CQ500 label files."""
import logging
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest
import torch
from torch.utils.data import DistributedSampler

from headct_foundation_amd import data as D
from headct_foundation_amd import nifti
from headct_foundation_amd.data import (DevicePool, LabelledVolumes, VolumeCache, WeightedShardSampler, class_weights, fewshot_rows,
                                        get_fewshots_dataloaders, get_finetune_dataloaders, label_column, read_labels)
from tests import loading_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RSNA = ["img_path", "epidural", "intraparenchymal", "intraventricular", "subarachnoid", "subdural", "any", "study_id"]
CQ500 = ["img_path", "ICH", "IPH", "IVH", "SDH", "EDH", "SAH", "BleedLocation-Left", "BleedLocation-Right", "ChronicBleed", "Fracture",
         "CalvarialFracture", "OtherFracture", "MassEffect", "MidlineShift", "Anomaly", "name"]


def _label_csv(path, header, paths, seed=0, column=None, values=None):
    """Rows of random 0/1 labels under `header`; `column` (a name) is set to `values`."""
    g = np.random.default_rng(seed)
    rows = []
    for i, p in enumerate(paths):
        row = [p] + [str(int(v)) for v in g.integers(0, 2, len(header) - 2)] + [f"ID_{i}"]
        if column is not None:
            row[header.index(column)] = str(int(values[i]))
        rows.append(row)
    with open(path, "w") as f:
        f.write(",".join(header) + "\n" + "".join(",".join(r) + "\n" for r in rows))
    return str(path)


class _CountingLoader:
    def __init__(self):
        self.calls = []

    def __call__(self, path, roi, in_channels, device):
        nifti.read_nifti(path)  # reader errors surface as they do in load_volume
        self.calls.append(str(path))
        g = torch.Generator().manual_seed(sum(str(path).encode()))
        return (0.25 + 0.5 * torch.rand((in_channels,) + tuple(roi), generator=g)).to(torch.float16).to(device)


def _scans(tmp_path, n):
    files = []
    for i in range(n):
        files.append(str(tmp_path / f"s{i}.nii"))
        R.write_nifti(files[-1], np.ones((4, 4, 4), np.uint8), np.eye(4))
    return files


# ---- labels -------------------------------------------------------------------------------------------------------------------------
def test_label_column_positions_and_refusals():
    assert label_column("rsna", "any") == 6 == RSNA.index("any")
    assert [label_column("cq500", n) for n in CQ500[1:15]] == list(range(1, 15))
    assert label_column("nyu", "cancer") == label_column("longisland", "cancer") == 1 and label_column("nyu", "fracture") == 11
    with pytest.raises(ValueError, match="Unrecognized dataset: kaggle"):
        label_column("kaggle", "any")
    with pytest.raises(ValueError, match="intraparenchymal"):  # the valid names are listed
        label_column("rsna", "ICH")


@pytest.mark.parametrize("header,dataset,name", [(RSNA, "rsna", "any"), (RSNA, "rsna", "subdural"), (CQ500, "cq500", "MidlineShift"),
                                                 (CQ500, "cq500", "ICH")])
def test_labels_and_class_weights_against_pandas(tmp_path, header, dataset, name):
    paths = [f"/data/{i}.nii.gz" for i in range(37)]
    csv = _label_csv(tmp_path / "t.csv", header, paths, seed=len(name))
    idx = label_column(dataset, name)
    got_paths, labels, label_of = read_labels(csv, idx, name)
    df = pd.read_csv(csv)
    assert got_paths == list(df["img_path"]) and labels.tolist() == list(df.iloc[:, idx]) == list(df[name])
    assert label_of == df.set_index("img_path").iloc[:, idx - 1].to_dict()
    y = np.array(list(df.iloc[:, idx]))
    want = torch.tensor([1 / (c / len(y)) for c in np.bincount(y)], dtype=torch.float)
    got = class_weights(labels, 2)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert np.allclose(got.numpy(), len(y) / np.bincount(y), rtol=1e-6)


def test_label_refusals_duplicates_and_header_warning(tmp_path, caplog):
    with pytest.raises(ValueError, match=r"\[1\]"):  # the reference makes inf of an empty class
        class_weights([0, 0, 0], 2)
    with pytest.raises(ValueError):
        class_weights([0, 1, 2], 2)
    # duplicate path: every row counts for the weights, the dictionary keeps the last
    csv = _label_csv(tmp_path / "d.csv", RSNA, ["/a.nii", "/b.nii", "/a.nii"], column="any", values=[0, 1, 1])
    paths, labels, label_of = read_labels(csv, 6, "any")
    assert paths == ["/a.nii", "/b.nii", "/a.nii"] and labels.tolist() == [0, 1, 1] and label_of == {"/a.nii": 1, "/b.nii": 1}
    assert label_of == pd.read_csv(csv).set_index("img_path").iloc[:, 5].to_dict()
    # a header that is not the label's name at that position: warned about, read by position
    with caplog.at_level(logging.WARNING, logger=D.__name__):
        _, by_position, _ = read_labels(csv, 5, "any")
    assert "subdural" in caplog.text and by_position.tolist() == list(pd.read_csv(csv).iloc[:, 5])
    with pytest.raises(ValueError, match="img_path"):
        read_labels(_label_csv(tmp_path / "bad.csv", ["image"] + RSNA[1:], ["/a.nii"]), 6, "any")


# ---- the class-balanced sampler -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_weighted_sampler_shard_is_the_distributed_samplers(world):
    n = 41
    w = np.linspace(1.0, 2.0, n)
    shards = []
    for rank in range(world):
        s = WeightedShardSampler(w, 30, rank, world, seed=7 + rank)
        assert s.shard == list(DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=True, seed=0))
        first, second = list(s), list(s)
        assert len(first) == len(second) == len(s) == 30 and set(first) <= set(s.shard) and set(second) <= set(s.shard)
        assert first != second  # a new draw every epoch, out of the same shard
        again = WeightedShardSampler(w, 30, rank, world, seed=7 + rank)
        assert [list(again), list(again)] == [first, second]  # seeded
        assert list(WeightedShardSampler(w, 30, rank, world, seed=99)) != first
        shards.append(s.shard)
    assert sorted(set(sum(shards, []))) == list(range(n))
    assert len(WeightedShardSampler(w)) == 500  # the reference's sample_size


def test_weighted_sampler_draws_from_its_own_generator():
    w = np.ones(20)
    torch.manual_seed(0)
    a = list(WeightedShardSampler(w, 50, seed=3))
    torch.manual_seed(12345)
    state = torch.get_rng_state()
    b = list(WeightedShardSampler(w, 50, seed=3))
    assert a == b and torch.equal(torch.get_rng_state(), state)  # the global generator is neither read nor advanced


def test_weighted_sampler_balances_classes():
    """9:1 labels, weights total / count: 4000 draws give class 1 a share of 0.5 +- 0.04 (5 sigma of a fair Bernoulli at n = 4000,
    sigma = 0.0079)."""
    y = np.array([0] * 900 + [1] * 100)
    cw = class_weights(y, 2)
    s = WeightedShardSampler(cw.double().numpy()[y], 4000, seed=42)
    share = float(np.mean(y[list(s)]))
    print(f"share of class 1 over 4000 draws: {share:.4f}")
    assert abs(share - 0.5) <= 0.04


# ---- few-shot -----------------------------------------------------------------------------------------------------------------------
def test_fewshot_rows_properties(tmp_path):
    y = np.array([0] * 20 + [1] * 3 + [0] * 7)
    csv = _label_csv(tmp_path / "t.csv", RSNA, [f"/d/{i}.nii" for i in range(len(y))], column="any", values=y)
    for n in (2, 8):  # 8 > the three rows of class 1: with replacement
        rows = fewshot_rows(csv, "any", n, seed=5)
        assert len(rows) == 2 * n and y[rows].tolist() == [0] * n + [1] * n  # n per class, ascending label order, own class only
        assert all(0 <= r < len(y) for r in rows)
    assert len(set(fewshot_rows(csv, "any", 8, seed=5)[8:])) <= 3
    assert fewshot_rows(csv, "any", 8, seed=5) == fewshot_rows(csv, "any", 8, seed=5)
    assert fewshot_rows(csv, "any", 8, seed=5) != fewshot_rows(csv, "any", 8, seed=6)
    with pytest.raises(ValueError, match="ICH"):
        fewshot_rows(csv, "ICH", 2, seed=0)
    with pytest.raises(ValueError):
        fewshot_rows(csv, "any", 0, seed=0)


# ---- the pool's bookkeeping ---------------------------------------------------------------------------------------------------------
def test_pool_loads_each_path_once_while_everything_fits(tmp_path):
    files = _scans(tmp_path, 6)
    cache = VolumeCache(tmp_path / "c", 8, 1, loader=_CountingLoader())
    pool = DevicePool(cache, 6, "cpu", 4, num_workers=2)
    assert pool.buf.shape == (6, 1, 8, 8, 8) and pool.buf.dtype == torch.float16
    for batch in ([0, 1, 2, 3], [4, 5, 0, 0], [3, 2, 1, 5], [5, 4, 3, 2]):
        slots = pool.slots([files[i] for i in batch])
        assert slots.dtype == torch.int32 and slots.shape == (4,)
        for s, i in zip(slots.tolist(), batch):
            assert torch.equal(pool.buf[s], cache.get(files[i], "cpu"))
    assert sorted(cache.loader.calls) == sorted(files) and pool.evictions == 0 and (pool.hits, pool.misses) == (9, 6)
    assert len(set(pool.slot_of.values())) == 6


def test_pool_evicts_least_recently_used_and_pins_the_batch(tmp_path):
    files = _scans(tmp_path, 6)
    cache = VolumeCache(tmp_path / "c", 8, 1, loader=_CountingLoader())
    pool = DevicePool(cache, 3, "cpu", 3)
    resident = lambda: [files.index(p) for p in pool.slot_of]  # least recently used first
    pool.slots_host([files[0], files[1], files[2]])
    assert resident() == [0, 1, 2]
    pool.slots_host([files[0]])               # 0 becomes the most recent
    pool.slots_host([files[3]])               # evicts 1
    assert resident() == [2, 0, 3] and pool.evictions == 1
    pool.slots_host([files[2], files[4]])     # 2 is used by this batch: 0 goes
    assert resident() == [3, 2, 4]
    # a batch that fills the pool: its own hit (4, the most recent) and every slot it was given stay distinct and intact
    slots = pool.slots_host([files[5], files[4], files[0]])
    assert len(set(slots)) == 3 and resident() == [4, 5, 0]
    for s, i in zip(slots, (5, 4, 0)):
        assert torch.equal(pool.buf[s], cache.get(files[i], "cpu"))
    with pytest.raises(ValueError, match="capacity"):
        pool.slots_host(files[:4])  # four different items cannot be resident at once
    with pytest.raises(ValueError, match="capacity 2 is below the batch size 3"):
        DevicePool(cache, 2, "cpu", 3)


def test_pool_reports_failures_as_slot_minus_one(tmp_path):
    files = _scans(tmp_path, 3)
    open(files[1], "wb").write(b"broken")
    pool = DevicePool(VolumeCache(tmp_path / "c", 8, 1, loader=_CountingLoader()), 3, "cpu", 3)
    seen = []
    slots = pool.slots_host([files[0], files[1], files[2], files[1]], on_error=lambda pos, e: seen.append((pos, type(e).__name__)))
    assert slots[1] == slots[3] == -1 and slots[0] >= 0 and slots[2] >= 0 and [p for p, _ in seen] == [1, 3]
    assert files[1] not in pool.slot_of and len(pool.free) == 1  # the slot was not spent


@pytest.mark.parametrize("n,num,rate,budget_items,want", [(100, -1, 1.0, 1000, 100), (100, 30, 1.0, 1000, 30), (100, -1, 0.25, 1000, 25),
                                                          (100, 30, 0.1, 1000, 10), (100, -1, 1.0, 40, 40), (100, 0, 1.0, 1000, 0),
                                                          (100, -1, 1.0, 0, 0), (7, 500, 1.0, 1000, 7), (3, -1, 0.5, 1000, 1)])
def test_pool_capacity_rule(n, num, rate, budget_items, want):
    item = 2 * 3 * 96 ** 3
    assert DevicePool.capacity_for(n, num, rate, budget_items * item + item // 2, item) == want


# ---- the loader ---------------------------------------------------------------------------------------------------------------------
def _widen(x):  # stands in for the device stage, which has no CPU form
    return x.float()


def test_labelled_volumes_placeholder_and_lengths(tmp_path, capsys):
    files = _scans(tmp_path, 5)
    open(files[3], "wb").write(b"broken")
    y = [0, 1, 1, 1, 0]
    csv = _label_csv(tmp_path / "t.csv", RSNA, files, column="any", values=y)
    paths, labels, label_of = read_labels(csv, 6, "any")
    cache = VolumeCache(tmp_path / "c", 8, 3, loader=_CountingLoader())
    val = LabelledVolumes(paths, label_of, list(range(5)), cache, 2, "cpu", augment=_widen, num_workers=2)
    assert len(val) == 3
    batches = list(val)
    assert [tuple(v.shape) for v, _, _ in batches] == [(2, 3, 8, 8, 8), (2, 3, 8, 8, 8), (1, 3, 8, 8, 8)]
    assert all(v.dtype == torch.float32 and t.dtype == torch.int64 for v, t, _ in batches)
    assert torch.cat([t for _, t, _ in batches]).tolist() == [0, 1, 1, 0, 0]  # the corrupt scan's label 1 became 0
    assert sum((n for _, _, n in batches), []) == files[:3] + ["None"] + files[4:]
    assert float(batches[1][0][1].abs().max()) == 0.0 and float(batches[1][0][0].abs().max()) > 0
    assert torch.equal(batches[0][0][1], cache.get(files[1], "cpu").float())
    out = capsys.readouterr().out
    assert "Error loading index 3:" in out and out.count("Error loading index") == 1
    sampler = WeightedShardSampler(class_weights(labels, 2).double().numpy()[labels], 7, seed=1)
    train = LabelledVolumes(paths, label_of, sampler, cache, 2, "cpu", augment=_widen)
    assert len(train) == 4 and [len(n) for _, _, n in train] == [2, 2, 2, 1]


def _config(tmp_path, csvs, **data):
    from config import _C
    cfg = _C.clone()
    cfg.defrost()
    cfg.DATA.SYNTHETIC, cfg.DATA.BATCH_SIZE, cfg.DATA.CACHE_DIR = False, 4, str(tmp_path / "cache")
    cfg.DATA.DATASET, cfg.TRAIN.LABEL_NAME, cfg.DATA.TRAIN_SAMPLES_PER_RANK = "rsna", "any", 10
    cfg.MODEL.ROI, cfg.MODEL.IN_CHANS, cfg.VIT.INPUT_SIZE, cfg.VIT.IN_CHANS = [16, 16, 16], 1, 16, 1
    cfg.DATA.TRAIN_CSV_PATH, cfg.DATA.VAL_CSV_PATH, cfg.DATA.TEST_CSV_PATH = csvs
    for k, v in data.items():
        setattr(cfg.DATA, k, v)
    return cfg


def test_loader_doors(tmp_path):
    y = np.array([0, 1] * 6)
    paths = [f"/d/{i}.nii" for i in range(12)]
    csvs = [_label_csv(tmp_path / f"{k}.csv", RSNA, paths[:n], column="any", values=y) for k, n in (("train", 12), ("val", 5), ("test", 3))]
    out = get_finetune_dataloaders(_config(tmp_path, csvs), "cpu", 0, 1)
    assert len(out) == 4
    train, val, test, weights = out
    assert [len(l) for l in (train, val, test)] == [3, 2, 1] and torch.equal(weights, torch.tensor([2.0, 2.0]))
    assert isinstance(train.sampler, WeightedShardSampler) and train.sampler.num_samples_per_rank == 10
    assert (train.augment.flip_prob, train.augment.shift_offsets, train.augment.shift_prob, train.augment.smooth_prob) == (0.1, 0.1, 0.5, 0.0)
    assert val.augment is None and test.augment is None and val.sampler == [0, 1, 2, 3, 4]
    assert train.pool is val.pool is test.pool and train.pool.capacity == 12 and train.pool.buf.shape == (12, 1, 16, 16, 16)
    # two ranks: val padded by wrapping, each rank's pool sized for what it touches
    r1 = get_finetune_dataloaders(_config(tmp_path, csvs), "cpu", 1, 2)
    assert r1[1].sampler == [1, 3, 0] and r1[2].sampler == [1, 0] and len(r1[0].sampler.shard) == 6
    assert r1[0].pool.capacity == len({paths[i] for i in r1[0].sampler.shard} | {paths[0], paths[1], paths[3]})
    # capacity: CACHE_NUM, CACHE_RATE and the byte budget; 0 GB turns the pool off
    assert get_finetune_dataloaders(_config(tmp_path, csvs, CACHE_NUM=5), "cpu", 0, 1)[0].pool.capacity == 5
    assert get_finetune_dataloaders(_config(tmp_path, csvs, CACHE_RATE=0.5), "cpu", 0, 1)[0].pool.capacity == 6
    assert get_finetune_dataloaders(_config(tmp_path, csvs, DEVICE_POOL_GB=7 * 2 * 16 ** 3 / 2 ** 30), "cpu", 0, 1)[0].pool.capacity == 7
    assert get_finetune_dataloaders(_config(tmp_path, csvs, DEVICE_POOL_GB=0.0), "cpu", 0, 1)[0].pool is None
    with pytest.raises(ValueError, match="capacity"):
        get_finetune_dataloaders(_config(tmp_path, csvs, CACHE_NUM=3), "cpu", 0, 1)
    few = get_fewshots_dataloaders(_config(tmp_path, csvs, FEW_SHOTS=3), "cpu", 0, 1)
    assert len(few) == 4 and few[3] is None and len(few[0].paths) == 6 and len(few[0]) == 2
    assert [few[0].label_of[p] for p in few[0].paths] == [0, 0, 0, 1, 1, 1]
    assert sorted(few[0].sampler) == list(range(6)) and few[0].sampler == list(DistributedSampler(range(6), 1, 0, shuffle=True))
    for door in (get_finetune_dataloaders, lambda *a: get_fewshots_dataloaders(*a)):
        cfg = _config(tmp_path, csvs, FEW_SHOTS=2)
        cfg.MODEL.ROI = [16, 16, 24]
        with pytest.raises(ValueError, match="MODEL.ROI"):
            door(cfg, "cpu", 0, 1)
        with pytest.raises(FileNotFoundError, match="DATA.VAL_CSV_PATH"):
            door(_config(tmp_path, [csvs[0], str(tmp_path / "absent.csv"), csvs[2]], FEW_SHOTS=2), "cpu", 0, 1)
    cfg = _config(tmp_path, csvs)
    cfg.TRAIN.LABEL_NAME = "ICH"
    with pytest.raises(ValueError, match="epidural"):
        get_finetune_dataloaders(cfg, "cpu", 0, 1)


# ---- config and exports -------------------------------------------------------------------------------------------------------------
def test_cli_lands_in_the_config(tmp_path, monkeypatch):
    import main_downstream as M
    from config import _C
    assert _C.DATA.TRAIN_SAMPLES_PER_RANK == 500 and _C.DATA.DEVICE_POOL_GB == 32 and _C.DATA.CACHE_NUM == -1 and _C.DATA.CACHE_RATE == 1.0
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    monkeypatch.setattr(sys, "argv", ["main_downstream.py", "--cfg", str(cfg), "--few_shots", "4", "--dataset", "rsna", "--label_name", "any",
                                      "--train_csv_path", "/d/train.csv", "--opts", "DATA.TRAIN_SAMPLES_PER_RANK", "16", "DATA.DEVICE_POOL_GB", "0.5"])
    _, config = M.parse_option()
    assert (config.DATA.FEW_SHOTS, config.DATA.DATASET, config.TRAIN.LABEL_NAME, config.DATA.TRAIN_CSV_PATH) == (4, "rsna", "any", "/d/train.csv")
    assert config.DATA.TRAIN_SAMPLES_PER_RANK == 16 and config.DATA.DEVICE_POOL_GB == 0.5
    src = open(os.path.join(ROOT, "main_downstream.py")).read()
    assert "NotImplementedError(\"few-shot" not in src and "get_fewshots_dataloaders" in src


def test_gather_augment_is_exported_and_declared(lib):
    import headct_foundation_amd as pkg
    from headct_foundation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "headct_hip.h")).read()
    assert re.search(r"\bhct_gather_augment\s*\(", hdr) and "hct_gather_augment" in _lib.exported_symbols() and hasattr(lib, "hct_gather_augment")
    for s in ("DevicePool", "LabelledVolumes", "gather_augment"):
        assert hasattr(pkg, s), s
    with pytest.raises(_lib.HctError):  # no CPU fallback
        pkg.gather_augment(torch.zeros(2, 1, 8, 8, 8, dtype=torch.float16), torch.tensor([0, 1], dtype=torch.int32))
