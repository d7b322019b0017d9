"""The fine-tuning loader's batch assembly at the RSNA yaml's shape: B 64 items of 3 x 96^3 fp16 out of a device-resident pool,
fp32 out (340 MB read, 679 MB written per batch).

    python scripts/bench_finetune_data.py [--batch 64] [--slots 256] [--reps 5] [--iters 10]
        hct_gather_augment (one launch) against the route it replaces on the same pool, index_select into an fp16 batch and then
        hct_augment_volume, with the same slots, flips and shifts; HIP events around `iters` calls, the cases alternating over
        `reps` repeats, a device copy as the yardstick for bandwidth.  The HBM floor of a route is its algorithmic bytes (fused:
        2 read + 4 written per voxel; two-pass: 2 + 2 and 2 + 4) over the copy's measured bandwidth.  One JSON line.
    python scripts/bench_finetune_data.py --epoch [--scans 256] [--samples 500] [--blocks 3]
        one fine-tuning epoch (bench_finetune.py's linear, unlocked ViT-B step fed by LabelledVolumes with the class-balanced
        sampler, `samples` draws in batches of `batch`) with the pool on against the pool off, alternating epochs in one process.
        The scans are random fp16 items written into a temporary VolumeCache directory first, so the pool-off arm reads a disk
        cache that the page cache holds (just written).  Also each loader drained alone, for the data share of a step.  One JSON line.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from headct_foundation_amd import _lib  # noqa: E402
from headct_foundation_amd.data import (DeviceAugment, DevicePool, LabelledVolumes, VolumeCache, WeightedShardSampler,  # noqa: E402
                                        class_weights)

C, S = 3, 96


def timed(fn, iters):
    """ms per call: HIP events around `iters` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def assembly(args):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    B, n = args.batch, args.slots
    g = torch.Generator(device=dev).manual_seed(42)
    pool = torch.rand(n, C, S, S, S, device=dev, generator=g, dtype=torch.float32).to(torch.float16)
    aug = DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=42)
    tables = []
    for k in range(2):
        flip, shift = aug.draw(B)
        slot = torch.randint(0, n, (B,), generator=torch.Generator().manual_seed(k), dtype=torch.int32)
        tables.append((slot.to(dev), slot.long().to(dev), flip.to(dev), shift.to(dev)))
    out = torch.empty(B, C, S, S, S, dtype=torch.float32, device=dev)
    src = torch.empty_like(out)
    half = torch.empty(B, C, S, S, S, dtype=torch.float16, device=dev)
    st = _lib.stream_ptr()
    k = [0]

    def fused():
        k[0] += 1
        slot, _, flip, shift = tables[k[0] % 2]
        _lib.check(lib.hct_gather_augment(pool.data_ptr(), slot.data_ptr(), out.data_ptr(), B, C, S, n, flip.data_ptr(), shift.data_ptr(), st),
                   "hct_gather_augment")

    def two_pass():
        k[0] += 1
        _, index, flip, shift = tables[k[0] % 2]
        torch.index_select(pool, 0, index, out=half)
        _lib.check(lib.hct_augment_volume(half.data_ptr(), _lib.HCT_F16, out.data_ptr(), B, C, S, flip.data_ptr(), shift.data_ptr(), st),
                   "hct_augment_volume")

    cases = {"gather_augment": fused, "index_select_then_augment_volume": two_pass, "device_copy_of_the_output": lambda: out.copy_(src)}
    for fn in cases.values():
        fn()
    fused()
    a = out.clone()
    k[0] -= 1
    two_pass()
    torch.cuda.synchronize()
    if not torch.equal(a, out):
        raise SystemExit("the two routes disagree")
    ms = {name: [] for name in cases}
    for _ in range(args.reps):  # the cases alternate, so a drift of the box hits all of them
        for name, fn in cases.items():
            ms[name].append(timed(fn, args.iters))
    med = {name: statistics.median(v) for name, v in ms.items()}
    vox = B * C * S ** 3
    copy_bw = 2 * out.numel() * 4 / (med["device_copy_of_the_output"] * 1e-3)  # bytes read + written per second
    byts = {"gather_augment": 6 * vox, "index_select_then_augment_volume": 10 * vox}
    print(json.dumps({
        "metric": "fine-tuning batch assembly out of a device-resident fp16 pool (gather, flips, shift, fp32 out)",
        "batch": B, "in_chans": C, "volume": S, "pool_slots": n, "reps": args.reps, "iters": args.iters,
        "ms": {name: stats(v) for name, v in ms.items()},
        "algorithmic_bytes": byts, "GBps": {name: round(b / med[name] / 1e6, 1) for name, b in byts.items()},
        "copy_GBps_read_plus_written": round(copy_bw / 1e9, 1),
        "hbm_floor_ms": {name: round(b / copy_bw * 1e3, 4) for name, b in byts.items()},
        "share_of_floor": {name: round(b / copy_bw * 1e3 / med[name], 3) for name, b in byts.items()},
        "fused_over_two_pass": round(med["gather_augment"] / med["index_select_then_augment_volume"], 3),
        "items_per_s_fused": round(B / (med["gather_augment"] * 1e-3), 1)}), flush=True)


def epoch(args):
    from headct_foundation_amd.classifier import LinearClassifier, cross_entropy
    from headct_foundation_amd.dino_model import ViTBackbone
    from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_
    dev = torch.device("cuda", 0)
    B, n = args.batch, args.scans
    root = tempfile.mkdtemp(prefix="finetune_data_")
    try:
        g = torch.Generator(device=dev).manual_seed(42)
        make = lambda path, roi, chans, device: torch.rand((chans,) + tuple(roi), device=device, generator=g).to(torch.float16)
        cache = VolumeCache(root, S, C, loader=make)
        paths = [f"/scans/{i}.nii.gz" for i in range(n)]
        for p in paths:
            cache.get(p, dev)
        labels = [int(i % 10 == 0) for i in range(n)]  # 9 : 1
        label_of = dict(zip(paths, labels))
        weights = class_weights(labels, 2).double().numpy()[labels]

        def loader(pooled):
            pool = DevicePool(cache, n, dev, B, args.workers) if pooled else None
            return LabelledVolumes(paths, label_of, WeightedShardSampler(weights, args.samples, seed=42), cache, B, dev,
                                   DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=42), pool, args.workers)
        arms = {"pool_on": loader(True), "pool_off": loader(False)}
        torch.manual_seed(0)
        vit = ViTBackbone(in_chans=C, img_size=S, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12, compute_dtype="bf16").to(dev)
        cls = LinearClassifier(768, 2).to(dev).train()
        opts = [HipAdamW(cls, lr=1.5e-1, weight_decay=0.04), HipAdamW(vit, lr=1.5e-5, weight_decay=0.04)]

        def run(ld, train):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for v, t, _ in ld:
                if not train:
                    continue
                for o in opts:
                    o.zero_grad()
                loss = cross_entropy(cls(vit(v)[0]), t)
                loss.backward()
                clip_grad_norm_(cls, 1.0)
                clip_grad_norm_(vit, 1.0)
                for o in opts:
                    o.step()
                float(loss)  # the engine reads the loss every step (all_reduce_mean + isfinite)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        fill_s = run(arms["pool_on"], False)  # the pool's first epoch: every item of the draws goes up once
        run(arms["pool_off"], False)
        for ld in arms.values():
            run(ld, True)
        ep, alone = {name: [] for name in arms}, {name: [] for name in arms}
        for _ in range(args.blocks):
            for name, ld in arms.items():
                ep[name].append(run(ld, True))
            for name, ld in arms.items():
                alone[name].append(run(ld, False))
        steps = len(arms["pool_on"])
        med = lambda v: statistics.median(v)
        print(json.dumps({
            "metric": "one fine-tuning epoch (ViT-B/12^3 linear head, bf16) fed by LabelledVolumes, device pool on vs off, alternating epochs",
            "batch": B, "scans": n, "samples_per_epoch": args.samples, "steps_per_epoch": steps, "workers": args.workers, "blocks": args.blocks,
            "disk_cache": "written by this process just before: served from the page cache",
            "pool_first_epoch_loader_alone_s": round(fill_s, 3), "pool_resident_items": len(arms["pool_on"].pool.slot_of),
            "epoch_s": {name: [round(t, 3) for t in v] for name, v in ep.items()},
            "epoch_median_s": {name: round(med(v), 3) for name, v in ep.items()},
            "loader_alone_s": {name: [round(t, 3) for t in v] for name, v in alone.items()},
            "loader_alone_ms_per_batch": {name: round(med(v) / steps * 1e3, 2) for name, v in alone.items()},
            "data_share_of_epoch": {name: round(med(alone[name]) / med(ep[name]), 3) for name in arms},
            "pool_on_over_pool_off": round(med(ep["pool_on"]) / med(ep["pool_off"]), 3)}), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--epoch", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--workers", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune_data.py measures on the GPU; there is no CPU path")
    (epoch if args.epoch else assembly)(args)
