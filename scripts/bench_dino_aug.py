"""The DINO multi-crop augmentation (DeviceAugmentDINO3D) at the `bench.py --config dino` shape: B 64 volumes of 3 x 96^3 fp16 in,
2 + 8 views of 3 x 96^3 fp32 out (6.8 GB written per batch).

    python scripts/bench_dino_aug.py [--batch 64] [--reps 5] [--iters 10]
        the augmentation alone, HIP events around `iters` launches, median and spread of `reps` repeats: the resample launch
        (hct_crop_resize_area with the reference's drawn boxes, and with every box the whole volume = one load per output), the
        contrast pair (hct_adjust_contrast, every sample firing), a device copy of the same size as the yardstick for bandwidth,
        and the whole __call__ with its own draws (host clock between two device fences).  The HBM floor of the resample is
        (bytes written + input bytes read once) over the copy's measured bandwidth.  One JSON line.
    python scripts/bench_dino_aug.py --step [--blocks 4] [--block-steps 5]
        the bench.py DINO step fed by MultiCropLoader (crops cut from fp16 volumes every step) against the same step fed by
        pre-generated noise crops, alternating blocks in one process as ab_step.py does; plus the augmentation's own time in the
        same process, so the gap over "step + augmentation" can be read against the spread between blocks.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from headct_foundation_amd import _lib  # noqa: E402
from headct_foundation_amd.data import DeviceAugmentDINO3D, MultiCropLoader, SyntheticVolumes  # noqa: E402

C, S, F, LOCAL = 3, 96, 96, bench.DINO["crops"] - 2


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


def alone(args):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    B, V = args.batch, 2 + LOCAL
    vols = SyntheticVolumes(2, B, C, S, dev, seed=42, dtype=torch.float16).batches
    aug = DeviceAugmentDINO3D(F, 112, 64, LOCAL, seed=42)
    out = torch.empty(V, B, C, F, F, F, dtype=torch.float32, device=dev)
    src = torch.empty_like(out)
    draws = [aug.draw(B, S) for _ in range(2)]
    tables = [aug._upload(d, dev) for d in draws]
    whole = torch.tensor([0, 0, 0, S, S, S], dtype=torch.int32).repeat(V, B, 1).to(dev)
    n = C * F ** 3
    ones = torch.ones(B, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.hct_adjust_contrast_workspace_bytes(B, n), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr()
    k = [0]

    def resample(boxes=None):
        k[0] += 1
        t = tables[k[0] % 2]
        _lib.check(lib.hct_crop_resize_area(vols[k[0] % 2].data_ptr(), _lib.HCT_F16, B, C, S, out.data_ptr(), F, V,
                                            (t[0] if boxes is None else boxes).data_ptr(), t[4].data_ptr(), t[1].data_ptr(), st), "hct_crop_resize_area")

    def contrast():
        _lib.check(lib.hct_adjust_contrast(out[1].data_ptr(), B, n, tables[0][2].data_ptr(), ones.data_ptr(), ws.data_ptr(), ws.numel(), st),
                   "hct_adjust_contrast")

    cases = {"resample_drawn_boxes": resample, "resample_whole_volume_boxes": lambda: resample(whole), "contrast_pair_all_fire": contrast,
             "device_copy_same_size": lambda: out.copy_(src)}
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in cases}
    for _ in range(args.reps):  # the cases alternate, so a drift of the box hits all of them
        for name, fn in cases.items():
            ms[name].append(timed(fn, args.iters))
    resample()
    nonzero = float((out != 0).float().mean())
    for _ in range(2):
        aug(vols[0])
    call = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.iters):
            aug(vols[i % 2])
        torch.cuda.synchronize()
        call.append((time.perf_counter() - t0) / args.iters * 1e3)
    written, read_once = out.numel() * 4, vols[0].numel() * 2
    med = {name: statistics.median(v) for name, v in ms.items()}
    copy_bw = 2 * written / (med["device_copy_same_size"] * 1e-3)  # bytes read + written per second
    floor_ms = (written + read_once) / copy_bw * 1e3
    print(json.dumps({
        "metric": "DINO multi-crop augmentation alone (DeviceAugmentDINO3D, fp16 volumes in, fp32 crops out)",
        "batch": B, "in_chans": C, "volume": S, "final_size": F, "views": V, "reps": args.reps, "iters": args.iters,
        "bytes_written": written, "bytes_read_once": read_once,
        "ms": {name: stats(v) for name, v in ms.items()}, "call_ms": stats(call),
        "resample_GBps_written": round(written / med["resample_drawn_boxes"] / 1e6, 1),
        "resample_whole_volume_GBps_written": round(written / med["resample_whole_volume_boxes"] / 1e6, 1),
        "contrast_GBps_read_twice_written_once": round(3 * B * n * 4 / med["contrast_pair_all_fire"] / 1e6, 1),
        "copy_GBps_read_plus_written": round(copy_bw / 1e9, 1), "resample_hbm_floor_ms": round(floor_ms, 4),
        "resample_share_of_floor": round(floor_ms / med["resample_drawn_boxes"], 3),
        "crops_per_s": round(V * B / (statistics.median(call) * 1e-3), 1), "nonzero_output_fraction_drawn_boxes": round(nonzero, 4)}), flush=True)


def step_ab(args):
    from headct_foundation_amd.dino import DINOLoss, DinoDataParallel, DinoOptimizer, SyntheticCrops, update_momentum_encoder, wd_cosine_scheduler
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    dev = torch.device("cuda", 0)
    B, V = args.batch, 2 + LOCAL
    torch.manual_seed(42)
    mk = lambda: MultiCropWrapper(ViTBackbone(**bench.DINO["vit"], compute_dtype="bf16"), DINOHead(**bench.DINO["head"], compute_dtype="bf16")).to(dev)
    student, teacher = mk(), mk()
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad_(False)
    model, momentum_model = DinoDataParallel(student), DinoDataParallel(teacher)
    lr = 5e-4 * B / 256
    opt = DinoOptimizer(model, lr=lr, betas=(0.9, 0.999), weight_decay=0.04)
    sched = get_cosine_schedule_with_warmup(opt.primary, 100, 1000, lr_end=lr * 1e-3)
    wd, mom = wd_cosine_scheduler(0.04, 0.4, 1, 1000), wd_cosine_scheduler(0.999, 1.0, 1, 1000)
    crit = DINOLoss(bench.DINO["head"]["out_dim"], V, 0.04, 0.04, 30, 200).to(dev)
    aug = DeviceAugmentDINO3D(F, 112, 64, LOCAL, seed=42)
    volumes = SyntheticVolumes(2, B, C, S, dev, seed=42, dtype=torch.float16)
    arms = {"synthetic_crops": SyntheticCrops(2, B, V, C, F, dev, seed=42), "multi_crop_loader": MultiCropLoader(volumes, aug)}
    it = [0]

    def block(loader, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = 0
        while done < n:
            for crops in loader:
                i = it[0]
                it[0] += 1
                opt.param_groups[0]["weight_decay"] = float(wd[i])
                opt.zero_grad()
                with torch.no_grad():
                    t_out = momentum_model(crops[:2])['dino_output']
                s_out = model(crops)['dino_output']
                loss = crit(s_out.float(), t_out.float(), 0)
                loss.backward()
                model.reduce_head_gradients()
                opt.step()
                sched.step()
                update_momentum_encoder(student.backbone, teacher.backbone, float(mom[i]))
                update_momentum_encoder(student.head, teacher.head, float(mom[i]))
                done += 1
                if done == n:
                    break
        torch.cuda.synchronize()
        if not bool(torch.isfinite(loss)):
            raise SystemExit("non-finite loss")
        return (time.perf_counter() - t0) / n * 1e3

    def aug_block(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            aug(volumes.batches[i % 2])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for loader in arms.values():
        block(loader, 2)
    aug_block(2)
    res = {name: [] for name in arms}
    aug_ms = []
    for _ in range(args.blocks):
        for name, loader in arms.items():
            res[name].append(block(loader, args.block_steps))
        aug_ms.append(aug_block(args.block_steps))
    mean = {name: sum(v) / len(v) for name, v in res.items()}
    spread = max(max(v) - min(v) for v in res.values())
    a = sum(aug_ms) / len(aug_ms)
    print(json.dumps({
        "metric": "DINO step (bench.py --config dino workload, bf16) fed by MultiCropLoader vs pre-generated noise crops, alternating blocks",
        "batch": B, "views": V, "blocks": args.blocks, "block_steps": args.block_steps,
        "ms_per_step": {name: [round(t, 3) for t in v] for name, v in res.items()}, "mean_ms_per_step": {name: round(t, 3) for name, t in mean.items()},
        "augmentation_alone_ms": [round(t, 3) for t in aug_ms], "augmentation_alone_mean_ms": round(a, 3),
        "spread_between_blocks_of_one_arm_ms": round(spread, 3),
        "gap_over_step_plus_augmentation_ms": round(mean["multi_crop_loader"] - mean["synthetic_crops"] - a, 3)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block-steps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dino_aug.py measures on the GPU; there is no CPU path")
    (step_ab if args.step else alone)(args)
