"""What the random 3-D affine of segmentation fine-tuning costs: the labels' half (hct_affine_labels) alone, and the training step.

Default: the label volumes of a [64, 96^3] batch out of a pool of 128 uint8 items, four cases alternating in one process after a warm-up:
  labels_p1    hct_affine_labels with every sample firing (rotation up to 10 degrees per axis, zoom +-10 %, translation +-5 % of the
               side, flips folded in): gather and nearest-neighbour resampling in one launch
  labels_p05   the same launch with half of the samples firing; the others take the flip / copy path
  gather       hct_gather_flip_labels alone: the cost of a batch's labels without the affine, and the floor of the launch
  torch        the composition torch offers: index_select -> .float() -> affine_grid -> grid_sample(mode='nearest', zeros,
               align_corners=True) -> flip -> .to(uint8).  The flip is ONE flip of the whole batch along the contiguous axis, and its
               ties round half to even, so it is not even the same function; the comparison leans towards torch.
Per case the median round and the spread between rounds, in microseconds, GB/s over 2 bytes per voxel (one read, one written) and the
share of the 6.29 TB/s a float4 copy reaches on an MI355X.

`--step` instead runs the segmentation step of scripts/bench_seg.py --step (ViT-B/12^3, 96^3 x 3 channels, B = 64, bf16,
SegmentationHead with K = 2, seg_loss with the gradient in place) in three legs, alternating blocks in one process:
  fixed_batch  that script's own step, on one fixed batch: no loader
  loader_off   the batch made by `augment_segmentation_batch` as the train loader makes it (host draws, pinned uploads,
               hct_augment_volume + hct_gather_flip_labels) out of a stacked fp16 batch and its labels, SEG.AFFINE_PROB 0
  loader_on    the same with SEG.AFFINE_PROB 0.5 (hct_affine_augment + hct_affine_labels)
Prints one JSON line.

  python scripts/bench_seg_affine.py [--iters 10] [--warmup 3] [--rounds 5] [--step] [--out profiles/seg_affine_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from headct_foundation_amd import _lib  # noqa: E402
from headct_foundation_amd.data import DeviceAugment, RandAffine3D, SyntheticSegmented, augment_segmentation_batch  # noqa: E402
from headct_foundation_amd.dino_model import ViTBackbone  # noqa: E402
from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_  # noqa: E402
from headct_foundation_amd.segmentation import SegmentationHead, seg_loss  # noqa: E402

HBM_COPY_GBS = 6290.0  # float4 copy on an MI355X: what a streaming pass can reach, GB/s
N_POOL = 128
RECIPE = dict(rotate_deg=10.0, scale=0.1, translate=0.05)


def event_us(call, iters: int) -> float:
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / iters


def summary(rounds) -> dict:
    return {"us": round(statistics.median(rounds), 1), "rounds_us": [round(v, 1) for v in rounds],
            "spread_pct": round(100 * (max(rounds) - min(rounds)) / min(rounds), 2)}


def kernel_part(lib, dev, B: int, S: int, iters: int, warmup: int, n_rounds: int) -> dict:
    g = torch.Generator(device=dev).manual_seed(0)
    pool = torch.randint(0, 3, (N_POOL, S, S, S), device=dev, generator=g, dtype=torch.uint8)
    slot = torch.randint(0, N_POOL, (B,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(dev)
    aug = DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=0, affine=RandAffine3D(prob=0.5, seed=0, **RECIPE))
    flip, _ = aug.draw(B)
    mat, _ = aug.draw_affine(B, S, flip)
    half = (torch.arange(B) % 2).to(torch.uint8)
    flip_d, mat_d, half_d = flip.to(dev), mat.to(dev), half.to(dev)
    out = torch.empty(B, S, S, S, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    cen = (S - 1) / 2
    m = mat.view(B, 3, 4)
    theta = torch.cat([m[:, :, :3].flip(1).flip(2), (m[:, :, 3:] / cen).flip(1)], dim=2).to(dev)  # (x, y, z) = (axis 2, 1, 0), normalised
    long_slot = slot.long()

    def labels(fire):
        _lib.check(lib.hct_affine_labels(pool.data_ptr(), slot.data_ptr(), N_POOL, out.data_ptr(), B, S, mat_d.data_ptr(), _lib.ptr(fire),
                                         flip_d.data_ptr(), 0, st), "hct_affine_labels")

    def gather():
        _lib.check(lib.hct_gather_flip_labels(pool.data_ptr(), slot.data_ptr(), out.data_ptr(), B, S, N_POOL, flip_d.data_ptr(), st),
                   "hct_gather_flip_labels")

    def composition():
        x = pool.index_select(0, long_slot).unsqueeze(1).float()
        grid = F.affine_grid(theta, list(x.shape), align_corners=True)
        return F.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=True).flip(4).to(torch.uint8)

    cases = {"labels_p1": lambda: labels(None), "labels_p05": lambda: labels(half_d), "gather": gather, "torch": composition}
    for call in cases.values():
        for _ in range(warmup):
            call()
    torch.cuda.synchronize()
    rounds = {k: [] for k in cases}
    for _ in range(n_rounds):  # the cases alternate inside one process
        for k, call in cases.items():
            rounds[k].append(event_us(call, iters))
    vox = B * S ** 3
    res = {"shape": [B, S, S, S], "pool_items": N_POOL, "recipe": RECIPE, "iters": iters, "warmup": warmup, "rounds": n_rounds,
           "bytes_floor": 2 * vox, "hbm_floor_us": round(2 * vox / HBM_COPY_GBS / 1e3, 1)}
    for k in cases:
        res[k] = summary(rounds[k])
        if k != "torch":
            gbs = 2 * vox / res[k]["us"] / 1e3
            res[k].update(GB_per_s=round(gbs, 1), share_of_hbm_floor_pct=round(100 * gbs / HBM_COPY_GBS, 1))
    res["labels_p1_over_torch"] = round(res["labels_p1"]["us"] / res["torch"]["us"], 3)
    res["labels_p1_over_gather"] = round(res["labels_p1"]["us"] / res["gather"]["us"], 3)
    res["labels_p05_over_gather"] = round(res["labels_p05"]["us"] / res["gather"]["us"], 3)
    return res


def step_part(dev, B: int, steps: int, warmup: int, n_rounds: int) -> dict:
    torch.manual_seed(0)
    S, C, K = 96, 3, 2
    vit = ViTBackbone(in_chans=C, img_size=S, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12,
                      compute_dtype="bf16").to(dev).train()
    head = SegmentationHead(768, 12, K).to(dev).train()
    opts = [HipAdamW(head, lr=1.5e-1, weight_decay=0.04), HipAdamW(vit, lr=1.5e-3, weight_decay=0.04)]
    v, y, _ = SyntheticSegmented(1, B, C, S, K, dev, seed=0).batches[0]
    x16 = v.to(torch.float16)  # what the cache hands the loader
    augs = {"loader_off": DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=0),
            "loader_on": DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=0, affine=RandAffine3D(prob=0.5, seed=0, **RECIPE))}

    def batch(leg):
        if leg == "fixed_batch":
            return v, y
        out, labels, _ = augment_segmentation_batch(x16, y, augs[leg], None, 0)
        return out, labels

    def step(leg):
        for o in opts:
            o.zero_grad()
        data, labels = batch(leg)
        loss = seg_loss(head(vit(data)[0]), labels, 12, K, 1, inplace_grad=True)
        loss.backward()
        clip_grad_norm_(head, 1.0)
        clip_grad_norm_(vit, 1.0)
        for o in opts:
            o.step()
        return loss

    def timed(leg) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step(leg)
        torch.cuda.synchronize()
        if not torch.isfinite(loss.detach()):
            raise SystemExit("non-finite loss")
        return (time.perf_counter() - t0) * 1e3 / steps

    legs = ["fixed_batch", "loader_off", "loader_on"]
    for leg in legs:
        for _ in range(warmup):
            step(leg)
    rounds = {leg: [] for leg in legs}
    for _ in range(n_rounds):
        for leg in legs:
            rounds[leg].append(timed(leg))
    res = {"metric": "segmentation step (ViT-B/12^3, 96^3 x 3, SegmentationHead K = 2, bf16, one MI355X), ms per step", "batch": B, "steps": steps,
           "warmup": warmup, "rounds": n_rounds, "affine_prob": 0.5, "recipe": RECIPE}
    for leg in legs:
        r = rounds[leg]
        res[leg] = {"ms_per_step": round(statistics.median(r), 3), "rounds_ms": [round(x, 3) for x in r],
                    "spread_pct": round(100 * (max(r) - min(r)) / min(r), 2)}
    res["affine_cost_pct"] = round(100 * (res["loader_on"]["ms_per_step"] / res["loader_off"]["ms_per_step"] - 1), 2)
    res["loader_cost_pct"] = round(100 * (res["loader_off"]["ms_per_step"] / res["fixed_batch"]["ms_per_step"] - 1), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="calls per timed round (kernel part) or steps per round (--step)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--step", action="store_true", help="time the segmentation step with the affine off and on instead of the launch alone")
    ap.add_argument("--out", default="", help="also write the JSON to this file (with --step: merged into it under the key 'step')")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_affine.py needs an MI355X: a timing off the GPU says nothing")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    if a.step:
        result = step_part(dev, a.batch, a.iters, a.warmup, a.rounds)
    else:
        result = {"metric": "hct_affine_labels against hct_gather_flip_labels and the torch composition (one MI355X), microseconds per call"}
        result.update(kernel_part(lib, dev, a.batch, a.size, a.iters, a.warmup, a.rounds))
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        merged = result
        if a.step and os.path.isfile(a.out):  # one file for both parts
            with open(a.out) as f:
                merged = json.load(f)
            merged["step"] = result
        with open(a.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()
