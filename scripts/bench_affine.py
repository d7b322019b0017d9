"""What the random 3-D affine costs when a fine-tuning batch is assembled on the HIP path.

Default: a [64, 3, 96, 96, 96] fp32 batch out of a pool of 128 fp16 items, four cases alternating in one process after a warm-up:
  fused_p1    hct_affine_augment with every sample firing (rotation up to 10 degrees per axis, zoom +-10 %, translation +-5 % of the
              side, flips folded in, shift): gather, resampling and shift in one launch
  fused_p05   the same launch with half of the samples firing; the others take the flip / copy / shift path
  gather      hct_gather_augment alone: the cost of a batch without the affine, and the floor of the fused launch
  torch       the composition torch offers: index_select -> .float() -> affine_grid -> grid_sample (bilinear, zeros,
              align_corners=True) -> flip -> add.  The flip is ONE flip of the whole batch along the contiguous axis; per-sample flips
              as the loader draws them would cost torch more, so the comparison leans towards torch.
Per case the median round and the spread between rounds; for the launches GB/s over 2 bytes read + 4 written per voxel and the share
of the HBM floor (the 6.29 TB/s a float4 copy reaches on an MI355X).  `--step` instead runs the fine-tuning step of
scripts/bench_mixup.py (ViT-B/12^3, linear head, B = 64, bf16) INCLUDING the assembly of its batch out of the pool the way
LabelledVolumes does it (host draws, one pinned upload per table, one launch), with the affine off and on (prob 0.5), alternating.
Prints one JSON line.

  python scripts/bench_affine.py [--iters 10] [--warmup 3] [--rounds 5] [--step] [--out profiles/affine_bench.json]
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
from headct_foundation_amd.classifier import LinearClassifier, cross_entropy  # noqa: E402
from headct_foundation_amd.data import DeviceAugment, RandAffine3D, _to_device, gather_augment  # noqa: E402
from headct_foundation_amd.dino_model import ViTBackbone  # noqa: E402
from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_  # noqa: E402

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


def make_pool(dev, C: int, S: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand(N_POOL, C, S, S, S, device=dev, generator=g).to(torch.float16)


def kernel_part(lib, dev, B: int, C: int, S: int, iters: int, warmup: int, n_rounds: int) -> dict:
    pool = make_pool(dev, C, S)
    slot = torch.randint(0, N_POOL, (B,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(dev)
    aug = DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=0, affine=RandAffine3D(prob=0.5, seed=0, **RECIPE))
    flip, shift = aug.draw(B)
    mat, _ = aug.draw_affine(B, S, flip)
    half = (torch.arange(B) % 2).to(torch.uint8)
    flip_d, shift_d, mat_d, half_d = flip.to(dev), shift.to(dev), mat.to(dev), half.to(dev)
    out = torch.empty(B, C, S, S, S, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    # affine_grid's theta: normalised coordinates n = (index - c) / c in (x, y, z) = (axis 2, 1, 0) order
    cen = (S - 1) / 2
    m = mat.view(B, 3, 4)
    theta = torch.cat([m[:, :, :3].flip(1).flip(2), (m[:, :, 3:] / cen).flip(1)], dim=2).to(dev)
    long_slot = slot.long()

    def fused(fire):
        _lib.check(lib.hct_affine_augment(pool.data_ptr(), _lib.HCT_F16, slot.data_ptr(), N_POOL, out.data_ptr(), B, C, S, mat_d.data_ptr(),
                                          _lib.ptr(fire), flip_d.data_ptr(), shift_d.data_ptr(), st), "hct_affine_augment")

    def gather():
        _lib.check(lib.hct_gather_augment(pool.data_ptr(), slot.data_ptr(), out.data_ptr(), B, C, S, N_POOL, flip_d.data_ptr(), shift_d.data_ptr(), st),
                   "hct_gather_augment")

    def composition():
        x = pool.index_select(0, long_slot).float()
        grid = F.affine_grid(theta, list(x.shape), align_corners=True)
        y = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        return y.flip(4).add_(shift_d.view(B, 1, 1, 1, 1))

    cases = {"fused_p1": lambda: fused(None), "fused_p05": lambda: fused(half_d), "gather": gather, "torch": composition}
    for call in cases.values():
        for _ in range(warmup):
            call()
    torch.cuda.synchronize()
    rounds = {k: [] for k in cases}
    for _ in range(n_rounds):  # the cases alternate inside one process
        for k, call in cases.items():
            rounds[k].append(event_us(call, iters))
    vox = B * C * S ** 3
    res = {"shape": [B, C, S, S, S], "pool_items": N_POOL, "recipe": RECIPE, "iters": iters, "warmup": warmup, "rounds": n_rounds,
           "bytes_floor": 6 * vox, "hbm_floor_us": round(6 * vox / HBM_COPY_GBS / 1e3, 1)}
    for k in cases:
        res[k] = summary(rounds[k])
        if k != "torch":
            gbs = 6 * vox / res[k]["us"] / 1e3
            res[k].update(GB_per_s=round(gbs, 1), share_of_hbm_floor_pct=round(100 * gbs / HBM_COPY_GBS, 1))
    res["fused_p1_over_torch"] = round(res["fused_p1"]["us"] / res["torch"]["us"], 3)
    res["fused_p1_over_gather"] = round(res["fused_p1"]["us"] / res["gather"]["us"], 3)
    res["fused_p05_over_gather"] = round(res["fused_p05"]["us"] / res["gather"]["us"], 3)
    return res


def step_part(dev, B: int, steps: int, warmup: int, n_rounds: int) -> dict:
    torch.manual_seed(0)
    S, C = 96, 3
    vit = ViTBackbone(in_chans=C, img_size=S, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12,
                      compute_dtype="bf16").to(dev).train()
    cls = LinearClassifier(768, 2, feature_grad=True).to(dev).train()
    opts = [HipAdamW(cls, lr=1.5e-1, weight_decay=0.04), HipAdamW(vit, lr=1.5e-3, weight_decay=0.04)]
    pool = make_pool(dev, C, S)
    target = (torch.arange(B, device=dev) % 2)
    draws = torch.Generator().manual_seed(2)
    augs = {False: DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=0),
            True: DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=0, affine=RandAffine3D(prob=0.5, seed=0, **RECIPE))}

    def batch(on: bool):  # LabelledVolumes._pooled without the path -> slot map
        aug = augs[on]
        slots = torch.randint(0, N_POOL, (B,), generator=draws, dtype=torch.int32)
        flip, shift = aug.draw(B)
        mat, fire = aug.draw_affine(B, S, flip)
        up = lambda t: None if t is None else _to_device(t, dev)
        return gather_augment(pool, up(slots), up(flip), up(shift), up(mat), up(fire))

    def step(on: bool):
        for o in opts:
            o.zero_grad()
        loss = cross_entropy(cls(vit(batch(on))[0]), target)
        loss.backward()
        clip_grad_norm_(cls, 1.0)
        clip_grad_norm_(vit, 1.0)
        for o in opts:
            o.step()
        return loss

    def timed(on: bool) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step(on)
        torch.cuda.synchronize()
        if not torch.isfinite(loss.detach()):
            raise SystemExit("non-finite loss")
        return (time.perf_counter() - t0) * 1e3 / steps

    for on in (False, True):
        for _ in range(warmup):
            step(on)
    rounds = {False: [], True: []}
    for _ in range(n_rounds):
        for on in (False, True):
            rounds[on].append(timed(on))
    res = {"metric": "fine-tuning step with its batch assembled out of the pool (ViT-B/12^3, linear head, bf16, one MI355X), ms per step",
           "batch": B, "steps": steps, "warmup": warmup, "rounds": n_rounds, "affine_prob": 0.5, "recipe": RECIPE}
    for on, name in ((False, "affine_off"), (True, "affine_on")):
        res[name] = {"ms_per_step": round(statistics.median(rounds[on]), 3), "rounds_ms": [round(r, 3) for r in rounds[on]],
                     "spread_pct": round(100 * (max(rounds[on]) - min(rounds[on])) / min(rounds[on]), 2)}
    res["affine_cost_pct"] = round(100 * (res["affine_on"]["ms_per_step"] / res["affine_off"]["ms_per_step"] - 1), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="calls per timed round (kernel part) or steps per round (--step)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--step", action="store_true", help="time the fine-tuning step with the affine off and on instead of the launch alone")
    ap.add_argument("--out", default="", help="also write the JSON to this file (with --step: merged into it under the key 'step')")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_affine.py needs an MI355X: a timing off the GPU says nothing")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    if a.step:
        result = step_part(dev, a.batch, a.iters, a.warmup, a.rounds)
    else:
        result = {"metric": "hct_affine_augment against hct_gather_augment and the torch composition (one MI355X), microseconds per call"}
        result.update(kernel_part(lib, dev, a.batch, 3, a.size, a.iters, a.warmup, a.rounds))
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
