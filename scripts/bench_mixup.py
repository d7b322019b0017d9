"""What mixing a fine-tuning batch costs on the HIP path.

Default: hct_mix_volumes alone on a [64, 3, 96, 96, 96] fp32 batch (680 MB), in place, for mixup at lam = 0.5 (every voxel of every
sample: one read and one write, 8 bytes per voxel) and for CutMix at lam = 0.5 (one centred cube of side int(96 * 0.5^(1/3)) = 76 per
sample: 8 bytes per voxel of the float4s the boxes overlap, 80 of a row's 96 for the 76 inside, nothing outside), each beside the
torch composition it replaces -- `x.flip(0).mul_(1 - lam)` then `x.mul_(lam).add_(...)` for mixup, `x[..., box] = x.flip(0)[..., box]`
for CutMix.  Kernel and composition alternate in one process,
after a warm-up; per case the median round and the spread between rounds, and for the kernel GB/s and the share of the HBM floor
(the 6.29 TB/s a float4 copy reaches on an MI355X).  `--step` instead runs the fine-tuning step of scripts/bench_drop_path.py (ViT-B/12^3,
linear head, B = 64, bf16) with the recipe off (cross_entropy) and on (Mixup 0.8 / 1.0 in batch mode + soft_cross_entropy at smoothing
0.1), alternating.  Prints one JSON line.

  python scripts/bench_mixup.py [--iters 10] [--warmup 3] [--rounds 5] [--step] [--out profiles/mixup_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from headct_foundation_amd import _lib  # noqa: E402
from headct_foundation_amd.classifier import LinearClassifier, cross_entropy  # noqa: E402
from headct_foundation_amd.data import SyntheticLabelled  # noqa: E402
from headct_foundation_amd.dino_model import ViTBackbone  # noqa: E402
from headct_foundation_amd.mixup import MixedCriterion, Mixup  # noqa: E402
from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_  # noqa: E402

HBM_COPY_GBS = 6290.0  # float4 copy on an MI355X: what a streaming pass can reach, GB/s


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


def kernel_part(lib, dev, B: int, C: int, S: int, iters: int, warmup: int, n_rounds: int) -> dict:
    lam = 0.5
    x = torch.rand(B, C, S, S, S, device=dev)
    lam_d = torch.full((B,), lam, dtype=torch.float32, device=dev)
    ones_d = torch.ones(B, dtype=torch.float32, device=dev)
    cut = int(S * (1.0 - lam) ** (1.0 / 3.0))
    lo, hi = S // 2 - cut // 2, S // 2 + cut // 2
    box_d = torch.tensor([[lo, hi] * 3] * B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def k_mixup():
        _lib.check(lib.hct_mix_volumes(x.data_ptr(), B, C, S, lam_d.data_ptr(), None, st), "hct_mix_volumes")

    def k_cutmix():
        _lib.check(lib.hct_mix_volumes(x.data_ptr(), B, C, S, ones_d.data_ptr(), box_d.data_ptr(), st), "hct_mix_volumes")

    def t_mixup():
        other = x.flip(0).mul_(1.0 - lam)
        x.mul_(lam).add_(other)

    def t_cutmix():
        x[:, :, lo:hi, lo:hi, lo:hi] = x.flip(0)[:, :, lo:hi, lo:hi, lo:hi]

    cases = {"mixup_kernel": k_mixup, "mixup_torch": t_mixup, "cutmix_kernel": k_cutmix, "cutmix_torch": t_cutmix}
    for call in cases.values():
        for _ in range(warmup):
            call()
    torch.cuda.synchronize()
    rounds = {k: [] for k in cases}
    for _ in range(n_rounds):  # kernel and composition alternate inside one process
        for k, call in cases.items():
            rounds[k].append(event_us(call, iters))
    vox = B * C * S ** 3
    # CutMix moves whole float4s: a row of the box costs the vectors it overlaps on the contiguous axis, faces inside a vector included
    row = (hi + 3) // 4 * 4 - lo // 4 * 4
    nbytes = {"mixup_kernel": 8 * vox, "cutmix_kernel": 8 * B * C * (hi - lo) ** 2 * row}
    out = {"shape": [B, C, S, S, S], "lam": lam, "box": [lo, hi] * 3, "iters": iters, "warmup": warmup, "rounds": n_rounds}
    for k in cases:
        out[k] = summary(rounds[k])
        if k in nbytes:
            gbs = nbytes[k] / out[k]["us"] / 1e3
            out[k].update(bytes=nbytes[k], GB_per_s=round(gbs, 1), hbm_floor_us=round(nbytes[k] / HBM_COPY_GBS / 1e3, 1),
                          share_of_hbm_floor_pct=round(100 * gbs / HBM_COPY_GBS, 1))
    out["mixup_kernel_over_torch"] = round(out["mixup_kernel"]["us"] / out["mixup_torch"]["us"], 3)
    out["cutmix_kernel_over_torch"] = round(out["cutmix_kernel"]["us"] / out["cutmix_torch"]["us"], 3)
    return out


def step_part(dev, B: int, steps: int, warmup: int, n_rounds: int) -> dict:
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=96, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12,
                      compute_dtype="bf16").to(dev).train()
    cls = LinearClassifier(768, 2, feature_grad=True).to(dev).train()
    opts = [HipAdamW(cls, lr=1.5e-1, weight_decay=0.04), HipAdamW(vit, lr=1.5e-3, weight_decay=0.04)]
    v, t, _ = SyntheticLabelled(1, B, 3, 96, 2, dev, seed=0).batches[0]
    crit = MixedCriterion(Mixup(0.8, 1.0, mode="batch", seed=0), 0.1)

    def step(on: bool):
        for o in opts:
            o.zero_grad()
        if on:  # the batch is mixed in place, as the engine mixes a loader's fresh batch
            data, state = crit.mix(v, t)
            loss = crit.train_loss(cls(vit(data)[0]), t, state)
        else:
            loss = cross_entropy(cls(vit(v)[0]), t)
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
    out = {"metric": "fine-tuning step (ViT-B/12^3, linear head, bf16, one MI355X), ms per step", "batch": B, "steps": steps, "warmup": warmup,
           "rounds": n_rounds}
    for on, name in ((False, "recipe_off"), (True, "recipe_on")):
        out[name] = {"ms_per_step": round(statistics.median(rounds[on]), 3), "rounds_ms": [round(r, 3) for r in rounds[on]],
                     "spread_pct": round(100 * (max(rounds[on]) - min(rounds[on])) / min(rounds[on]), 2)}
    out["recipe_cost_pct"] = round(100 * (out["recipe_on"]["ms_per_step"] / out["recipe_off"]["ms_per_step"] - 1), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="calls per timed round (kernel part) or steps per round (--step)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--step", action="store_true", help="time the fine-tuning step with the recipe off and on instead of the kernel alone")
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixup.py needs an MI355X: a timing off the GPU says nothing")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    if a.step:
        result = step_part(dev, a.batch, a.iters, a.warmup, a.rounds)
    else:
        result = {"metric": "hct_mix_volumes against the torch composition, in place (one MI355X), microseconds per call"}
        result.update(kernel_part(lib, dev, a.batch, 3, a.size, a.iters, a.warmup, a.rounds))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
