"""The bench.py workload (ViT-B/16^3, 96^3, mask 0.75, B = 256, bf16, one GPU) with `norm_layer=RMSNorm` (or `--norm layernorm`),
set up, warmed up and timed the way bench.py does: reference init at seed 42, four pooled volumes, zero_grad / forward / backward /
per-tensor clip / HipAdamW / cosine LR per step, wall time between two device fences.  Prints one JSON line.

    python scripts/bench_rmsnorm.py [--norm rmsnorm|layernorm] [--steps 20] [--warmup 5] [--batch 256]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import WORKLOADS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--norm", default="rmsnorm", choices=["rmsnorm", "layernorm"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--config", default="vitb", choices=sorted(WORKLOADS))
    args = ap.parse_args()
    from headct_foundation_amd import MaskedAutoencoderViT, RMSNorm
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    from headct_foundation_amd.optim import HipAdamW, clip_gradients
    if not torch.cuda.is_available():
        raise SystemExit("bench_rmsnorm.py needs an MI355X: the HIP hot path has no CPU fallback")
    device = torch.device("cuda", 0)
    arch, default_batch, workload, _ = WORKLOADS[args.config]
    B, S = args.batch or default_batch, arch["input_size"]
    torch.manual_seed(42)
    model = MaskedAutoencoderViT(**arch, norm_layer=RMSNorm if args.norm == "rmsnorm" else nn.LayerNorm, compute_dtype="bf16").to(device)
    total_steps = max(1000, args.steps + args.warmup)
    base_lr = 1.5e-4 * B / 256
    opt = HipAdamW(model, lr=base_lr, weight_decay=5e-3, betas=(0.9, 0.95))
    sched = get_cosine_schedule_with_warmup(opt, int(0.05 * total_steps), total_steps, lr_end=base_lr * 1e-3)
    torch.manual_seed(42)
    pool = [torch.rand(B, 1, S, S, S, device=device) for _ in range(4)]
    losses = torch.zeros(args.steps + args.warmup, device=device)

    def step(i):
        opt.zero_grad()
        loss, _, _ = model(pool[i % 4])
        loss.backward()
        clip_gradients(model, 3.0)
        opt.step()
        sched.step()
        losses[i] = loss.detach()

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, args.warmup + args.steps):
        step(i)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    lv = losses.cpu()
    if not torch.isfinite(lv).all():
        raise SystemExit(f"non-finite loss: {lv.tolist()}")
    print(json.dumps({"norm_layer": args.norm, "workload": workload, "per_gpu_batch": B, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(elapsed / args.steps * 1e3, 3), "value": round(B * args.steps / elapsed, 2), "unit": "CT-volumes/s",
                      "loss_first": round(float(lv[0]), 5), "loss_last": round(float(lv[-1]), 5)}), flush=True)


if __name__ == "__main__":
    main()
