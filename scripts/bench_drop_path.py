"""What stochastic depth (drop path) costs on the HIP path: the fine-tuning step of scripts/bench_finetune.py's ViT-B/12^3 case (linear
head, 96^3 x 3 channels, 513 tokens, B = 64, bf16) at VIT.DROP_PATH_RATE 0 and 0.1, built once and timed in alternating rounds (one
machine state for both); per rate the median round and the spread between rounds, plus the time of the streaming passes from the
in-library profile.  Then the streaming pass alone, hct_residual_drop_apply on [64 * 513, 768] (bf16 in, fp32 residual and output, the
forward's form): microseconds, GB/s and the share of the HBM floor.  Prints one JSON line.

  python scripts/bench_drop_path.py [--steps 10] [--warmup 3] [--rounds 3] [--rates 0,0.1] [--out profiles/drop_path_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from headct_foundation_amd import _lib, dropout  # noqa: E402
from headct_foundation_amd.classifier import LinearClassifier, cross_entropy  # noqa: E402
from headct_foundation_amd.data import SyntheticLabelled  # noqa: E402
from headct_foundation_amd.dino_model import ViTBackbone  # noqa: E402
from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_  # noqa: E402

PROF_DROPOUT = 8       # csrc/prof.h
HBM_GBS = 8000.0       # MI355X peak HBM bandwidth, GB/s: the floor of a streaming pass is its bytes over this


def finetune_case(rate: float, B: int, dev):
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=96, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12,
                      drop_path_rate=rate, compute_dtype="bf16").to(dev).train()
    cls = LinearClassifier(768, 2, feature_grad=True).to(dev).train()
    opts = [HipAdamW(cls, lr=1.5e-1, weight_decay=0.04), HipAdamW(vit, lr=1.5e-3, weight_decay=0.04)]
    v, t, _ = SyntheticLabelled(1, B, 3, 96, 2, dev, seed=0).batches[0]

    def step():
        for o in opts:
            o.zero_grad()
        loss = cross_entropy(cls(vit(v)[0]), t)
        loss.backward()
        clip_grad_norm_(cls, 1.0)
        clip_grad_norm_(vit, 1.0)
        for o in opts:
            o.step()
        return loss
    return step


def timed(step, steps: int) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    if not torch.isfinite(loss.detach()):
        raise SystemExit("non-finite loss")
    return (time.perf_counter() - t0) * 1e3 / steps


def streaming_ms(lib, step):
    """(ms, launches) of the streaming passes over one profiled step (HIP events around every launch of the class)."""
    lib.hct_prof_reset()
    lib.hct_prof_enable(1 << PROF_DROPOUT)
    step()
    torch.cuda.synchronize()
    lib.hct_prof_enable(0)
    ms, n, w = C.c_double(), C.c_int64(), C.c_double()
    _lib.check(lib.hct_prof_read(PROF_DROPOUT, C.byref(ms), C.byref(n), C.byref(w)), "hct_prof_read")
    lib.hct_prof_reset()
    return round(ms.value, 3), int(n.value)


def pass_alone(lib, dev, B: int = 64, N: int = 513, d: int = 768, iters: int = 50) -> dict:
    """y (fp32) = x (bf16) * s_b + residual (fp32) on [B * N, d] at element rate 0: 2 + 4 + 4 bytes per element."""
    x = torch.randn(B, N, d, device=dev).bfloat16()
    res = torch.randn(B, N, d, device=dev)
    y = torch.empty_like(res)
    scales = dropout.path_scales(1234, [dropout.path_site(6, 0)], [0.1], B, device=dev)[0].contiguous()
    st = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(lib.hct_residual_drop_apply(x.data_ptr(), _lib.HCT_BF16, y.data_ptr(), _lib.HCT_F32, res.data_ptr(), B, N * d, scales.data_ptr(),
                                               1234, dropout.path_site(6, 0), 0.0, st), "hct_residual_drop_apply")
    for _ in range(5):
        call()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    us = ev[0].elapsed_time(ev[1]) * 1e3 / iters
    nbytes = x.numel() * 10
    gbs = nbytes / us / 1e3
    return {"shape": [B * N, d], "us": round(us, 2), "GB_per_s": round(gbs, 1), "bytes": nbytes, "hbm_floor_us": round(nbytes / HBM_GBS / 1e3, 2),
            "share_of_hbm_floor_pct": round(100 * gbs / HBM_GBS, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rates", default="0,0.1")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rates = [float(r) for r in a.rates.split(",")]
    result = {"metric": "fine-tuning step with drop path (ViT-B/12^3, bf16, one MI355X), ms per step", "steps": a.steps, "warmup": a.warmup,
              "rounds": a.rounds, "batch": a.batch}
    steps = {r: finetune_case(r, a.batch, dev) for r in rates}
    for s in steps.values():
        for _ in range(a.warmup):
            s()
    rounds = {r: [] for r in rates}
    for _ in range(a.rounds):  # alternate the rates inside one session
        for r in rates:
            rounds[r].append(timed(steps[r], a.steps))
    for r in rates:
        ms, n = streaming_ms(lib, steps[r])
        result[f"rate_{r:g}"] = {"ms_per_step": round(statistics.median(rounds[r]), 3), "rounds_ms": [round(v, 3) for v in rounds[r]],
                                 "spread_pct": round(100 * (max(rounds[r]) - min(rounds[r])) / min(rounds[r]), 2),
                                 "streaming_ms": ms, "streaming_launches": n}
    if 0.0 in rates:
        base = result["rate_0"]["ms_per_step"]
        for r in rates:
            if r:
                result[f"rate_{r:g}"]["cost_pct_of_rate_0"] = round(100 * (result[f"rate_{r:g}"]["ms_per_step"] / base - 1), 2)
    del steps
    torch.cuda.empty_cache()
    result["pass_alone"] = pass_alone(lib, dev)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
