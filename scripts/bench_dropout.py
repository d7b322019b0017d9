"""What dropout costs on the HIP path: the fine-tuning step of scripts/bench_finetune.py's ViT-B/12^3 case (linear head, 96^3 x 3
channels, 513 tokens, B = 64, bf16) and the MAE ViT-B step of bench.py (96^3, patch 16, B = 256, bf16), each at dropout rate 0 and
0.1.  The cases are built once and then timed in alternating rounds (one machine state for all of them); per case the median round
and the spread between rounds are reported, plus the time of the dropout kernels themselves from the in-library profile (streaming
passes; the attention launches are those of the general kernels with the mask).  Prints one JSON line.

  python scripts/bench_dropout.py [--steps 10] [--warmup 3] [--rounds 3] [--cases finetune,mae] [--out profiles/dropout_bench.json]
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

from headct_foundation_amd import MaskedAutoencoderViT, _lib  # noqa: E402
from headct_foundation_amd.classifier import LinearClassifier, cross_entropy  # noqa: E402
from headct_foundation_amd.data import SyntheticLabelled  # noqa: E402
from headct_foundation_amd.dino_model import ViTBackbone  # noqa: E402
from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_, clip_gradients  # noqa: E402

PROF_ATTN_FWD, PROF_ATTN_BWD, PROF_DROPOUT = 3, 4, 8  # csrc/prof.h


def finetune_case(rate: float, B: int, dev):
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=96, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12,
                      dropout_rate=rate, compute_dtype="bf16").to(dev).train()
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


def mae_case(rate: float, B: int, dev):
    torch.manual_seed(42)
    m = MaskedAutoencoderViT(input_size=96, patch_size=16, mask_ratio=0.75, pos_embed="sincos", dropout_rate=rate, compute_dtype="bf16").to(dev).train()
    opt = HipAdamW(m, lr=1.5e-4 * B / 256, weight_decay=5e-3, betas=(0.9, 0.95))
    pool = [torch.rand(B, 1, 96, 96, 96, device=dev) for _ in range(2)]
    i = [0]

    def step():
        opt.zero_grad()
        loss, _, _ = m(pool[i[0] % 2])
        i[0] += 1
        loss.backward()
        clip_gradients(m, 3.0)
        opt.step()
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


def kernel_ms(lib, step, ids) -> dict:
    """Per-step time of the kernel classes `ids` over one profiled step (HIP events around every launch of the class)."""
    lib.hct_prof_reset()
    lib.hct_prof_enable(sum(1 << i for i in ids))
    step()
    torch.cuda.synchronize()
    lib.hct_prof_enable(0)
    out = {}
    for i in ids:
        ms, n, w = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(lib.hct_prof_read(i, C.byref(ms), C.byref(n), C.byref(w)), "hct_prof_read")
        out[i] = (round(ms.value, 3), int(n.value))
    lib.hct_prof_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="finetune,mae")
    ap.add_argument("--rates", default="0,0.1")
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rates = [float(r) for r in a.rates.split(",")]
    builders = {"finetune": (finetune_case, 64), "mae": (mae_case, 256)}
    result = {"metric": "training step with dropout (bf16, one MI355X), ms per step", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "cases": {}}
    for name in [c for c in a.cases.split(",") if c]:
        build, B = builders[name]
        steps = {r: build(r, B, dev) for r in rates}
        for s in steps.values():
            for _ in range(a.warmup):
                s()
        rounds = {r: [] for r in rates}
        for _ in range(a.rounds):  # alternate the rates inside one session
            for r in rates:
                rounds[r].append(timed(steps[r], a.steps))
        entry = {"batch": B}
        for r in rates:
            k = kernel_ms(lib, steps[r], (PROF_ATTN_FWD, PROF_ATTN_BWD, PROF_DROPOUT))
            entry[f"rate_{r:g}"] = {"ms_per_step": round(statistics.median(rounds[r]), 3), "rounds_ms": [round(v, 3) for v in rounds[r]],
                                    "spread_pct": round(100 * (max(rounds[r]) - min(rounds[r])) / min(rounds[r]), 2),
                                    "attention_fwd_ms": k[PROF_ATTN_FWD][0], "attention_bwd_ms": k[PROF_ATTN_BWD][0],
                                    "dropout_streaming_ms": k[PROF_DROPOUT][0], "dropout_streaming_launches": k[PROF_DROPOUT][1]}
        if 0.0 in rates and len(rates) > 1:
            base = entry["rate_0"]["ms_per_step"]
            for r in rates:
                if r:
                    entry[f"rate_{r:g}"]["cost_pct_of_rate_0"] = round(100 * (entry[f"rate_{r:g}"]["ms_per_step"] / base - 1), 2)
        result["cases"][name] = entry
        del steps
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
