"""Downstream fine-tuning step on the HIP path: ViT-B/12^3 on 96^3 x 3 channels (513 tokens), B = 64, bf16 -- the reference's
downstream launch settings (--classifier linear|attentive --grad_clip 1.0 --batch_size 64).  One step = zero_grad, backbone
forward (under no_grad with LOCK), head forward, cross_entropy, backward, clip_grad_norm_ of the head (and of the backbone
without LOCK), HipAdamW step(s).  Prints one JSON line: ms per step and volumes/s for {linear, attentive} x {LOCK off, on} and for
LoRA fine-tuning (TRAIN.LORA: rank-128 adapters on q and v, the block matrices frozen) with both heads.

  python scripts/bench_finetune.py [--steps 10] [--warmup 3] [--batch 64] [--cases linear_lora,linear]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from headct_foundation_amd.classifier import AttentionClassifier, LinearClassifier, cross_entropy  # noqa: E402
from headct_foundation_amd.data import SyntheticLabelled  # noqa: E402
from headct_foundation_amd.dino_model import ViTBackbone  # noqa: E402
from headct_foundation_amd.misc import set_requires_grad_false  # noqa: E402
from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_  # noqa: E402


def run(head: str, lock: bool, B: int, steps: int, warmup: int, dev, lora: bool = False) -> float:
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=96, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12,
                      lora=lora, compute_dtype="bf16").to(dev)
    cls = (LinearClassifier(768, 2, feature_grad=not lock) if head == "linear" else
           AttentionClassifier(768, 2, num_heads=12, num_queries=1, compute_dtype="bf16")).to(dev).train()
    if lock:
        for p in vit.parameters():
            p.requires_grad_(False)
    if lora:
        set_requires_grad_false(vit, lora=True)
        with torch.no_grad():  # adapters that do something (B = 0 at init makes dA an exact zero)
            for n, p in vit.named_parameters():
                if n.endswith("lora_matrix_B"):
                    p.normal_(std=0.005)
        vit.mark_weights_updated()
    opts = [HipAdamW(cls, lr=1.5e-1, weight_decay=0.04)] + ([] if lock else [HipAdamW(vit, lr=1.5e-3, weight_decay=0.04)])
    v, t, _ = SyntheticLabelled(1, B, 3, 96, 2, dev, seed=0).batches[0]

    def step():
        for o in opts:
            o.zero_grad()
        if lock:
            with torch.no_grad():
                tok = vit(v)[0]
        else:
            tok = vit(v)[0]
        loss = cross_entropy(cls(tok), t)
        loss.backward()
        clip_grad_norm_(cls, 1.0)
        if not lock:
            clip_grad_norm_(vit, 1.0)
        for o in opts:
            o.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    if not torch.isfinite(loss.detach()):
        raise SystemExit(f"non-finite loss ({head}, lock={lock})")
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--cases", default="", help="comma-separated subset of the cases (default: all six), e.g. for a kernel trace of one")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = {}
    todo = [(f"{head}{'_lock' if lock else ''}", head, lock, False) for head in ("linear", "attentive") for lock in (False, True)]
    todo += [(f"{head}_lora", head, False, True) for head in ("linear", "attentive")]
    want = [c for c in a.cases.split(",") if c]
    if set(want) - {n for n, *_ in todo}:
        raise SystemExit(f"unknown case(s) {sorted(set(want) - {n for n, *_ in todo})}; known: {[n for n, *_ in todo]}")
    for name, head, lock, lora in todo:
        if want and name not in want:
            continue
        ms = run(head, lock, a.batch, a.steps, a.warmup, dev, lora=lora)
        cases[name] = {"ms_per_step": round(ms, 3), "volumes_per_s": round(a.batch * 1e3 / ms, 1)}
    print(json.dumps({"metric": "downstream fine-tuning step (ViT-B/12^3, 96^3 x 3ch, 513 tokens, bf16)", "batch": a.batch,
                      "steps": a.steps, "warmup": a.warmup, "cases": cases}))


if __name__ == "__main__":
    main()
