"""What patch dropout saves on the HIP path: the fine-tuning step of scripts/bench_finetune.py's ViT-B/12^3 case (linear head, 96^3 x 3
channels, L = 512 patches, B = 64, bf16) at VIT.PATCH_DROPOUT 0, 0.25, 0.5 and 0.75 (513, 385, 257 and 129 tokens per sample), built once
and timed in alternating rounds (one machine state for all rates); per rate the median round, the spread between rounds and the ratio to
rate 0 of the same process.  Then the two assembly kernels alone, hct_vit_assemble_keep_fwd / _bwd at each rate's shape (bf16 tokens,
every gradient written): microseconds and GB/s.  Prints one JSON line.

  python scripts/bench_patch_dropout.py [--steps 10] [--warmup 3] [--rounds 3] [--rates 0,0.25,0.5,0.75] [--out profiles/patch_dropout_bench.json]
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
from headct_foundation_amd.dropout import patch_keep_count  # noqa: E402
from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_  # noqa: E402


def finetune_case(rate: float, B: int, dev):
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=96, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12,
                      patch_dropout=rate, compute_dtype="bf16").to(dev).train()
    cls = LinearClassifier(768, 2, feature_grad=True).to(dev).train()
    opts = [HipAdamW(cls, lr=1.5e-1, weight_decay=0.04), HipAdamW(vit, lr=1.5e-3, weight_decay=0.04)]
    v, t, _ = SyntheticLabelled(1, B, 3, 96, 2, dev, seed=0).batches[0]

    def step():
        for o in opts:
            o.zero_grad()
        loss = cross_entropy(cls(vit(v)[0]), t)  # (noise: the default draw, as a training run makes it)
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


def assemble_alone(lib, dev, K: int, B: int = 64, L: int = 512, D: int = 768, iters: int = 50) -> dict:
    """The two kernels at [B, 1 + K, D]: forward reads bf16 tokens and fp32 position rows and writes fp32; backward reads the fp32 gradient
    once for dtok and once more (the kept rows, through the ids) for the three sums."""
    tok = torch.randn(B * K, D, device=dev).bfloat16()
    cls, pos = torch.randn(D, device=dev), torch.randn(L, D, device=dev)
    ids_shuffle = torch.stack([torch.randperm(L, device=dev) for _ in range(B)]).to(torch.int32).contiguous()
    ids_restore = torch.argsort(ids_shuffle.long(), dim=1).to(torch.int32).contiguous()
    h0 = torch.empty(B, 1 + K, D, device=dev)
    dtok, dcls, dpos = torch.empty_like(tok), torch.empty_like(cls), torch.empty_like(pos)
    st = torch.cuda.current_stream().cuda_stream

    def fwd():
        _lib.check(lib.hct_vit_assemble_keep_fwd(tok.data_ptr(), _lib.HCT_BF16, cls.data_ptr(), None, pos.data_ptr(), ids_shuffle.data_ptr(), B, L, K, 0, D,
                                                 h0.data_ptr(), st), "hct_vit_assemble_keep_fwd")

    def bwd():
        _lib.check(lib.hct_vit_assemble_keep_bwd(h0.data_ptr(), ids_restore.data_ptr(), B, L, K, 0, D, dtok.data_ptr(), _lib.HCT_BF16, dcls.data_ptr(), None,
                                                 dpos.data_ptr(), st), "hct_vit_assemble_keep_bwd")
    out = {"rows": B * (1 + K)}
    n = B * K * D
    for name, call, nbytes in (("fwd", fwd, n * (2 + 4 + 4)), ("bwd", bwd, n * (4 + 2) + n * 4 + L * D * 4)):
        for _ in range(5):
            call()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(iters):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        us = ev[0].elapsed_time(ev[1]) * 1e3 / iters
        out[name] = {"us": round(us, 2), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rates", default="0,0.25,0.5,0.75")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rates = [float(r) for r in a.rates.split(",")]
    result = {"metric": "fine-tuning step with patch dropout (ViT-B/12^3, 96^3, linear head, bf16, one MI355X), ms per step", "steps": a.steps,
              "warmup": a.warmup, "rounds": a.rounds, "batch": a.batch}
    steps = {r: finetune_case(r, a.batch, dev) for r in rates}
    for s in steps.values():
        for _ in range(a.warmup):
            s()
    rounds = {r: [] for r in rates}
    for _ in range(a.rounds):  # alternate the rates inside one session
        for r in rates:
            rounds[r].append(timed(steps[r], a.steps))
    for r in rates:
        K = patch_keep_count(512, r)
        result[f"rate_{r:g}"] = {"keep": K, "tokens_per_sample": 1 + K, "ms_per_step": round(statistics.median(rounds[r]), 3),
                                 "rounds_ms": [round(v, 3) for v in rounds[r]],
                                 "spread_pct": round(100 * (max(rounds[r]) - min(rounds[r])) / min(rounds[r]), 2)}
    if 0.0 in rates:
        base = result["rate_0"]["ms_per_step"]
        for r in rates:
            if r:
                result[f"rate_{r:g}"]["ratio_to_rate_0"] = round(result[f"rate_{r:g}"]["ms_per_step"] / base, 4)
    del steps
    torch.cuda.empty_cache()
    for r in rates:
        if r:
            result[f"rate_{r:g}"]["assemble_alone"] = assemble_alone(lib, dev, patch_keep_count(512, r), a.batch)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
