"""What segmentation fine-tuning costs on the HIP path.

  kernel   hct_seg_loss, forward + gradient in one call (stats, finalize, gradient), alone at ViT-B/12^3, 96^3, B = 64, bf16, K = 2 and
           K = 6: microseconds per call from HIP events around a window of back-to-back calls, beside the torch composition
           (un-patchify, fp32 log_softmax, one-hot, Dice and cross-entropy, autograd backward) in alternating windows of one process;
           the bytes the call has to move (logits read by the stats pass and by the gradient pass, the gradient written, the labels
           read twice) and the rate that is, against the 6.29 TB/s float4-copy floor the other benches quote.
  --step   the segmentation step (ViT-B/12^3, 96^3 x 3 channels, B = 64, bf16, SegmentationHead with K = 2, seg_loss with the
           gradient in place) against the classification fine-tuning step with the linear head on the same backbone and batch,
           alternating blocks in one process.

  python scripts/bench_seg.py [--step] [--batch 64] [--calls 20] [--rounds 3] [--out profiles/seg_bench.json]
Prints one JSON line.
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
from headct_foundation_amd.data import SyntheticLabelled, SyntheticSegmented  # noqa: E402
from headct_foundation_amd.dino_model import ViTBackbone  # noqa: E402
from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_  # noqa: E402
from headct_foundation_amd.segmentation import SegmentationHead, seg_loss  # noqa: E402

COPY_FLOOR_BYTES_PER_S = 6.29e12  # float4 copy on one MI355X, as scripts/bench_ibot.py quotes it
EPS = 1e-5


def torch_composition(logits, labels, first, G, P, K):
    """The loss composed in torch: what a port without the kernel would run."""
    B = logits.shape[0]
    x = logits[:, first:first + G ** 3].reshape(B, G, G, G, K, P, P, P).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(B, K, G * P, G * P, G * P).float()
    y = labels.long()
    valid = y < K
    oh = torch.nn.functional.one_hot(torch.where(valid, y, torch.zeros_like(y)), K).movedim(-1, 1).float() * valid.unsqueeze(1)
    logp = torch.log_softmax(x, dim=1)
    ce = -(logp * oh).sum() / valid.sum().clamp_min(1)
    p = logp.exp() * valid.unsqueeze(1)
    I, Pc, Y = (p * oh).flatten(2).sum(2), p.flatten(2).sum(2), oh.flatten(2).sum(2)
    return ce + (1 - (2 * I + EPS) / (Pc + Y + EPS)).mean()


def window(fn, calls: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def kernel_part(lib, dev, B: int, calls: int, rounds: int) -> dict:
    out = {}
    P, G, first = 12, 8, 1
    T, S = first + G ** 3, G * P
    for K in (2, 6):
        N = K * P ** 3
        g = torch.Generator(device=dev).manual_seed(K)
        logits = (2 * torch.randn(B, T, N, device=dev, generator=g)).to(torch.bfloat16)
        labels = torch.randint(0, K, (B, S, S, S), device=dev, generator=g).to(torch.uint8)
        labels[torch.rand(B, S, S, S, device=dev, generator=g) < 0.02] = 255
        dl = torch.empty_like(logits)
        loss = torch.empty(1, device=dev)
        ws = torch.empty(lib.hct_seg_loss_workspace_bytes(B, G, P, K), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def hip():
            _lib.check(lib.hct_seg_loss(logits.data_ptr(), _lib.HCT_BF16, N, labels.data_ptr(), None, B, T, first, G, P, K, 1.0, 1.0, None,
                                        loss.data_ptr(), None, None, None, dl.data_ptr(), N, 0, ws.data_ptr(), ws.numel(), st), "hct_seg_loss")
        leaf = logits.clone().requires_grad_(True)

        def composed():
            leaf.grad = None
            torch_composition(leaf, labels, first, G, P, K).backward()
        for _ in range(3):
            hip()
        composed()
        torch.cuda.synchronize()
        w_hip, w_torch = [], []
        for _ in range(rounds):  # alternate the two in one process
            w_hip.append(window(hip, calls))
            w_torch.append(window(composed, max(1, calls // 10)))
        hip()
        composed()
        torch.cuda.synchronize()
        voxels = B * S ** 3
        nbytes = 3 * voxels * K * 2 + 2 * voxels + B * first * N * 2  # logits twice in, gradient once out, labels twice, the zeroed leading rows
        us = statistics.median(w_hip)
        out[f"K{K}"] = {"us_per_call": round(us, 1), "windows_us": [round(v, 1) for v in w_hip], "calls_per_window": calls,
                        "torch_composition_us": round(statistics.median(w_torch), 1), "torch_windows_us": [round(v, 1) for v in w_torch],
                        "speedup": round(statistics.median(w_torch) / us, 2), "bytes": nbytes, "TB_per_s": round(nbytes / us * 1e-6, 3),
                        "share_of_copy_floor": round(nbytes / us * 1e6 / COPY_FLOOR_BYTES_PER_S, 3),
                        "loss_hip": round(float(loss), 6), "loss_torch": round(float(torch_composition(leaf.detach(), labels, first, G, P, K)), 6),
                        "grad_rel_diff": round(float((dl.float() - leaf.grad.float()).norm() / leaf.grad.float().norm()), 5)}
        del logits, labels, dl, leaf
        torch.cuda.empty_cache()
    return {"shape": f"ViT-B/12^3, 96^3, B {B}, bf16", **out}


def step_part(dev, B: int, steps: int, warmup: int, rounds: int) -> dict:
    def case(kind):
        torch.manual_seed(0)
        vit = ViTBackbone(in_chans=3, img_size=96, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12,
                          compute_dtype="bf16").to(dev).train()
        if kind == "segmentation_K2":
            head = SegmentationHead(768, 12, 2).to(dev).train()
            v, t, _ = SyntheticSegmented(1, B, 3, 96, 2, dev, seed=0).batches[0]
            crit = lambda tok: seg_loss(head(tok), t, 12, 2, 1, inplace_grad=True)
        else:
            head = LinearClassifier(768, 2, feature_grad=True).to(dev).train()
            v, t, _ = SyntheticLabelled(1, B, 3, 96, 2, dev, seed=0).batches[0]
            crit = lambda tok: cross_entropy(head(tok), t)
        opts = [HipAdamW(head, lr=1.5e-1, weight_decay=0.04), HipAdamW(vit, lr=1.5e-3, weight_decay=0.04)]

        def step():
            for o in opts:
                o.zero_grad()
            loss = crit(vit(v)[0])
            loss.backward()
            clip_grad_norm_(head, 1.0)
            clip_grad_norm_(vit, 1.0)
            for o in opts:
                o.step()
            return loss
        return step

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        if not torch.isfinite(loss.detach()):
            raise SystemExit("non-finite loss")
        return (time.perf_counter() - t0) * 1e3 / steps
    kinds = ["classification_linear_head", "segmentation_K2"]
    fns = {k: case(k) for k in kinds}
    for f in fns.values():
        for _ in range(warmup):
            f()
    blocks = {k: [] for k in kinds}
    for _ in range(rounds):
        for k in kinds:
            blocks[k].append(timed(fns[k]))
    out = {"batch": B, "steps_per_block": steps, "blocks": rounds}
    for k in kinds:
        out[k] = {"ms_per_step_median": round(statistics.median(blocks[k]), 3), "blocks_ms": [round(v, 3) for v in blocks[k]]}
    out["difference_ms"] = round(out[kinds[1]]["ms_per_step_median"] - out[kinds[0]]["ms_per_step_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="also time the segmentation step against the classification step")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg.py needs an MI355X: nothing here is measured on the CPU")
    dev = torch.device("cuda:0")
    result = {"metric": "segmentation fine-tuning (bf16, one MI355X)", "hct_seg_loss": kernel_part(_lib.load(), dev, a.batch, a.calls, a.rounds)}
    if a.step:
        result["finetune_step"] = step_part(dev, a.batch, a.steps, a.warmup, a.rounds)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
