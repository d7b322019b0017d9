"""What multi-label fine-tuning costs on the HIP path.

  kernel   hct_sigmoid_bce, loss + label_loss + gradient in one call, alone at 64 x 14 (a fine-tuning batch over CQ500's labels) and
           4096 x 33: microseconds per call from HIP events around a window of back-to-back calls (warmed up; the window is long
           enough to time the device, not the enqueue), the in-library profile's time of one call, and the bytes the call has
           to move (logits and targets read twice -- loss pass and gradient pass --, the gradient written) against the HBM floor.
  step     the fine-tuning step of scripts/bench_dropout.py (ViT-B/12^3, 96^3 x 3 channels, B = 64, bf16, linear head) with
           `cross_entropy` on 2 classes against `bce_with_logits` on 14 labels.  Both are built once and timed in alternating blocks
           in one process; per loss the median block and the spread between its blocks are reported.  The claim under test: the two
           medians agree within the spread of the cross-entropy step across its own blocks.

  python scripts/bench_multilabel.py [--steps 10] [--warmup 3] [--rounds 5] [--parts kernel,step] [--out profiles/multilabel_bench.json]
Prints one JSON line.
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

from headct_foundation_amd import _lib  # noqa: E402
from headct_foundation_amd.classifier import LinearClassifier, bce_with_logits, cross_entropy  # noqa: E402
from headct_foundation_amd.data import SyntheticLabelled, SyntheticMultiLabelled  # noqa: E402
from headct_foundation_amd.dino_model import ViTBackbone  # noqa: E402
from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_  # noqa: E402

PROF_BCE = 9  # csrc/prof.h
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak


def kernel_part(lib, dev, calls: int) -> dict:
    out = {}
    for B, T in ((64, 14), (4096, 33)):
        g = torch.Generator(device=dev).manual_seed(B)
        x = 4 * torch.randn(B, T, device=dev, generator=g)
        y = (torch.rand(B, T, device=dev, generator=g) < 0.5).float()
        y.view(-1)[2::5] = -1.0
        w = 0.05 + 19.95 * torch.rand(T, device=dev, generator=g)
        loss, label_loss, dx = torch.empty(1, device=dev), torch.empty(T, device=dev), torch.empty_like(x)
        ws = torch.empty(lib.hct_sigmoid_bce_workspace_bytes(B, T), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def call():
            _lib.check(lib.hct_sigmoid_bce(x.data_ptr(), y.data_ptr(), w.data_ptr(), B, T, None, loss.data_ptr(), label_loss.data_ptr(),
                                           dx.data_ptr(), ws.data_ptr(), ws.numel(), st), "hct_sigmoid_bce")
        for _ in range(50):
            call()
        windows = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                call()
            b.record()
            b.synchronize()
            windows.append(a.elapsed_time(b) * 1e3 / calls)
        lib.hct_prof_reset()
        lib.hct_prof_enable(1 << PROF_BCE)
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        lib.hct_prof_enable(0)
        ms, n, work = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(lib.hct_prof_read(PROF_BCE, C.byref(ms), C.byref(n), C.byref(work)), "hct_prof_read")
        lib.hct_prof_reset()
        nbytes = B * T * 4 * (2 + 2 + 1) + 2 * T * 4  # x, y read by the loss pass and by the gradient pass; dlogits written; pos_weight
        out[f"{B}x{T}"] = {"us_per_call_back_to_back": round(statistics.median(windows), 2), "windows_us": [round(v, 2) for v in windows],
                           "calls_per_window": calls, "us_per_call_in_library_events": round(ms.value * 1e3 / max(1, n.value), 2),
                           "launches_per_call": 3, "bytes": nbytes, "hbm_floor_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 4)}
    return out


def finetune_case(kind: str, B: int, dev):
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=96, patch_size=12, hidden_size=768, mlp_dim=3072, num_layers=12, num_heads=12,
                      compute_dtype="bf16").to(dev).train()
    n_out = 2 if kind == "cross_entropy_2_classes" else 14
    cls = LinearClassifier(768, n_out, feature_grad=True).to(dev).train()
    opts = [HipAdamW(cls, lr=1.5e-1, weight_decay=0.04), HipAdamW(vit, lr=1.5e-3, weight_decay=0.04)]
    if n_out == 2:
        v, t, _ = SyntheticLabelled(1, B, 3, 96, 2, dev, seed=0).batches[0]
        criterion = cross_entropy
    else:
        v, t, _ = SyntheticMultiLabelled(1, B, 3, 96, 14, dev, seed=0).batches[0]
        criterion = bce_with_logits

    def step():
        for o in opts:
            o.zero_grad()
        loss = criterion(cls(vit(v)[0]), t)
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


def step_part(dev, steps: int, warmup: int, rounds: int) -> dict:
    kinds = ["cross_entropy_2_classes", "bce_with_logits_14_labels"]
    fns = {k: finetune_case(k, 64, dev) for k in kinds}
    for f in fns.values():
        for _ in range(warmup):
            f()
    blocks = {k: [] for k in kinds}
    for _ in range(rounds):  # alternate the two losses inside one process
        for k in kinds:
            blocks[k].append(timed(fns[k], steps))
    out = {"batch": 64, "steps_per_block": steps, "blocks": rounds}
    for k in kinds:
        out[k] = {"ms_per_step_median": round(statistics.median(blocks[k]), 3), "blocks_ms": [round(v, 3) for v in blocks[k]],
                  "spread_ms": round(max(blocks[k]) - min(blocks[k]), 3)}
    ce, ml = out[kinds[0]], out[kinds[1]]
    out["difference_ms"] = round(ml["ms_per_step_median"] - ce["ms_per_step_median"], 3)
    out["within_cross_entropy_spread"] = bool(abs(out["difference_ms"]) <= ce["spread_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000, help="back-to-back kernel calls per timed window")
    ap.add_argument("--parts", default="kernel,step")
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multilabel.py needs an MI355X: nothing here is measured on the CPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    result = {"metric": "multi-label fine-tuning (bf16, one MI355X)"}
    parts = [p for p in a.parts.split(",") if p]
    if "kernel" in parts:
        result["hct_sigmoid_bce"] = kernel_part(lib, dev, a.calls)
    if "step" in parts:
        result["finetune_step"] = step_part(dev, a.steps, a.warmup, a.rounds)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
