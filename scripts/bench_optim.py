"""The optimizer pass of the bench.py workload (ViT-B/16^3 MAE, 149 M parameters in one flat buffer), alone and inside the full step.

    python scripts/bench_optim.py --mode kernels [--reps 5] [--iters 20]
        hct_adamw_step / hct_lion_step / hct_sgd_step / hct_lamb_step (and hct_grad_norms, the reduction yardstick) on the model's
        own segment table: clip coefficient pending (all 1: nothing is clipped, so no gradient is written back), bf16 shadow on,
        inputs rotated over two sets of buffers, HIP events around `iters` launches, `reps` repeats alternated between the kernels.
        One JSON line: microseconds (median and spread of the repeats) and achieved GB/s from the streams' byte counts per element
        (AdamW 30, Lion / SGD 22, Lamb 42, the norm pass 4).
    python scripts/bench_optim.py --mode kernels --scaled [--reps 9] [--iters 20]
        the same, plus each `_scaled` entry point with layer decay 0.75 on the encoder blocks and the no-decay set as its
        per-segment scales, alternated with the unscaled entry point in the same process.  Both move the same bytes (the scaled
        one reads up to two more floats per 1024-element block); per kernel the line adds the scaled timing, the difference of the
        medians and the spread (max - min) of the unscaled timing over its own repeats, which is what that difference is read
        against.
    python scripts/bench_optim.py --mode kernels --counts [--reps 9] [--iters 20]
        AdamW only: hct_adamw_step (one step count for all segments, the launch of a run whose parameters have all had the same
        number of updates) alternated with hct_adamw_step_counts on the same buffers, the counts mixed (every third segment three
        updates behind, as a layer thawed late would be).  Same bytes plus one int per block and two pow() per thread; the line
        gives both timings, the difference of the medians and the spread of the uniform launch over its own repeats.
    python scripts/bench_optim.py --mode step --optimizer AdamW|Lion|SGD|Lamb [--steps 20] [--warmup 5]
        the bench.py step (reference init at seed 42, four pooled volumes, zero_grad / forward / backward / per-tensor clip /
        optimizer / cosine LR, wall time between two device fences) built with that optimizer.  One JSON line.

Run the modes as separate processes, one after another.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import WORKLOADS  # noqa: E402

BYTES = {"adamw": 30, "lion": 22, "sgd": 22, "lamb": 42, "grad_norms": 4}
STEP_LR = {"AdamW": 1.5e-4, "Lion": 1.5e-5, "SGD": 1.5e-2, "Lamb": 1.5e-3}  # per 256 volumes


def kernels(args):
    from headct_foundation_amd import MaskedAutoencoderViT, _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    arch = WORKLOADS["vitb"][0]
    torch.manual_seed(42)
    model = MaskedAutoencoderViT(**arch, compute_dtype="bf16").to(dev)
    names, seg = model.flat_segments()
    nseg, total = len(names), seg[-1]
    seg_t = torch.tensor(seg, dtype=torch.int64, device=dev)
    skip = torch.zeros(nseg, dtype=torch.uint8, device=dev)
    coef = torch.ones(nseg, dtype=torch.float32, device=dev)
    norms = torch.empty(nseg, dtype=torch.float32, device=dev)
    diag = [torch.empty(nseg, dtype=torch.float32, device=dev) for _ in range(3)]
    ws = torch.empty(lib.hct_grad_norms_workspace_bytes(total), dtype=torch.uint8, device=dev)
    lws = torch.empty(lib.hct_lamb_workspace_bytes(total, nseg), dtype=torch.uint8, device=dev)
    nset = 2
    sets = []
    for _ in range(nset):
        p = model._flat.clone()
        g = torch.randn(total, device=dev) * 1e-4  # per-tensor norms far below the clip
        sets.append(dict(p=p, g=g, m=torch.zeros(total, device=dev), v=torch.zeros(total, device=dev), sh=torch.empty(total, dtype=torch.bfloat16, device=dev)))
    if args.scaled:
        from headct_foundation_amd.param_scales import no_decay_scales, vit_layer_id
        depth = 1 + max(int(n.split(".")[1]) for n in names if n.startswith("blocks."))
        undecayed = no_decay_scales(model)
        lr_s = torch.tensor([0.75 ** (depth + 1 - vit_layer_id(n, depth)) for n in names], dtype=torch.float32, device=dev)
        wd_s = torch.tensor([0.0 if n in undecayed else 1.0 for n in names], dtype=torch.float32, device=dev)
    del model
    st = torch.cuda.current_stream().cuda_stream
    d = lambda t: t.data_ptr()
    step = [0]

    def adamw(i):
        s = sets[i % nset]
        step[0] += 1
        return lib.hct_adamw_step(d(s["p"]), d(s["g"]), d(s["m"]), d(s["v"]), d(seg_t), d(coef), d(skip), nseg, total, 1.5e-4, 0.9, 0.95, 1e-8, 5e-3, step[0], d(s["sh"]), st)

    def lion(i):
        s = sets[i % nset]
        return lib.hct_lion_step(d(s["p"]), d(s["g"]), d(s["m"]), d(seg_t), d(coef), d(skip), nseg, total, 1.5e-5, 0.9, 0.95, 5e-3, d(s["sh"]), st)

    def sgd(i):
        s = sets[i % nset]
        return lib.hct_sgd_step(d(s["p"]), d(s["g"]), d(s["m"]), d(seg_t), d(coef), d(skip), nseg, total, 1.5e-2, 0.9, d(s["sh"]), st)

    def lamb(i):
        s = sets[i % nset]
        return lib.hct_lamb_step(d(s["p"]), d(s["g"]), d(s["m"]), d(s["v"]), d(seg_t), d(coef), d(skip), nseg, total, 1.5e-3, 0.9, 0.95, 1e-6, 5e-3,
                                 d(diag[0]), d(diag[1]), d(diag[2]), d(lws), lws.numel(), d(s["sh"]), st)

    def grad_norms(i):
        s = sets[i % nset]
        return lib.hct_grad_norms(d(s["g"]), d(seg_t), nseg, total, 3.0, 0, d(norms), d(coef), d(ws), ws.numel(), st)

    def adamw_scaled(i):
        s = sets[i % nset]
        step[0] += 1
        return lib.hct_adamw_step_scaled(d(s["p"]), d(s["g"]), d(s["m"]), d(s["v"]), d(seg_t), d(coef), d(skip), nseg, total, 1.5e-4, 0.9, 0.95, 1e-8, 5e-3,
                                         step[0], d(s["sh"]), d(lr_s), d(wd_s), st)

    def lion_scaled(i):
        s = sets[i % nset]
        return lib.hct_lion_step_scaled(d(s["p"]), d(s["g"]), d(s["m"]), d(seg_t), d(coef), d(skip), nseg, total, 1.5e-5, 0.9, 0.95, 5e-3, d(s["sh"]),
                                        d(lr_s), d(wd_s), st)

    def sgd_scaled(i):
        s = sets[i % nset]
        return lib.hct_sgd_step_scaled(d(s["p"]), d(s["g"]), d(s["m"]), d(seg_t), d(coef), d(skip), nseg, total, 1.5e-2, 0.9, d(s["sh"]), d(lr_s), st)

    def lamb_scaled(i):
        s = sets[i % nset]
        return lib.hct_lamb_step_scaled(d(s["p"]), d(s["g"]), d(s["m"]), d(s["v"]), d(seg_t), d(coef), d(skip), nseg, total, 1.5e-3, 0.9, 0.95, 1e-6, 5e-3,
                                        d(diag[0]), d(diag[1]), d(diag[2]), d(lws), lws.numel(), d(s["sh"]), d(lr_s), d(wd_s), st)

    counts_t = torch.tensor([1 if i % 3 == 0 else 4 for i in range(nseg)], dtype=torch.int32, device=dev)

    def adamw_counts(i):
        s = sets[i % nset]
        counts_t.add_(1)  # in stream, as HipAdamW keeps its device counts current: part of what the mixed launch costs
        return lib.hct_adamw_step_counts(d(s["p"]), d(s["g"]), d(s["m"]), d(s["v"]), d(seg_t), d(coef), d(skip), nseg, total, 1.5e-4, 0.9, 0.95, 1e-8, 5e-3,
                                         d(counts_t), d(s["sh"]), None, None, st)

    calls = {"grad_norms": grad_norms, "adamw": adamw, "lion": lion, "sgd": sgd, "lamb": lamb}
    if args.counts:
        calls = {"adamw": adamw, "adamw_counts": adamw_counts}
    elif args.scaled:  # each scaled call right after its unscaled twin
        calls = {"grad_norms": grad_norms, "adamw": adamw, "adamw_scaled": adamw_scaled, "lion": lion, "lion_scaled": lion_scaled, "sgd": sgd,
                 "sgd_scaled": sgd_scaled, "lamb": lamb, "lamb_scaled": lamb_scaled}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters * 1e3

    for name, fn in calls.items():
        _lib.check(fn(0), name)
        for i in range(4):
            fn(i)
    torch.cuda.synchronize()
    assert float(coef.min()) == 1.0, "a tensor was clipped: the byte counts assume no gradient write-back"
    us = {k: [] for k in calls}
    for _ in range(args.reps):  # alternated
        for name, fn in calls.items():
            us[name].append(timed(fn))
    out = {"mode": "kernels", "elements": total, "segments": nseg, "iters": args.iters, "reps": args.reps, "kernels": {}}
    for name, v in us.items():
        med = statistics.median(v)
        nbytes = BYTES[name.replace("_scaled", "").replace("_counts", "")]
        out["kernels"][name] = {"us_median": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1), "bytes_per_element": nbytes,
                                "GBps": round(nbytes * total / med / 1e3, 1)}
    if args.scaled and not args.counts:
        out["scaled_minus_unscaled"] = {}
        for name in ("adamw", "lion", "sgd", "lamb"):
            a, b = us[name], us[name + "_scaled"]
            out["scaled_minus_unscaled"][name] = {"us_median_delta": round(statistics.median(b) - statistics.median(a), 1),
                                                  "unscaled_spread_us": round(max(a) - min(a), 1),
                                                  "paired_delta_us": [round(y - x, 1) for x, y in zip(a, b)]}
    if args.counts:
        a, b = us["adamw"], us["adamw_counts"]
        out["counts_minus_uniform"] = {"us_median_delta": round(statistics.median(b) - statistics.median(a), 1),
                                       "uniform_spread_us": round(max(a) - min(a), 1), "paired_delta_us": [round(y - x, 1) for x, y in zip(a, b)]}
    if not all(torch.isfinite(s["p"]).all() for s in sets):
        raise SystemExit("non-finite parameters after the timed launches")
    print(json.dumps(out), flush=True)


def full_step(args):
    from headct_foundation_amd import MaskedAutoencoderViT
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    from headct_foundation_amd.optim import clip_gradients, make_optimizer
    device = torch.device("cuda", 0)
    arch, default_batch, workload, _ = WORKLOADS["vitb"]
    B, S = args.batch or default_batch, arch["input_size"]
    torch.manual_seed(42)
    model = MaskedAutoencoderViT(**arch, compute_dtype="bf16").to(device)
    total_steps = max(1000, args.steps + args.warmup)
    base_lr = STEP_LR[args.optimizer] * B / 256
    opt = make_optimizer(args.optimizer, model, base_lr, betas=(0.9, 0.95), weight_decay=5e-3, momentum=0.9)
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
    print(json.dumps({"mode": "step", "optimizer": args.optimizer, "workload": workload, "per_gpu_batch": B, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(elapsed / args.steps * 1e3, 3), "value": round(B * args.steps / elapsed, 2), "unit": "CT-volumes/s",
                      "loss_first": round(float(lv[0]), 5), "loss_last": round(float(lv[-1]), 5)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["kernels", "step"])
    ap.add_argument("--optimizer", default="AdamW", choices=sorted(STEP_LR))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", action="store_true", help="--mode kernels: hct_adamw_step against hct_adamw_step_counts with mixed counts")
    ap.add_argument("--scaled", action="store_true", help="--mode kernels: also time the _scaled entry points against the unscaled ones")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs an MI355X: the HIP hot path has no CPU fallback")
    kernels(args) if args.mode == "kernels" else full_step(args)


if __name__ == "__main__":
    main()
