"""What the iBOT masked patch-token loss costs on the HIP path.

Default, three cases, the sides of each alternating in one process after a warm-up (per side the median round and the spread):
  (a) hct_ibot_loss alone (loss + gradient + centre sums) at M = 9 800 masked rows (an estimate of the row count at the bench shape: 64 of the
      128 global crops masked at a mean ratio of 0.3 of 512 patches), K = 65 536 prototypes, bf16 logits, beside the torch composition
      (softmax / log_softmax in fp32, autograd backward).  Reported as microseconds and as GB/s over (2 + 2 + 1) * M * K * 2 bytes: student
      and teacher read twice, the gradient written once.
  (b) hct_vit_assemble_masked_fwd and hct_vit_assemble_masked_bwd alone at the student's shape of `bench.py --config dino` (640 volumes,
      512 patches, 4 register tokens, width 768, bf16 tokens; the masks of a step's draw), beside hct_vit_assemble_fwd / _bwd.
`--step` instead runs the `bench.py --config dino` training step (ViT-B/12^3 student + teacher, 2 + 8 crops of 96^3 x 3 channels, B = 64,
bf16) with the iBOT term off and on (weight 1), alternating, on ONE pair of models built with a mask token: the student's plan of 640
volumes takes 143 GB of workspace, so two pairs do not fit on one card.  The side without the term runs the plain recipe's launches plus
the memset of the unused mask token's gradient; `bench.py --config dino` itself is the step without a mask token.  Prints one JSON line.

  python scripts/bench_ibot.py [--iters 20] [--warmup 3] [--rounds 5] [--step] [--out profiles/ibot_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from headct_foundation_amd import _lib  # noqa: E402
from headct_foundation_amd.dino import DINOLoss, DinoDataParallel, DinoOptimizer, update_momentum_encoder, wd_cosine_scheduler  # noqa: E402
from headct_foundation_amd.ibot import IBOTPatchLoss, IBotMaskGenerator, IBotObjective, ibot_rows_and_weights  # noqa: E402
from scripts.bench_dino_v2 import alternate  # noqa: E402


def torch_ibot_loss(student, teacher, weight, center, inv_images, Ts=0.1, Tt=0.04):
    q = F.softmax((teacher.float() - center) / Tt, dim=-1)
    logp = F.log_softmax(student.float() / Ts, dim=-1)
    return -inv_images * (weight * (q * logp).sum(dim=-1)).sum()


def kernel_part(dev, iters: int, warmup: int, n_rounds: int) -> dict:
    lib = _lib.load()
    st = _lib.stream_ptr()
    M, K, n_g = 9800, 65536, 128
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    # prototype logits are cosines (weight-normalised prototypes on L2-normalised features): |logit| <= 1
    student = (torch.rand(M, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
    teacher = (torch.rand(M, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
    weight = 1.0 / torch.randint(51, 257, (M,), device=dev, generator=g).float()
    center = torch.zeros(K, device=dev)
    loss, ds, csum = torch.empty(1, device=dev), torch.empty_like(student), torch.empty(K, device=dev)
    ws = torch.empty(lib.hct_ibot_loss_workspace_bytes(M, K), dtype=torch.uint8, device=dev)

    def hip():
        _lib.check(lib.hct_ibot_loss(student.data_ptr(), teacher.data_ptr(), _lib.HCT_BF16, M, K, weight.data_ptr(), center.data_ptr(), 0.1, 0.04,
                                     1.0 / n_g, loss.data_ptr(), ds.data_ptr(), None, csum.data_ptr(), ws.data_ptr(), ws.numel(), st), "hct_ibot_loss")

    s_t = student.clone().requires_grad_(True)

    def composed():
        s_t.grad = None
        torch_ibot_loss(s_t, teacher, weight, center, 1.0 / n_g).backward()

    a = alternate({"ibot_loss_hip": hip, "ibot_loss_torch": composed}, iters, warmup, n_rounds)
    with torch.no_grad():
        same = abs(float(loss) - float(torch_ibot_loss(student, teacher, weight, center, 1.0 / n_g)))
    nbytes = (2 + 2 + 1) * M * K * 2
    a.update(shape={"M": M, "K": K, "dtype": "bf16"}, hip_minus_torch_loss=same, bytes=nbytes,
             hip_gb_per_s=round(nbytes / a["ibot_loss_hip"]["us"] * 1e-3, 1), hip_over_torch=round(a["ibot_loss_hip"]["us"] / a["ibot_loss_torch"]["us"], 3))
    del s_t, student, teacher, ds, ws

    B, L, R, D = 640, 512, 4, 768
    masks = np.zeros((B, L), dtype=np.uint8)
    masks[:n_g] = IBotMaskGenerator(8, seed=0)(n_g)
    mask = torch.from_numpy(masks).to(dev)
    tok = torch.randn(B * L, D, device=dev, generator=g).to(torch.bfloat16)
    cls, reg, pos, mt = (torch.randn(n, D, device=dev, generator=g) for n in (1, R, L, 1))
    h0 = torch.empty(B, 1 + R + L, D, device=dev)
    dh0 = torch.randn(B, 1 + R + L, D, device=dev, generator=g)
    dtok = torch.empty_like(tok)
    dcls, dreg, dpos, dmt = (torch.empty(n, D, device=dev) for n in (1, R, L, 1))
    ws = torch.empty(lib.hct_vit_assemble_masked_bwd_workspace_bytes(B, L, D), dtype=torch.uint8, device=dev)
    code = _lib.HCT_BF16
    b = alternate({
        "masked_fwd": lambda: _lib.check(lib.hct_vit_assemble_masked_fwd(tok.data_ptr(), code, cls.data_ptr(), reg.data_ptr(), pos.data_ptr(), mt.data_ptr(),
                                                                         mask.data_ptr(), B, L, R, D, h0.data_ptr(), st), "hct_vit_assemble_masked_fwd"),
        "plain_fwd": lambda: _lib.check(lib.hct_vit_assemble_fwd(tok.data_ptr(), code, cls.data_ptr(), reg.data_ptr(), pos.data_ptr(), B, L, R, D,
                                                                 h0.data_ptr(), st), "hct_vit_assemble_fwd"),
        "masked_bwd": lambda: _lib.check(lib.hct_vit_assemble_masked_bwd(dh0.data_ptr(), mask.data_ptr(), B, L, R, D, dtok.data_ptr(), code, dcls.data_ptr(),
                                                                         dreg.data_ptr(), dpos.data_ptr(), dmt.data_ptr(), ws.data_ptr(), ws.numel(), st),
                                         "hct_vit_assemble_masked_bwd"),
        "plain_bwd": lambda: _lib.check(lib.hct_vit_assemble_bwd(dh0.data_ptr(), B, L, R, D, dtok.data_ptr(), code, dcls.data_ptr(), dreg.data_ptr(),
                                                                 dpos.data_ptr(), st), "hct_vit_assemble_bwd"),
    }, iters, warmup, n_rounds)
    b.update(shape={"B": B, "L": L, "R": R, "D": D, "tok": "bf16", "masked_rows": int(masks.sum())})
    return {"ibot_loss": a, "assembly": b, "iters": iters, "warmup": warmup, "rounds": n_rounds}


def step_part(dev, B: int, steps: int, warmup: int, n_rounds: int) -> dict:
    import bench
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    cfg = bench.DINO
    V, K = cfg["crops"], cfg["head"]["out_dim"]
    S = cfg["vit"]["img_size"]
    pool = [[torch.rand(B, 3, S, S, S, device=dev) for _ in range(V)] for _ in range(2)]
    total = 1000
    lr = 5e-4 * B / 256
    wd, mom = wd_cosine_scheduler(0.04, 0.4, 1, total), wd_cosine_scheduler(0.999, 1.0, 1, total)
    torch.manual_seed(42)
    mk = lambda: MultiCropWrapper(ViTBackbone(**cfg["vit"], compute_dtype="bf16", mask_token=True), DINOHead(**cfg["head"], compute_dtype="bf16")).to(dev)
    student, teacher = mk(), mk()
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad_(False)
    model, momentum_model = DinoDataParallel(student), DinoDataParallel(teacher)
    opt = DinoOptimizer(model, lr=lr, betas=(0.9, 0.999), weight_decay=0.04)
    sched = get_cosine_schedule_with_warmup(opt.primary, int(0.1 * total), total, lr_end=lr * 1e-3)
    crit = DINOLoss(K, V, 0.04, 0.04, 30, 200).to(dev)
    ibot = IBotObjective(1.0, IBotMaskGenerator(S // cfg["vit"]["patch_size"], seed=42), IBOTPatchLoss(K, 0.04, 0.04, 30, 200).to(dev),
                         cfg["vit"]["num_register_tokens"])
    shared = dict(student=student, teacher=teacher, model=model, momentum_model=momentum_model, opt=opt, sched=sched, crit=crit, ibot=ibot, count=0, rows=[])
    sides = {False: shared, True: shared}  # one pair of models, one step counter

    def step(on: bool):
        s = sides[on]
        i = s["count"]
        s["count"] += 1
        s["opt"].param_groups[0]["weight_decay"] = float(wd[i])
        s["opt"].zero_grad()
        crops = pool[i % 2]
        if not on:
            with torch.no_grad():
                t_out = s["momentum_model"](crops[:2])['dino_output']
            out = s["model"](crops)
            loss = s["crit"](out['dino_output'].float(), t_out.float(), 0)
        else:
            masks, rows, weights = s["ibot"].draw(2 * B, dev)
            s["rows"].append(len(rows))
            with torch.no_grad():
                t_out = s["momentum_model"](crops[:2], patch_rows=rows)
            out = s["model"](crops, masks=masks, patch_rows=rows)
            loss = s["crit"](out['dino_output'].float(), t_out['dino_output'].float(), 0)
            loss = loss + s["ibot"].weight * s["ibot"].loss(out['ibot_output'], t_out['ibot_output'], weights, 2 * B, 0)
        loss.backward()
        s["model"].reduce_head_gradients()
        s["opt"].step()
        s["sched"].step()
        update_momentum_encoder(s["student"].backbone, s["teacher"].backbone, float(mom[i]))
        update_momentum_encoder(s["student"].head, s["teacher"].head, float(mom[i]))
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
    out = {"metric": "DINO training step of bench.py --config dino (one MI355X, bf16), ms per step", "batch": B, "steps": steps, "warmup": warmup,
           "rounds": n_rounds, "masked_rows_per_step_mean": round(statistics.mean(sides[True]["rows"]), 1),
           "head_rows": {"weight_0": V * B, "weight_1_mean": round(V * B + statistics.mean(sides[True]["rows"]), 1)}}
    for on, name in ((False, "weight_0"), (True, "weight_1")):
        out[name] = {"ms_per_step": round(statistics.median(rounds[on]), 3), "rounds_ms": [round(r, 3) for r in rounds[on]],
                     "spread_pct": round(100 * (max(rounds[on]) - min(rounds[on])) / min(rounds[on]), 2)}
    out["cost_pct"] = round(100 * (out["weight_1"]["ms_per_step"] / out["weight_0"]["ms_per_step"] - 1), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="calls per timed round (kernel cases) or steps per round (--step)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--step", action="store_true", help="time the DINO training step with the iBOT weight at 0 and at 1 instead of the kernels alone")
    ap.add_argument("--out", default="", help="also write the JSON to this file (a file that holds the other part keeps it)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ibot.py needs an MI355X: a timing off the GPU says nothing")
    dev = torch.device("cuda:0")
    key, result = ("step", step_part(dev, a.batch, a.iters, a.warmup, a.rounds)) if a.step else ("kernels", kernel_part(dev, a.iters, a.warmup, a.rounds))
    print(json.dumps({key: result}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        merged = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                merged = json.load(f)
        merged[key] = result
        with open(a.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()
