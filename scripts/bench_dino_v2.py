"""What the DINOv2 additions cost on the HIP path: the Sinkhorn-Knopp teacher and the KoLeo regulariser.

Default, two cases, the sides of each alternating in one process after a warm-up (per side the median round and the spread):
  (a) teacher distribution + DINO loss + gradient at V = 10 crops, B = 64, K = 65 536 prototypes, bf16 logits: DINOLoss with
      centering="sinkhorn_knopp" (three rounds of hct_dino_sk_col_lse / hct_dino_sk_row_lse, then hct_dino_loss_sk) beside DINOLoss with the
      EMA centre (hct_dino_loss + hct_dino_center_update) and beside the torch composition of Sinkhorn-Knopp (DINOv2's exp / normalise form
      on a transposed fp32 [K, 2B] matrix) plus the soft cross-entropy of this project's pairing with its autograd backward.
  (b) koleo_loss forward + backward on the class-token rows of a [64, 517, 768] bf16 token tensor beside the torch composition
      (F.normalize, the [n, n] product, argmax, F.pairwise_distance, log, mean; autograd backward).
`--step` instead runs the `bench.py --config dino` training step (ViT-B/12^3 student + teacher, 2 + 8 crops of 96^3 x 3 channels, B = 64,
bf16) with both additions off and with both on (sinkhorn_knopp, KoLeo weight 0.1), alternating.  Prints one JSON line.

  python scripts/bench_dino_v2.py [--iters 20] [--warmup 3] [--rounds 5] [--step] [--out profiles/dino_v2_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from headct_foundation_amd.dino import DINOLoss, DinoDataParallel, DinoOptimizer, koleo_loss, update_momentum_encoder, wd_cosine_scheduler  # noqa: E402


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


def alternate(cases: dict, iters: int, warmup: int, n_rounds: int) -> dict:
    for call in cases.values():
        for _ in range(warmup):
            call()
    torch.cuda.synchronize()
    rounds = {k: [] for k in cases}
    for _ in range(n_rounds):
        for k, call in cases.items():
            rounds[k].append(event_us(call, iters))
    return {k: summary(v) for k, v in rounds.items()}


def torch_sinkhorn_knopp(teacher, temp: float, n_iters: int = 3):
    """DINOv2's sinkhorn_knopp_teacher on one rank."""
    Q = torch.exp(teacher.float() / temp).t()
    K, N = Q.shape
    Q /= Q.sum()
    for _ in range(n_iters):
        Q /= Q.sum(dim=1, keepdim=True)
        Q /= K
        Q /= Q.sum(dim=0, keepdim=True)
        Q /= N
    Q *= N
    return Q.t()


def torch_dino_loss(student, q, V: int, student_temp: float):
    """This project's pairing and 1 / (2 (V - 1)) normalisation over a given teacher distribution."""
    B = q.shape[0] // 2
    logp = F.log_softmax(student.float() / student_temp, dim=-1).view(V, B, -1)
    qq = q.view(2, B, -1)
    total = 0.0
    for i in range(2):
        for v in range(V):
            if v != i:
                total = total + (-(qq[i] * logp[v]).sum(dim=-1)).mean()
    return total / (2 * (V - 1))


def torch_koleo(x):
    xh = F.normalize(x.float(), eps=1e-8, p=2, dim=-1)
    with torch.no_grad():
        dots = xh @ xh.t()
        dots.view(-1)[:: x.shape[0] + 1].fill_(-1)
        idx = dots.argmax(dim=1)
    return -torch.log(F.pairwise_distance(xh, xh[idx], eps=1e-8) + 1e-8).mean()


def kernel_part(dev, iters: int, warmup: int, n_rounds: int) -> dict:
    V, B, K, temp = 10, 64, 65536, 0.04
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    # prototype logits are cosines (weight-normalised prototypes on L2-normalised features): |logit| <= 1
    student = (torch.rand(V * B, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16).requires_grad_(True)
    teacher = (torch.rand(2 * B, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
    crit_c = DINOLoss(K, V, temp, temp, 0, 2).to(dev)
    crit_sk = DINOLoss(K, V, temp, temp, 0, 2, centering="sinkhorn_knopp").to(dev)

    def run(loss_fn):
        student.grad = None
        loss_fn().backward()

    a = alternate({"sinkhorn_knopp_hip": lambda: run(lambda: crit_sk(student, teacher, 0)),
                   "centering_hip": lambda: run(lambda: crit_c(student, teacher, 0)),
                   "sinkhorn_knopp_torch": lambda: run(lambda: torch_dino_loss(student, torch_sinkhorn_knopp(teacher, temp), V, 0.1))}, iters, warmup, n_rounds)
    with torch.no_grad():
        same = abs(float(crit_sk(student, teacher, 0)) - float(torch_dino_loss(student, torch_sinkhorn_knopp(teacher, temp), V, 0.1)))
    a.update(shape={"V": V, "B": B, "K": K, "dtype": "bf16"}, hip_minus_torch_loss=same,
             sinkhorn_over_centering=round(a["sinkhorn_knopp_hip"]["us"] / a["centering_hip"]["us"], 3),
             sinkhorn_hip_over_torch=round(a["sinkhorn_knopp_hip"]["us"] / a["sinkhorn_knopp_torch"]["us"], 3))

    n, T, D = 64, 517, 768
    tokens = torch.randn(n, T, D, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)

    def run_k(fn):
        tokens.grad = None
        fn(tokens[:, 0, :]).backward()

    b = alternate({"koleo_hip": lambda: run_k(koleo_loss), "koleo_torch": lambda: run_k(torch_koleo)}, iters, warmup, n_rounds)
    with torch.no_grad():
        same = abs(float(koleo_loss(tokens[:, 0, :])) - float(torch_koleo(tokens[:, 0, :])))
    b.update(shape={"n": n, "tokens": T, "D": D, "dtype": "bf16"}, hip_minus_torch_loss=same, koleo_hip_over_torch=round(b["koleo_hip"]["us"] / b["koleo_torch"]["us"], 3))
    return {"teacher_and_loss": a, "koleo": b, "iters": iters, "warmup": warmup, "rounds": n_rounds}


def step_part(dev, B: int, steps: int, warmup: int, n_rounds: int) -> dict:
    import bench
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    cfg = bench.DINO
    V, w = cfg["crops"], 0.1
    torch.manual_seed(42)
    mk = lambda: MultiCropWrapper(ViTBackbone(**cfg["vit"], compute_dtype="bf16"), DINOHead(**cfg["head"], compute_dtype="bf16")).to(dev)
    student, teacher = mk(), mk()
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad_(False)
    model, momentum_model = DinoDataParallel(student), DinoDataParallel(teacher)
    total = 1000
    lr = 5e-4 * B / 256
    opt = DinoOptimizer(model, lr=lr, betas=(0.9, 0.999), weight_decay=0.04)
    sched = get_cosine_schedule_with_warmup(opt.primary, int(0.1 * total), total, lr_end=lr * 1e-3)
    wd, mom = wd_cosine_scheduler(0.04, 0.4, 1, total), wd_cosine_scheduler(0.999, 1.0, 1, total)
    crit = {False: DINOLoss(cfg["head"]["out_dim"], V, 0.04, 0.04, 30, 200).to(dev),
            True: DINOLoss(cfg["head"]["out_dim"], V, 0.04, 0.04, 30, 200, centering="sinkhorn_knopp").to(dev)}
    S = cfg["vit"]["img_size"]
    pool = [[torch.rand(B, 3, S, S, S, device=dev) for _ in range(V)] for _ in range(2)]
    count = [0]

    def step(on: bool):
        i = count[0]
        count[0] += 1
        opt.param_groups[0]["weight_decay"] = float(wd[i])
        opt.zero_grad()
        crops = pool[i % 2]
        student.return_cls = on
        with torch.no_grad():
            t_out = momentum_model(crops[:2])['dino_output']
        out = model(crops)
        loss = crit[on](out['dino_output'].float(), t_out.float(), 0)
        if on:
            cls = out['cls_tokens']
            loss = loss + w * (koleo_loss(cls[:B]) + koleo_loss(cls[B:2 * B]))
        loss.backward()
        model.reduce_head_gradients()
        opt.step()
        sched.step()
        update_momentum_encoder(student.backbone, teacher.backbone, float(mom[i]))
        update_momentum_encoder(student.head, teacher.head, float(mom[i]))
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
           "rounds": n_rounds, "koleo_weight": w}
    for on, name in ((False, "both_off"), (True, "both_on")):
        out[name] = {"ms_per_step": round(statistics.median(rounds[on]), 3), "rounds_ms": [round(r, 3) for r in rounds[on]],
                     "spread_pct": round(100 * (max(rounds[on]) - min(rounds[on])) / min(rounds[on]), 2)}
    out["cost_pct"] = round(100 * (out["both_on"]["ms_per_step"] / out["both_off"]["ms_per_step"] - 1), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="calls per timed round (kernel cases) or steps per round (--step)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--step", action="store_true", help="time the DINO training step with both additions off and on instead of the kernels alone")
    ap.add_argument("--out", default="", help="also write the JSON to this file (a file that holds the other part keeps it)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dino_v2.py needs an MI355X: a timing off the GPU says nothing")
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
