"""Generate tests/golden/optimizers.json from the REFERENCE's own optimizers and schedules (build container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_optim.py

Stand-ins for the third-party symbols the image lacks come from make_golden.install_standins (`import src.utils` pulls in timm /
MONAI / transformers through the package's __init__; optimizers.py itself needs only torch).  The fixture holds results only:
  * tensors: for the small hash-generated tensors of tests/optim_ref.CASES, 5 steps of `Lion` and `torch.optim.SGD` built through the
    reference's get_optimizer and of `JITLamb` (constructed directly with the hyper-parameters get_optimizer would pass; the class
    `Lamb` it names accumulates the squared gradient in its first moment, optimizers.py:120) -- parameters and state after every
    step as samples + norms;
  * manifests: the state-dict keys of `Lamb`, `Lion`, `SGD`;
  * schedules: the reference's poly (power 2.0, as its factory calls it) and constant curves for optim_ref.SCHEDULE_CASE;
  * curves: the 4-step loss curve of the reference's engine_pretrain_mae.train_one_epoch on the `micro` MAE case (b2, s0) for
    every (optimizer, schedule) pair of optim_ref.curve_runs().
Before writing, the restatement (tests/optim_ref.py) is asserted against the reference: parameters and state <= 1e-6 relative
(fp32 against fp32), schedule values <= 1e-12, loss curves within 6e-5 (make_golden.run_case's bar).
"""
import json
import logging
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import REF, build_reference_model, install_standins  # noqa: E402
from oracle import mae_oracle as O  # noqa: E402
from tests import optim_ref as R  # noqa: E402

TOL = 1e-6


def sample(t, n):
    f = t.detach().double().flatten()
    idx = np.unique(np.linspace(0, f.numel() - 1, min(n, f.numel())).astype(np.int64))
    r = lambda v: float(f"{v:.9g}")
    return dict(idx=idx.tolist(), val=[r(v) for v in f[idx].tolist()], l2=r(float(f.norm())))


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


class _Cfg:
    def __init__(self, kind, hp):
        class TRAIN:
            OPTIMIZER, MOMENTUM, WEIGHT_DECAY, BETA1, BETA2 = kind, hp["momentum"], hp["weight_decay"], hp["beta1"], hp["beta2"]
        self.TRAIN = TRAIN


def reference_optimizer(RO, kind, module, lr, hp):
    if kind == "Lamb":  # what get_optimizer passes to `Lamb`, given to the class with the first moment of the GRADIENT
        return RO.JITLamb(module.parameters(), lr=lr, weight_decay=hp["weight_decay"], betas=(hp["beta1"], hp["beta2"]))
    return RO.get_optimizer(_Cfg(kind, hp), lr, [module])


def tensor_cases(RO, kind):
    hp = R.HP
    mod = nn.ParameterDict({n: nn.Parameter(p.clone()) for n, p in R.case_params().items()})
    opt = reference_optimizer(RO, kind, mod, hp["lr"], hp)
    mine = R.run_cases(kind, torch.float32)
    mine64 = R.run_cases(kind, torch.float64)
    steps, worst, worst64 = [], 0.0, 0.0
    for s in range(R.NSTEPS):
        for n, g in R.case_grads(s).items():
            mod[n].grad = None if g is None else g.clone()
        opt.step()
        entry = dict(params={}, state={})
        for n, p in mod.items():
            entry["params"][n] = sample(p, 8)
            worst = max(worst, rel(mine[s][0][n], p))
            worst64 = max(worst64, rel(mine64[s][0][n], p))
            st = opt.state.get(p, {})
            assert (n in mine[s][1]) == bool(st) or kind == "SGD", (kind, n)
            entry["state"][n] = {}
            for k in R.STATE_KEYS[kind]:
                if k in st:
                    entry["state"][n][k] = sample(st[k], 8)
                    worst = max(worst, rel(mine[s][1][n][k], st[k]))
        steps.append(entry)
    print(f"[{kind}] restatement vs reference over {R.NSTEPS} steps: fp32 {worst:.2e}, fp64 {worst64:.2e}")
    assert worst <= TOL, (kind, worst)
    sd = opt.state_dict()
    manifest = dict(param_group_keys=sorted(sd["param_groups"][0]), n_groups=len(sd["param_groups"]),
                    state_keys={str(i): sorted(v) for i, v in sd["state"].items()}, params=sd["param_groups"][0]["params"])
    return dict(hp=hp, steps=steps, restatement_rel_dev=float(f"{worst:.3g}"), restatement_fp64_rel_dev=float(f"{worst64:.3g}")), manifest


def lamb_class_manifest(RO):
    """Key layout of the class `get_optimizer` maps 'Lamb' to (one step; its arithmetic is not recorded)."""
    hp = R.HP
    mod = nn.ParameterDict({n: nn.Parameter(p.clone()) for n, p in R.case_params().items()})
    opt = RO.get_optimizer(_Cfg("Lamb", hp), hp["lr"], [mod])
    assert type(opt).__name__ == "Lamb"
    for n, g in R.case_grads(0).items():
        mod[n].grad = None if g is None else g.clone()
    opt.step()
    sd = opt.state_dict()
    return dict(param_group_keys=sorted(sd["param_groups"][0]), n_groups=len(sd["param_groups"]),
                state_keys={str(i): sorted(v) for i, v in sd["state"].items()}, params=sd["param_groups"][0]["params"],
                defaults={k: (list(v) if isinstance(v, tuple) else v) for k, v in opt.defaults.items()})


def schedules(RL):
    c = R.SCHEDULE_CASE
    out = {}
    for kind in ("poly", "constant"):
        opt = torch.optim.SGD([nn.Parameter(torch.zeros(1))], lr=c["lr0"])
        if kind == "poly":
            sch = RL.get_polynomial_decay_schedule_with_warmup(opt, num_warmup_steps=c["warmup"], num_training_steps=c["total"], lr_end=c["lr_end"],
                                                               power=2.0, last_epoch=-1)
        else:
            sch = RL.get_constant_schedule_with_warmup(opt, num_warmup_steps=c["warmup"])
        vals = []
        for _ in range(c["steps"]):
            vals.append(opt.param_groups[0]["lr"])
            opt.step()
            sch.step()
        mine = [c["lr0"] * R.factor(kind, s, c["warmup"], c["total"], c["lr0"], c["lr_end"]) for s in range(c["steps"])]
        assert np.allclose(vals, mine, rtol=1e-12, atol=0), (kind, vals, mine)
        out[kind] = vals
    return dict(case=c, lrs=out)


def curve(RO, RL, kind, sched, name="micro", batch=2, seed=0, nsteps=4):
    import engine_pretrain_mae as E
    cfg = O.CONFIGS[name]
    hp = dict(R.CURVE_HP, base_lr=R.CURVE_LR[kind])
    params = O.make_params(cfg, seed)
    model = build_reference_model(cfg, params)
    if kind == "AdamW":
        opt = RO.get_optimizer(_Cfg("AdamW", hp), hp["base_lr"], [model])
    else:
        opt = reference_optimizer(RO, kind, model, hp["base_lr"], hp)
    sch = {"cosine": lambda: RL.get_cosine_schedule_with_warmup(opt, hp["warmup"], hp["total"], lr_end=hp["min_lr"]),
           "poly": lambda: RL.get_polynomial_decay_schedule_with_warmup(opt, hp["warmup"], hp["total"], lr_end=hp["min_lr"], power=2.0),
           "constant": lambda: RL.get_constant_schedule_with_warmup(opt, hp["warmup"])}[sched]()
    batches = [O.make_volume(cfg, batch, seed + 10 + i) for i in range(nsteps)]
    noises = [O.make_noise(cfg, batch, seed + 10 + i) for i in range(nsteps)]
    it = iter(noises)

    class Cfg:  # the two attributes train_one_epoch reads
        class MODEL: NAME = "mae"
        class TRAIN: GRAD_CLIP = hp["grad_clip"]
    losses, lrs = [], []

    class L(logging.Logger):
        def info(self, msg, *a, **k):
            if "Loss:" in str(msg):
                losses.append(float(str(msg).split("Loss:")[1]))
    real_rand, real_sync, real_step = torch.rand, torch.cuda.synchronize, sch.step

    def step_spy(*a, **k):
        lrs.append(opt.param_groups[0]["lr"])
        return real_step(*a, **k)
    sch.step = step_spy
    torch.cuda.synchronize = lambda *a, **k: None
    torch.rand = lambda *a, **k: next(it).clone()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            stats = E.train_one_epoch(Cfg, model, batches, opt, sch, 0, 1, logger=L("g"), device=torch.device("cpu"), use_amp=False,
                                      scaler=torch.amp.GradScaler(enabled=False), wandb_run=None)
    finally:
        torch.rand, torch.cuda.synchronize = real_rand, real_sync
    st = R.TrainState({k: v.clone() for k, v in params.items()})
    o_losses, o_lrs = [], []
    for i in range(nsteps):
        l, lr, _ = R.train_step(cfg, st, batches[i], noises[i], kind, sched, **hp)
        o_losses.append(l)
        o_lrs.append(lr)
    ref_params = dict(model.named_parameters())
    perr = max(rel(st.params[k], ref_params[k]) for k in ref_params if not k.endswith("qkv.bias"))
    print(f"[{kind}/{sched}] curve ref {losses} restatement {[round(v, 5) for v in o_losses]} lrs {lrs} param-relerr (qkv.bias aside) {perr:.2e}")
    assert np.allclose(losses, o_losses, atol=6e-5) and np.allclose(lrs, o_lrs, rtol=1e-12, atol=0), (kind, sched)
    return dict(optimizer=kind, scheduler=sched, hp=hp, config=name, batch=batch, seed=seed, steps=nsteps, logged_losses=losses, lrs=lrs,
                avg_loss=stats["loss"], restatement_param_rel_dev=float(f"{perr:.3g}"),
                params_after={k: sample(v, 3) for k, v in ref_params.items()} if sched == "cosine" else None)


def main():
    install_standins()
    sys.path.insert(0, REF)
    from src.utils import lr_sched as RL
    from src.utils import optimizers as RO
    fx = dict(tensors={}, manifests={})
    for kind in R.KINDS:
        fx["tensors"][kind], man = tensor_cases(RO, kind)
        fx["manifests"]["JITLamb" if kind == "Lamb" else kind] = man
    fx["manifests"]["Lamb"] = lamb_class_manifest(RO)
    fx["schedules"] = schedules(RL)
    fx["curves"] = [curve(RO, RL, k, s) for k, s in R.curve_runs()]
    path = os.path.join(HERE, "optimizers.json")
    with open(path, "w") as f:
        json.dump(fx, f, separators=(",", ":"))
    print("optimizers.json:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
