"""Plain-torch restatement of the Lion / SGD / Lamb updates and the poly / constant schedules the HIP path implements
(reference: src/utils/optimizers.py:267-279 `update_fn`, torch.optim.SGD as :347-353 builds it, :154-172 `lamb_kernel`;
src/utils/lr_sched.py:89-99 and :119-122).  Every function works in the dtype of the tensors it is given (fp32 to mirror the
kernels, fp64 as the yardstick) and updates them in place.  tests/golden/make_golden_optim.py asserts this file against the
reference's own classes before it writes tests/golden/optimizers.json; tests/test_optim_cpu.py pins it to that fixture.
"""
from typing import Dict, List, Optional

import numpy as np
import torch

from oracle import mae_oracle as O

KINDS = ("Lion", "SGD", "Lamb")
STATE_KEYS = {"Lion": ("exp_avg",), "SGD": ("momentum_buffer",), "Lamb": ("exp_avg", "exp_avg_sq")}
# hyper-parameters of the fixture's tensor cases and of its MAE curves (lr per optimizer: a rate at which 4 steps move the loss;
# warm-up 1 of 4 steps, so that the three schedules already differ at the rate of the third step, which the fourth loss sees)
HP = dict(lr=1e-3, weight_decay=5e-3, beta1=0.9, beta2=0.95, momentum=0.9, eps=1e-6)
CURVE_LR = {"Lion": 1e-3, "SGD": 5e-2, "Lamb": 5e-3, "AdamW": 1e-3}
CURVE_HP = dict(min_lr=1e-6, warmup=1, total=4, weight_decay=5e-3, beta1=0.9, beta2=0.95, momentum=0.9, grad_clip=3.0)
SCHEDULE_CASE = dict(warmup=3, total=12, lr0=1e-3, lr_end=1e-6, steps=16)  # steps 13..15 are past `total`
LAMB_EPS = 1e-6  # the class default: the reference's get_optimizer passes none


# ---- the three updates -----------------------------------------------------------------------------------------------------------
def lion_step_(p, g, m, lr, wd, beta1, beta2):
    """Returns c = beta1*m + (1-beta1)*g (m BEFORE the step), whose sign is the update."""
    p.mul_(1 - lr * wd)
    c = m.clone().mul_(beta1).add(g, alpha=1 - beta1)
    p.add_(torch.sign(c), alpha=-lr)
    m.mul_(beta2).add_(g, alpha=1 - beta2)
    return c


def sgd_step_(p, g, buf, lr, momentum):
    """buf is None with momentum 0 (torch keeps no buffer); a zero buffer gives the first step's buf = g."""
    if buf is None:
        p.add_(g, alpha=-lr)
    else:
        buf.mul_(momentum).add_(g)
        p.add_(buf, alpha=-lr)


def lamb_step_(p, g, m, v, lr, beta1, beta2, eps, wd):
    """Returns (weight_norm, adam_norm, trust_ratio) as 0-d tensors."""
    m.copy_(m * beta1 + (1 - beta1) * g)
    v.copy_(v * beta2 + (1 - beta2) * (g * g))
    u = m / (v.sqrt() + eps) + wd * p
    w = p.norm(p=2).clamp(0, 10)
    a = u.norm(p=2)
    r = torch.where((w == 0) | (a == 0), torch.ones_like(w), w / (a + eps))
    p.copy_(p - lr * r * u)
    return w, a, r


def new_state(kind, p, momentum=0.9):
    if kind == "SGD" and momentum == 0:
        return {}
    return {k: torch.zeros_like(p) for k in STATE_KEYS[kind]}


def apply_(kind, p, g, state, lr, hp):
    """One update of one tensor; `state` from new_state.  Returns what the update function returns."""
    if kind == "Lion":
        return lion_step_(p, g, state["exp_avg"], lr, hp["weight_decay"], hp["beta1"], hp["beta2"])
    if kind == "SGD":
        return sgd_step_(p, g, state.get("momentum_buffer"), lr, hp["momentum"])
    if kind == "Lamb":
        out = lamb_step_(p, g, state["exp_avg"], state["exp_avg_sq"], lr, hp["beta1"], hp["beta2"], hp.get("eps", LAMB_EPS), hp["weight_decay"])
        state["weight_norm"], state["adam_norm"], state["trust_ratio"] = out
        return out
    raise ValueError(kind)


def lion_excused(c, m_before, g, beta1, tol=1e-5):
    """Elements whose sign argument cancels to rounding: |c| <= tol * (beta1*|m| + (1-beta1)*|g|).  Two correct implementations may
    step such an element in opposite directions.  An element with m = g = 0 is NOT excused: its c is an exact 0 in any arithmetic
    (sign 0, no step), so there is nothing to forgive -- the masked rows of the position table are of that kind on the MAE."""
    scale = beta1 * m_before.abs() + (1 - beta1) * g.abs()
    return (c.abs() <= tol * scale) & (scale > 0)


# ---- schedules -------------------------------------------------------------------------------------------------------------------
def poly_factor(step, warmup, total, lr0, lr_end, power=2.0):
    if step < warmup:
        return float(step) / float(max(1, warmup))
    if step > total:
        return lr_end / lr0
    return ((lr0 - lr_end) * (1 - (step - warmup) / (total - warmup)) ** power + lr_end) / lr0


def constant_factor(step, warmup):
    return float(step) / float(max(1.0, warmup)) if step < warmup else 1.0


def factor(sched, step, warmup, total, lr0, lr_end):
    if sched == "cosine":
        return O.cosine_warmup_lambda(step, warmup, total, lr0, lr_end)
    if sched == "poly":
        return poly_factor(step, warmup, total, lr0, lr_end)
    if sched == "constant":
        return constant_factor(step, warmup)
    raise ValueError(sched)


# ---- the fixture's tensor cases ----------------------------------------------------------------------------------------------------
NSTEPS = 5
CASES = [  # name, shape, parameter scale, gradient: "rand" | "zero" | None
    ("plain", (3, 40), 0.5, "rand"),
    ("big_norm", (64, 8), 1.0, "rand"),   # ||p|| ~ 13 > 10: Lamb's clamp
    ("param_zero", (17,), 0.0, "rand"),   # weight_norm == 0 -> trust ratio 1
    ("grad_zero", (5, 9), 0.3, "zero"),   # sign(0) = 0; Lamb's adam_norm = wd * ||p||
    ("grad_none", (11,), 0.2, None),
    ("vector", (300,), 0.05, "rand"),
]


def case_params(dtype=torch.float32) -> Dict[str, torch.Tensor]:
    return {n: (s * torch.from_numpy(O.hash_uniform(int(np.prod(shape)), 900 + k)).reshape(shape)).to(dtype)
            for k, (n, shape, s, _) in enumerate(CASES)}


def case_grads(step: int, dtype=torch.float32) -> Dict[str, Optional[torch.Tensor]]:
    """Fresh hash per step (about half the elements change sign from one step to the next), magnitude growing with the step."""
    out = {}
    for k, (n, shape, _, kind) in enumerate(CASES):
        if kind is None:
            out[n] = None
        elif kind == "zero":
            out[n] = torch.zeros(shape, dtype=dtype)
        else:
            out[n] = ((1.0 + 0.25 * step) * torch.from_numpy(O.hash_uniform(int(np.prod(shape)), 1900 + 37 * step + k)).reshape(shape)).to(dtype)
    return out


def run_cases(kind, dtype=torch.float32, hp=HP, nsteps=NSTEPS):
    """[(params, states)] after every step, deep copies."""
    params = case_params(dtype)
    states = {n: new_state(kind, p, hp["momentum"]) for n, p in params.items() if dict((c[0], c[3]) for c in CASES)[n] is not None}
    hist = []
    for s in range(nsteps):
        for n, g in case_grads(s, dtype).items():
            if g is not None:
                apply_(kind, params[n], g, states[n], hp["lr"], hp)
        hist.append(({n: p.clone() for n, p in params.items()}, {n: {k: v.clone() for k, v in st.items()} for n, st in states.items()}))
    return hist


# ---- torch-side optimizers with the reference's state-dict layout (what a reference checkpoint holds) ------------------------------
class RefLion(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self):
        for grp in self.param_groups:
            for p in grp["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["exp_avg"] = torch.zeros_like(p)
                lion_step_(p, p.grad, st["exp_avg"], grp["lr"], grp["weight_decay"], *grp["betas"])


class RefLamb(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=LAMB_EPS, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self):
        for grp in self.param_groups:
            for p in grp["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st.update(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
                st["step"] += 1
                st["weight_norm"], st["adam_norm"], st["trust_ratio"] = lamb_step_(
                    p, p.grad, st["exp_avg"], st["exp_avg_sq"], grp["lr"], *grp["betas"], grp["eps"], grp["weight_decay"])


def torch_optimizer(kind, params, lr, hp=HP):
    if kind == "Lion":
        return RefLion(params, lr=lr, betas=(hp["beta1"], hp["beta2"]), weight_decay=hp["weight_decay"])
    if kind == "Lamb":
        return RefLamb(params, lr=lr, betas=(hp["beta1"], hp["beta2"]), weight_decay=hp["weight_decay"])
    if kind == "SGD":
        return torch.optim.SGD(params, lr=lr, momentum=hp["momentum"])
    if kind == "AdamW":
        return torch.optim.AdamW(params, lr=lr, betas=(hp["beta1"], hp["beta2"]), weight_decay=hp["weight_decay"])
    raise ValueError(kind)


# ---- one MAE iteration (engine_pretrain_mae.py:52-71) with one of the optimizers and schedules --------------------------------------
class TrainState:
    def __init__(self, params):
        self.params, self.state, self.step = params, {}, 0


def train_step(cfg, st: TrainState, x, noise, kind: str, sched: str, *, base_lr, min_lr, warmup, total, weight_decay, beta1, beta2,
               momentum, grad_clip, emulate_bf16=False):
    loss, _, _, grads, _ = O.forward_backward(cfg, st.params, x, noise, emulate_bf16=emulate_bf16)
    if grad_clip:
        O.clip_gradients_(grads, grad_clip)
    lr = base_lr * factor(sched, st.step, warmup, total, base_lr, min_lr)
    st.step += 1
    hp = dict(weight_decay=weight_decay, beta1=beta1, beta2=beta2, momentum=momentum)
    with torch.no_grad():
        for k, g in grads.items():
            if kind == "AdamW":
                s = st.state.setdefault(k, {"exp_avg": torch.zeros_like(g), "exp_avg_sq": torch.zeros_like(g)})
                O.adamw_step_(st.params[k], g, s["exp_avg"], s["exp_avg_sq"], st.step, lr, beta1, beta2, 1e-8, weight_decay)
            else:
                if k not in st.state:
                    st.state[k] = new_state(kind, g, momentum)
                apply_(kind, st.params[k], g, st.state[k], lr, hp)
    return float(loss), lr, grads


def curve_runs() -> List[List[str]]:
    """(optimizer, schedule) pairs whose 4-step MAE loss curve the fixture holds."""
    return [[k, s] for k in KINDS for s in ("cosine", "poly", "constant")] + [["AdamW", "poly"], ["AdamW", "constant"]]
