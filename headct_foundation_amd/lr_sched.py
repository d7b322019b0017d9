"""Learning-rate schedules (cosine, polynomial, constant; each with a linear warm-up), stepped once per iteration.

Contract of the cosine one, the MAE recipe's (reference: src/utils/lr_sched.py:18-55 for the curve, :127-139 for the factory): the rate climbs linearly from 0
to the optimizer's initial rate over `num_warmup_steps` iterations, then follows `lr_end + (lr0 - lr_end) * (1 + cos(2*pi*
num_cycles * t)) / 2` with t = fraction of the post-warm-up iterations done, never below 0.  The object handed back is a
`torch.optim.lr_scheduler.LambdaLR`, so its `state_dict()` is what reference checkpoints carry under "scheduler".
Pure host arithmetic: one Python float per step.
"""
import math

from torch.optim.lr_scheduler import LambdaLR


def warmup_cosine(lr0: float, lr_end: float, warmup: int, total: int, cycles: float):
    """Multiplicative factor lr(step) / lr0 as a plain closure: LambdaLR.state_dict() stores `None` for functions (only callable
    OBJECTS have their attributes saved), exactly what a reference checkpoint holds under scheduler["lr_lambdas"] -- so a resume
    with a changed MAX_EPOCHS / PER_WARMUP / LR follows the NEW run's curve, as the reference's does, instead of silently
    restoring the old one's constants."""
    lr0, lr_end, warmup, total, cycles = float(lr0), float(lr_end), int(warmup), int(total), float(cycles)

    def factor(step: int) -> float:
        if step < warmup:
            return step / max(1, warmup)
        done = (step - warmup) / max(1, total - warmup)
        wave = 0.5 * (1.0 + math.cos(2.0 * math.pi * cycles * done))
        return max(0.0, (lr_end + (lr0 - lr_end) * wave) / lr0)

    return factor


def get_cosine_schedule_with_warmup(optimizer, num_warmup_steps: int, num_training_steps: int, num_cycles: float = 0.5,
                                    lr_end: float = 1e-6, last_epoch: int = -1):
    lr0 = optimizer.defaults["lr"]
    if lr_end >= lr0:
        raise ValueError(f"cosine schedule needs lr_end < initial lr, got lr_end={lr_end} and lr={lr0}")
    return LambdaLR(optimizer, warmup_cosine(lr0, lr_end, num_warmup_steps, num_training_steps, num_cycles), last_epoch)


def warmup_poly(lr0: float, lr_end: float, warmup: int, total: int, power: float):
    """lr(step) / lr0 of the polynomial decay (reference: src/utils/lr_sched.py:89-99): linear warm-up, then
    ((lr0 - lr_end) * (1 - (step - warmup) / (total - warmup)) ** power + lr_end) / lr0, and lr_end / lr0 once step > total.
    A plain closure for the reason `warmup_cosine` gives."""
    lr0, lr_end, warmup, total = float(lr0), float(lr_end), int(warmup), int(total)

    def factor(step: int) -> float:
        if step < warmup:
            return float(step) / float(max(1, warmup))
        if step > total:
            return lr_end / lr0
        remaining = 1 - (step - warmup) / (total - warmup)
        return ((lr0 - lr_end) * remaining ** power + lr_end) / lr0

    return factor


def get_polynomial_decay_schedule_with_warmup(optimizer, num_warmup_steps: int, num_training_steps: int, lr_end: float = 1e-7,
                                              power: float = 1.0, last_epoch: int = -1):
    lr0 = optimizer.defaults["lr"]
    if not (lr0 > lr_end):
        raise ValueError(f"lr_end ({lr_end}) must be be smaller than initial lr ({lr0})")
    return LambdaLR(optimizer, warmup_poly(lr0, lr_end, num_warmup_steps, num_training_steps, power), last_epoch)


def warmup_constant(warmup: int):
    """lr(step) / lr0 of the constant schedule (reference: src/utils/lr_sched.py:119-122): linear warm-up, then 1."""
    warmup = int(warmup)

    def factor(step: int) -> float:
        if step < warmup:
            return float(step) / float(max(1.0, warmup))
        return 1.0

    return factor


def get_constant_schedule_with_warmup(optimizer, num_warmup_steps: int, last_epoch: int = -1):
    """What the reference's function of this name defines (lr_sched.py:104-124).  The reference's own factory cannot reach it: it
    passes a `num_training_steps` keyword this function does not take (:134-136) and raises TypeError; `get_lr_scheduler` here
    calls it with the arguments it has."""
    return LambdaLR(optimizer, warmup_constant(num_warmup_steps), last_epoch=last_epoch)


def get_lr_scheduler(config, optimizer, num_warmup_steps, total_steps, min_lr):
    """TRAIN.SCHEDULER -> scheduler (reference: src/utils/lr_sched.py:127-140): "cosine" (the MAE recipe), "poly" (power 2.0, ending
    at `min_lr`) or "constant" (warm-up, then the base rate; `total_steps` and `min_lr` play no part)."""
    kind = config.TRAIN.SCHEDULER
    if kind == "cosine":
        return get_cosine_schedule_with_warmup(optimizer, num_warmup_steps, total_steps, lr_end=min_lr)
    if kind == "poly":
        return get_polynomial_decay_schedule_with_warmup(optimizer, num_warmup_steps, total_steps, lr_end=min_lr, power=2.0, last_epoch=-1)
    if kind == "constant":
        return get_constant_schedule_with_warmup(optimizer, num_warmup_steps)
    raise ValueError(f"Scheduler {kind} not supported")
