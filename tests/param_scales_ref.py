"""Shared pieces of tests/test_param_scales_{cpu,gpu}.py: the tiny backbone, the scale lists of the issue, and one update of one
tensor at a scaled rate / decay by the restatements (oracle.mae_oracle.adamw_step_, tests/optim_ref.py).  What "scale" means is
pinned against torch's own param groups in tests/test_param_scales_cpu.py."""
from oracle import mae_oracle as O
from tests import optim_ref as R

KINDS = ("AdamW", "Lion", "SGD", "Lamb")
STATE_KEYS = dict(R.STATE_KEYS, AdamW=("exp_avg", "exp_avg_sq"))
ADAMW_EPS = 1e-8
# the CPU semantics test: six tensors
CPU_LR_SCALES = [1, 0.5, 0.75 ** 3, 0, 2, 1]
CPU_WD_SCALES = [1, 0, 1, 1, 0, 3]


def tiny_vit(lora=False, **kw):
    from headct_foundation_amd.dino_model import ViTBackbone
    return ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=2,
                       qkv_bias=True, lora=lora, **kw)


def new_state(kind, p, momentum=0.9):
    import torch
    if kind == "AdamW":
        return {k: torch.zeros_like(p) for k in STATE_KEYS[kind]}
    return R.new_state(kind, p, momentum)


def apply_scaled_(kind, p, g, state, lr, hp, step, lr_scale=1.0, wd_scale=1.0):
    """One update of one tensor at lr * lr_scale and weight_decay * wd_scale; `step` is 1-based (AdamW's bias correction)."""
    lr_s, wd_s = lr * lr_scale, hp["weight_decay"] * wd_scale
    if kind == "AdamW":
        O.adamw_step_(p, g, state["exp_avg"], state["exp_avg_sq"], step, lr_s, hp["beta1"], hp["beta2"], ADAMW_EPS, wd_s)
        return None
    return R.apply_(kind, p, g, state, lr_s, dict(hp, weight_decay=wd_s))
