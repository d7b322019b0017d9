"""Torch restatement of the models built with `norm_layer=RMSNorm` (src/models/layers.py:11-54; MAE.NORM_LAYER: rmsnorm).

The oracle (oracle/mae_oracle.py) restates the LayerNorm models.  RMSNorm differs in one function and in the parameter set:
    y = x * rsqrt(mean_d(x^2) + 1e-6) * weight        (statistics in fp32, no mean subtraction, no bias; eps 1e-6 at every site)
so `plugged()` swaps the oracle's `_layer_norm` for `rms_norm`, and the state dicts are served through `NoNormBias`, which answers
`None` for the `*norm.bias` keys the RMSNorm models do not have.  The bf16-storage emulation (`O._r`) stays at the oracle's points:
the normalisation's output is rounded, its statistics are not.  tests/golden/rmsnorm.json pins this file to the reference's own
modules (tests/golden/make_golden_rmsnorm.py).
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import lora_ref

RMS_EPS = 1e-6


def rms_norm(x, w, b=None):
    assert b is None, "RMSNorm has no bias"
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + RMS_EPS) * w


def is_norm_bias(name: str) -> bool:
    return name.endswith("norm.bias")


class NoNormBias(dict):
    """State dict of an RMSNorm model as the oracle's forward reads it: the norm biases are absent and read as None."""

    def __missing__(self, key):
        if is_norm_bias(key):
            return None
        raise KeyError(key)


def param_shapes(cfg):
    """O.param_shapes without the norm biases: names, shapes and order of the reference's state dict under RMSNorm."""
    return [t for t in O.param_shapes(cfg) if not is_norm_bias(t[0])]


def make_params(cfg, seed: int = 0):
    """O.make_params without the norm biases (every other tensor keeps the value it has in the LayerNorm model's set)."""
    return {k: v for k, v in O.make_params(cfg, seed).items() if not is_norm_bias(k)}


@contextlib.contextmanager
def plugged(lora: bool = False):
    """Inside the context the oracle's blocks / MAE forward normalise with `rms_norm` (and, with `lora`, run lora_ref's block)."""
    old_ln, old_block = O._layer_norm, O._block
    O._layer_norm = rms_norm
    if lora:
        O._block = lora_ref.block
    try:
        yield
    finally:
        O._layer_norm, O._block = old_ln, old_block


def forward(cfg, p, x, noise, want_inter: bool = False, emulate_bf16: bool = False):
    with plugged():
        return O.forward(cfg, NoNormBias(p), x, noise, want_inter, emulate_bf16=emulate_bf16)


def forward_backward(cfg, params, x, noise, want_inter: bool = False, emulate_bf16: bool = False):
    """O.forward_backward on the RMSNorm parameter set."""
    frozen = {n for n, _, rg in param_shapes(cfg) if not rg}
    p = {k: v.clone().requires_grad_(k not in frozen) for k, v in params.items()}
    loss, pred, mask, inter = forward(cfg, p, x, noise, want_inter, emulate_bf16=emulate_bf16)
    loss.backward()
    grads = {k: v.grad for k, v in p.items() if v.grad is not None}
    return loss.detach(), pred.detach(), mask, grads, ({k: v.detach() for k, v in inter.items()} if inter else None)


def train_step(cfg, st, x, noise, *, base_lr, min_lr, warmup, total, weight_decay, beta1=0.9, beta2=0.95, grad_clip=0.0,
               emulate_bf16: bool = False):
    """O.train_step (per-tensor clip -> AdamW -> cosine LR) on the RMSNorm parameter set."""
    loss, _, _, grads, _ = forward_backward(cfg, st.params, x, noise, emulate_bf16=emulate_bf16)
    norms = O.clip_gradients_(grads, grad_clip) if grad_clip else {}
    lr = base_lr * O.cosine_warmup_lambda(st.step, warmup, total, base_lr, min_lr)
    st.step += 1
    with torch.no_grad():
        for k, g in grads.items():
            if k not in st.exp_avg:
                st.exp_avg[k] = torch.zeros_like(g)
                st.exp_avg_sq[k] = torch.zeros_like(g)
            O.adamw_step_(st.params[k], g, st.exp_avg[k], st.exp_avg_sq[k], st.step, lr, beta1, beta2, 1e-8, weight_decay)
    return float(loss), lr, grads, norms


def vit_forward(p, x, patch_size: int, heads: int, layers: int, emulate_bf16: bool = False):
    """ViT.forward (vit.py:144-173) with RMSNorm: every patch embedded (+ position table), class token, register tokens behind it,
    the blocks (with the adapters when the state dict holds them), final RMSNorm.  Returns (tokens, hidden_states_out)."""
    p = NoNormBias(p)
    lora = any("lora_" in k for k in p)
    old_emu = O._EMU[0]
    O._EMU[0] = bool(emulate_bf16)
    try:
        with plugged(lora=lora):
            B = x.shape[0]
            pe = "patch_embedding.patch_embeddings"
            tok = F.conv3d(O._r(x), O._r(p[pe + ".weight"]), p[pe + ".bias"], stride=patch_size)
            tok = O._r(tok.flatten(2).transpose(-1, -2))
            if "patch_embedding.position_embeddings" in p:
                pos = p["patch_embedding.position_embeddings"]
                if pos.shape[1] != tok.shape[1]:  # a volume of another size: the table is resized (patch_embedding.py:136-144)
                    pos = O.interpolate_pos_embed_3d(pos, round(tok.shape[1] ** (1.0 / 3.0)), 0)
                tok = tok + pos
            h = torch.cat((p["cls_token"].expand(B, -1, -1), tok), dim=1)
            if "register_tokens" in p:
                h = torch.cat((h[:, :1], p["register_tokens"].expand(B, -1, -1), h[:, 1:]), dim=1)
            hidden = []
            for i in range(layers):
                h = O._block(p, f"blocks.{i}", h, heads, None, "")
                hidden.append(h)
            return rms_norm(h, p["norm.weight"]), hidden
    finally:
        O._EMU[0] = old_emu


# the encoder-only fixture cases (tests/golden/make_golden_rmsnorm.py): weights by seed from O.make_vit_params
VIT_CASE = dict(in_chans=1, img_size=16, patch_size=8, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=2,
                qkv_bias=True, batch=2, seed=500, x_seed=91)


def vit_case_params(shapes):
    """Values for a ViT state dict under RMSNorm; the adapters scaled as in lora_ref.case_params."""
    p = O.make_vit_params(shapes, VIT_CASE["seed"])
    for k in p:
        if k.endswith("lora_matrix_A"):
            p[k] = p[k] * 50.0
        if k.endswith("lora_matrix_B"):
            p[k] = p[k] * 0.25
    return p


def vit_case_input():
    c = VIT_CASE
    n = c["batch"] * c["in_chans"] * c["img_size"] ** 3
    return torch.from_numpy(O.hash_uniform(n, c["x_seed"]).astype(np.float32)).view(c["batch"], c["in_chans"], *[c["img_size"]] * 3)


case_loss = lora_ref.case_loss
