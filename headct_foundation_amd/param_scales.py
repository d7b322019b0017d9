"""The two per-parameter rules of the standard ViT fine-tuning recipe, as scale dicts for `_FlatOptimizer.set_scales`
(`HipAdamW`, `HipLion`, `HipSGD`, `HipLamb`, `DinoOptimizer`): layer-wise learning-rate decay (BEiT / MAE fine-tuning: block i of L
trains at lr * decay^(L - i), the embeddings at lr * decay^(L + 1)) and no weight decay on biases, norm scales and the learned
tokens / position table.  The reference has one torch param group (src/utils/optimizers.py:344-379) and neither rule; with torch
they would be param groups, here they are one multiplier per segment of the flat buffer, read by the fused kernel.
"""
from __future__ import annotations

import math
from typing import Dict

NO_DECAY_NAMES = ("cls_token", "register_tokens", "position_embeddings", "weight_g")


def vit_layer_id(name: str, num_layers: int) -> int:
    """Layer of a `ViTBackbone` parameter for layer-wise decay: 0 for the embeddings (`cls_token`, `register_tokens`, the
    backbone's `mask_token`, `patch_embedding.*`), i + 1 for `blocks.i.*` (LoRA adapters included), `num_layers` for everything else (the final `norm.*`)."""
    if name in ("cls_token", "register_tokens", "mask_token") or name.startswith("patch_embedding."):
        return 0
    if name.startswith("blocks."):
        i = int(name.split(".")[1])
        if not 0 <= i < num_layers:
            raise ValueError(f"{name}: block {i} of a backbone with {num_layers} layers")
        return i + 1
    return num_layers


def layer_decay_scales(backbone, decay: float) -> Dict[str, float]:
    """{name: decay ** (num_layers + 1 - vit_layer_id(name))} over a `ViTBackbone`'s parameters: the last block trains at
    lr * decay, the embeddings at lr * decay ** (num_layers + 1).  The classification head sits one layer above and keeps scale 1.
    `decay` lies in (0, 1]; 1.0 gives the empty dict (no scales)."""
    decay = float(decay)
    if not (math.isfinite(decay) and 0.0 < decay <= 1.0):
        raise ValueError(f"layer decay must lie in (0, 1]: got {decay}")
    if decay == 1.0:
        return {}
    num_layers = len(backbone.blocks)
    return {n: decay ** (num_layers + 1 - vit_layer_id(n, num_layers)) for n, _ in backbone.named_parameters()}


def no_decay_scales(module) -> Dict[str, float]:
    """{name: 0.0} for every parameter that is not regularised in the standard recipe: those with ndim <= 1 (biases, LayerNorm /
    RMSNorm / BatchNorm scales and shifts) and, under any prefix, `cls_token`, `register_tokens`, `position_embeddings` and the
    `weight_g` gain of a weight-normalised layer (DINO's last layer; a vector stored as [out, 1]).  Matrices, LoRA matrices
    included, are absent (scale 1).  The `mask_token` of a `ViTBackbone` built with one (iBOT) joins the set as its `cls_token` does; the
    MAE's decoder `mask_token` is none of these and stays decayed."""
    out = {n: 0.0 for n, p in module.named_parameters() if p.ndim <= 1 or n.rsplit(".", 1)[-1] in NO_DECAY_NAMES}
    for prefix, m in module.named_modules():
        if getattr(m, "has_mask_token", False):
            out[(prefix + "." if prefix else "") + "mask_token"] = 0.0
    return out


def describe_scales(scales: Dict[str, tuple]) -> str:
    """One log line for `optimizer.scales()`: the distinct lr scales and the number of tensors at each, and how many tensors are
    not decayed."""
    lr: Dict[float, int] = {}
    for a, _ in scales.values():
        lr[a] = lr.get(a, 0) + 1
    parts = ", ".join(f"{k:.6g} x{v}" for k, v in sorted(lr.items()))
    undecayed = sum(1 for _, w in scales.values() if w == 0.0)
    return f"parameter scales: lr scale {{{parts}}}; {undecayed} of {len(scales)} tensors without weight decay"
