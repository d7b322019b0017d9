"""Torch restatement of the reference's attention block with LoRA adapters (src/models/attentionblock.py:51-66 with lora=True), in
the index form the HIP path implements, and a context manager that plugs it into the oracle's ViT (oracle.mae_oracle.vit_forward).

The reference adds lora_q(x) [B, N, D] to q [B, H, N, dh] after a RAW reshape.  Per volume, with U = (x1 A^T) B^T [N, D]:
    block r = n' H + h' of U  (= U[n', h' dh : (h'+1) dh])  is added to  q[head = r // N, token = r % N, :]
and the same for v.  `lora_update` writes that with explicit indices (no reshape of U), so it restates the arithmetic rather than
repeating the reference's expression; tests/golden/lora_vit.json pins it to the reference's own modules.

Rounding points of the bf16 path (O._EMU): T = x1 A^T is stored, the adapters' B / A matrices are working copies, and the q / v
slots are the stored qkv value plus the fp32 product, rounded once.
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import mae_oracle as O


def lora_positions(N: int, H: int):
    """(head, token) that block (n', h') of U lands on, as two [N, H] index tensors."""
    r = torch.arange(N).view(N, 1) * H + torch.arange(H).view(1, H)
    return r // N, r % N


def lora_update(x1: torch.Tensor, A: torch.Tensor, Bm: torch.Tensor, heads: int) -> torch.Tensor:
    """[B, H, N, dh] tensor that the reference adds to q (or v): x1 [B, N, D], A [r, D], Bm [D, r]."""
    B, N, D = x1.shape
    dh = D // heads
    T = O._r(x1 @ O._r(A).T)           # [B, N, r]
    U = T @ O._r(Bm).T                 # [B, N, D]
    head, tok = lora_positions(N, heads)
    out = torch.zeros(B, heads, N, dh, dtype=U.dtype)
    out[:, head, tok] = U.view(B, N, heads, dh)
    return out


def block(p, prefix, h, heads, inter, tag):
    """oracle.mae_oracle._block with the adapters of `prefix`.attn.lora_{q,v} when the state dict holds them."""
    B, N, D = h.shape
    x1 = O._r(O._layer_norm(h, p[f"{prefix}.att_norm.weight"], p[f"{prefix}.att_norm.bias"]))
    qkv = F.linear(x1, O._r(p[f"{prefix}.attn.qkv.weight"]), p.get(f"{prefix}.attn.qkv.bias"))
    qkv = O._r(qkv).reshape(B, N, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    if f"{prefix}.attn.lora_q.lora_matrix_A" in p:
        q = O._r(q + lora_update(x1, p[f"{prefix}.attn.lora_q.lora_matrix_A"], p[f"{prefix}.attn.lora_q.lora_matrix_B"], heads))
        v = O._r(v + lora_update(x1, p[f"{prefix}.attn.lora_v.lora_matrix_A"], p[f"{prefix}.attn.lora_v.lora_matrix_B"], heads))
    att = torch.softmax((q @ k.transpose(-1, -2)) * (D // heads) ** -0.5, dim=-1)
    y = O._r((O._r(att) @ v).transpose(1, 2).contiguous().view(B, N, D))
    y = F.linear(y, O._r(p[f"{prefix}.attn.proj.weight"]), p[f"{prefix}.attn.proj.bias"])
    h = h + y
    x2 = O._r(O._layer_norm(h, p[f"{prefix}.ffn_norm.weight"], p[f"{prefix}.ffn_norm.bias"]))
    u = F.linear(x2, O._r(p[f"{prefix}.mlp.linear1.weight"]), p[f"{prefix}.mlp.linear1.bias"])
    h = h + F.linear(O._r(F.gelu(u)), O._r(p[f"{prefix}.mlp.linear2.weight"]), p[f"{prefix}.mlp.linear2.bias"])
    if inter is not None:
        inter[f"{tag}.out"] = h
    return h


@contextlib.contextmanager
def plugged(emulate_bf16: bool = False):
    """`O.vit_forward` runs this file's block (and, with emulate_bf16, rounds at the bf16 path's storage points) inside the context."""
    old_block, old_emu = O._block, O._EMU[0]
    O._block, O._EMU[0] = block, emulate_bf16
    try:
        yield
    finally:
        O._block, O._EMU[0] = old_block, old_emu


def vit_forward(p, x, patch_size: int, heads: int, layers: int, emulate_bf16: bool = False):
    with plugged(emulate_bf16):
        return O.vit_forward(p, x, patch_size, heads, layers)


LORA_TRAINABLE_KEYS = ("lora", "bias", "embeddings", "norm")


def trainable(name: str) -> bool:
    return any(k in name for k in LORA_TRAINABLE_KEYS)


# the fixture's case (tests/golden/make_golden_lora.py): weights by seed from O.make_vit_params, adapters' B scaled up from the
# matrix scale 0.02 so that the adapters carry a visible part of the output
CASE = dict(in_chans=1, img_size=16, patch_size=8, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=2,
            qkv_bias=True, batch=2, seed=300, x_seed=77)


def case_params(shapes):
    p = O.make_vit_params(shapes, CASE["seed"])
    for k in p:
        if k.endswith("lora_matrix_A"):
            p[k] = p[k] * 50.0   # ~ unit scale, as the reference's randn init
        if k.endswith("lora_matrix_B"):
            p[k] = p[k] * 0.25   # 0.005: non-zero, so that every adapter gradient is exercised
    return p


def case_input():
    c = CASE
    n = c["batch"] * c["in_chans"] * c["img_size"] ** 3
    return torch.from_numpy(O.hash_uniform(n, c["x_seed"]).astype("float32")).view(c["batch"], c["in_chans"], *[c["img_size"]] * 3)


def case_loss(tokens: torch.Tensor) -> torch.Tensor:
    """A scalar that reaches every token with distinct weights (so that every gradient is non-trivial)."""
    w = torch.linspace(-1.0, 1.0, tokens.numel(), dtype=tokens.dtype, device=tokens.device).view_as(tokens)
    return (tokens * w).sum() + 0.5 * (tokens ** 2).sum()
