"""Parameter trees shared by the host modules: holders that give parameters the reference's names, the transformer block,
the fixed sine/cosine position table, torch's default Linear / Conv3d initialisation and the plain ViT's tree
(src/models/vit.py), which the forward-only `ViT` and the trainable `ViTBackbone` both register.  No arithmetic of the
hot path runs here."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from ._lib import NORM_LAYERNORM, NORM_RMSNORM, HctError

POS_CODES = {"none": 0, "learnable": 1, "sincos": 2}  # hct_mae_config.pos_embed

LORA_RANK = 128  # SelfAttention hard-codes r=128 for both adapters (attentionblock.py:45-47)


def _to_3tuple(x):
    return tuple(x) if isinstance(x, (list, tuple)) else (x, x, x)


def build_sincos_position_embedding(grid_size, embed_dim: int, spatial_dims: int = 3, temperature: float = 10000.0):
    """Fixed 3-D sine/cosine position table [1, L, D] (contract: src/utils/pos_embed.py:51-78).

    D/6 frequencies 1 / T^(j / (D/6)); token (a, b, c) of the row-major grid gets, in this order, sin and cos of its b, a
    and c coordinate times the frequencies.  (The reference names the axes so that the second grid axis comes first; for
    the cubic grids of this path only that order matters.)  fp32 throughout, one multiply per entry, so the table is
    bit-identical to the reference's (tests/golden/sincos.json)."""
    if spatial_dims != 3:
        raise NotImplementedError(f"Spatial Dimension Size {spatial_dims} Not Implemented!")
    if embed_dim % 6:
        raise AssertionError("Embed dimension must be divisible by 6 for 3D sin-cos position embedding")
    n0, n1, n2 = _to_3tuple(grid_size)
    nfreq = embed_dim // 6
    freq = 1.0 / (temperature ** (torch.arange(nfreq, dtype=torch.float32) / nfreq))
    # coordinates of every token along the three axes of the (n1, n0, n2) meshgrid the reference builds
    axes = [torch.arange(n, dtype=torch.float32) for n in (n1, n0, n2)]
    shape = (n1, n0, n2)
    coords = [ax.reshape([-1 if k == i else 1 for k in range(3)]).expand(shape).reshape(-1) for i, ax in enumerate(axes)]
    parts = []
    for i in (1, 0, 2):
        angle = coords[i][:, None] * freq[None, :]
        parts += [torch.sin(angle), torch.cos(angle)]
    return torch.cat(parts, dim=1).unsqueeze(0)


class _Holder(nn.Module):
    """Parameter container: gives parameters their reference names; never called."""

    def forward(self, *a, **k):  # pragma: no cover
        raise HctError("sub-modules of the HIP models are parameter holders; call the model itself")


class _Affine(_Holder):
    def __init__(self, *wshape, bias_shape=None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(*wshape))
        if bias_shape is not None:
            self.bias = nn.Parameter(torch.empty(*bias_shape))
        else:
            self.register_parameter("bias", None)


class RMSNorm(_Holder):
    """Parameter holder with the signature of the reference's RMSNorm (src/models/layers.py:11-27): one `weight` of ones, no bias.
    Passed as `norm_layer=RMSNorm` it selects y = x * rsqrt(mean(x^2) + eps) * weight (`hct_rmsnorm_*`) for every normalisation of
    the model; the reference builds every instance with eps 1e-6, and so does the HIP path."""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))


def norm_kind(norm_layer, who: str) -> int:
    """hct_mae_config.norm_kind of a `norm_layer` constructor argument; any class but nn.LayerNorm / RMSNorm is refused."""
    if norm_layer is nn.LayerNorm:
        return NORM_LAYERNORM
    if norm_layer is RMSNorm:
        return NORM_RMSNORM
    raise NotImplementedError(f"HIP {who}: norm_layer must be torch.nn.LayerNorm or headct_foundation_amd.RMSNorm, got {norm_layer!r}")


def _norm(d: int, norm_layer=nn.LayerNorm) -> nn.Module:
    """Holder of one normalisation layer's parameters: weight + bias (LayerNorm) or the weight alone (RMSNorm)."""
    return RMSNorm(d) if norm_layer is RMSNorm else _Affine(d, bias_shape=(d,))


class _Lora(_Holder):
    """LoraLinear's parameters (attentionblock.py:6-18): B [out, r] zeros, A [r, in] standard normal, registered in that order."""

    def __init__(self, d: int, r: int):
        super().__init__()
        self.lora_matrix_B = nn.Parameter(torch.zeros(d, r))
        self.lora_matrix_A = nn.Parameter(torch.randn(r, d))


def _block(d: int, m: int, qkv_bias: bool, lora_rank: int = 0, norm_layer=nn.LayerNorm) -> nn.Module:
    """Names of AttentionBlock (attentionblock.py:91-94) + MONAI MLPBlock (linear1/linear2); with `lora_rank` the two adapters of
    SelfAttention behind qkv and proj (attentionblock.py:41-47)."""
    blk = _Holder()
    blk.mlp = _Holder()
    blk.mlp.linear1 = _Affine(m, d, bias_shape=(m,))
    blk.mlp.linear2 = _Affine(d, m, bias_shape=(d,))
    blk.att_norm = _norm(d, norm_layer)
    blk.ffn_norm = _norm(d, norm_layer)
    blk.attn = _Holder()
    blk.attn.qkv = _Affine(3 * d, d, bias_shape=(3 * d,) if qkv_bias else None)
    blk.attn.proj = _Affine(d, d, bias_shape=(d,))
    if lora_rank:
        blk.attn.lora_q = _Lora(d, lora_rank)
        blk.attn.lora_v = _Lora(d, lora_rank)
    return blk


def init_linear_(m: _Affine) -> None:
    """torch's nn.Linear / nn.Conv3d default initialisation: kaiming_uniform_(a=sqrt(5)) weight, bias uniform in
    +-1/sqrt(fan_in) with fan_in = weight[0].numel()."""
    nn.init.kaiming_uniform_(m.weight, a=math.sqrt(5))
    if m.bias is not None:
        bound = 1 / math.sqrt(m.weight[0].numel())
        nn.init.uniform_(m.bias, -bound, bound)


def build_vit_tree(m: nn.Module, in_chans: int, img_size, patch_size, hidden_size: int, mlp_dim: int, num_layers: int, num_heads: int,
                   patch_embed: str, pos_embed: str, classification: bool, num_classes: int, dropout_rate: float, spatial_dims: int,
                   num_register_tokens: int, post_activation: str, qkv_bias: bool, lora: bool, norm_layer, compute_dtype: str,
                   drop_path_rate: float = 0.0):
    """Checks the arguments of the reference's `ViT` (src/models/vit.py:26-142) as far as the HIP path builds them, registers its
    parameters on `m` under the reference's names and in its order (state_dict: own parameters first, then patch_embedding,
    blocks, norm, classification_head) and applies its initialisation (patch_embedding.py:112-130, torch's Linear / Conv3d /
    LayerNorm defaults, vit.py:139-142).  Sets `m.in_chans`, `m.grid`, `m.num_register_tokens`, `m.compute_dtype`, `m.lora`, `m.norm_kind`;
    returns the volume and patch edge (S, P)."""
    if not (0 <= dropout_rate <= 1):
        raise ValueError("dropout_rate should be between 0 and 1.")
    if hidden_size % num_heads != 0:
        raise ValueError("hidden_size should be divisible by num_heads.")
    if dropout_rate == 1:
        raise ValueError("dropout_rate 1 drops every value and has no finite scale 1 / (1 - p): the HIP path takes 0 <= dropout_rate < 1")
    if not (0 <= drop_path_rate <= 1):
        raise ValueError("drop_path_rate should be between 0 and 1.")
    if drop_path_rate == 1:
        raise ValueError("drop_path_rate 1 drops every sample in the last block and has no finite scale 1 / (1 - q): the HIP path takes "
                         "0 <= drop_path_rate < 1")
    if spatial_dims != 3 or patch_embed != "conv":
        raise NotImplementedError(f"HIP {type(m).__name__}: 3-D conv patch embedding")
    m.dropout_rate = float(dropout_rate)  # (the forward-only ViT never trains: its rates are inert)
    m.drop_path_rate = float(drop_path_rate)
    m.norm_kind = norm_kind(norm_layer, type(m).__name__)
    if pos_embed not in POS_CODES:
        raise ValueError(f"pos_embed type {pos_embed} not supported.")
    if compute_dtype not in ("bf16", "fp32"):
        raise ValueError("compute_dtype must be 'bf16' or 'fp32'")
    S = img_size if isinstance(img_size, int) else img_size[0]
    P = patch_size if isinstance(patch_size, int) else patch_size[0]
    if S % P:
        raise ValueError("patch_size should be divisible by img_size.")
    D = hidden_size
    m.in_chans, m.grid, m.num_register_tokens, m.compute_dtype, m.lora = in_chans, S // P, num_register_tokens, compute_dtype, bool(lora)
    L = m.grid ** 3
    m.patch_embedding = _Holder()
    m.patch_embedding.n_patches = L
    m.patch_embedding.position_embeddings = nn.Parameter(torch.zeros(1, L, D)) if pos_embed != "none" else None
    m.patch_embedding.patch_embeddings = _Affine(D, in_chans, P, P, P, bias_shape=(D,))
    m.blocks = nn.ModuleList([_block(D, mlp_dim, qkv_bias, LORA_RANK if lora else 0, norm_layer) for _ in range(num_layers)])
    m.cls_token = nn.Parameter(torch.zeros(1, 1, D))
    m.norm = _norm(D, norm_layer)
    m.register_tokens = nn.Parameter(torch.zeros(1, num_register_tokens, D)) if num_register_tokens else None
    lin = [m.patch_embedding.patch_embeddings]
    if classification:  # vit.py:133-137: Sequential(Linear, Tanh) -> keys `classification_head.0.*`, else a bare Linear
        head = _Affine(num_classes, D, bias_shape=(num_classes,))
        m.classification_head = nn.Sequential(head) if post_activation == "Tanh" else head
        lin.append(head)
    for b_ in m.blocks:
        lin += [b_.attn.qkv, b_.attn.proj, b_.mlp.linear1, b_.mlp.linear2]
    with torch.no_grad():
        pe = m.patch_embedding
        if pos_embed == "learnable":
            nn.init.trunc_normal_(pe.position_embeddings, mean=0.0, std=0.02, a=-2.0, b=2.0)
        elif pos_embed == "sincos":
            pe.position_embeddings.copy_(build_sincos_position_embedding([m.grid] * 3, D, 3))
        for ln in [m.norm] + [b_.att_norm for b_ in m.blocks] + [b_.ffn_norm for b_ in m.blocks]:
            ln.weight.fill_(1.0)
            if getattr(ln, "bias", None) is not None:
                ln.bias.zero_()
        for a in lin:  # the reference's ViT has no custom weight init
            init_linear_(a)
        nn.init.normal_(m.cls_token, std=1e-6)
        if m.register_tokens is not None:
            nn.init.normal_(m.register_tokens, std=1e-6)
    return S, P
