"""Yardstick of the dropout path: the counter-based keep mask restated in numpy (DESIGN.md "Dropout", include/headct_hip.h) and
the transformer block, the MAE and the ViT forward restated in plain torch with INJECTED masks (autograd supplies the gradients).
Nothing here calls the code under test.

Mask definition.  Philox4x32-10 keyed by the 64-bit seed (low word, high word).
    streaming sites   element e of the row-major tensor: counter (low32(e >> 2), high32(e >> 2), 0, site), word e & 3
    attention site    score (b, h, q, k): counter (k >> 2, q, b * H + h, site), word k & 3
    keep iff word >= T, T = floor(p * 2^32) of the fp32 value of p; kept values are scaled by 1 / (1 - p), evaluated in fp32.
Sites: 0 the patch embedding; block j (encoder blocks first, then the MAE decoder's) has 1 + 4 j + {0 attention probabilities,
1 proj_drop, 2 drop1 behind the GELU, 3 drop2 behind linear2}.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import lora_ref

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
ATTN, PROJ, DROP1, DROP2 = 0, 1, 2, 3


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays (or scalars) of counter words, two key words -> four uint32 arrays of output."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def threshold(p) -> int:
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def scale(p) -> float:
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def stream_words(seed: int, site: int, n: int) -> np.ndarray:
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10(g & MASK32, g >> np.uint64(32), 0, site, seed & MASK32, (seed >> 32) & MASK32)
    return np.stack(w, axis=1).reshape(-1)[:n]


def stream_mask(seed: int, site: int, shape, p) -> np.ndarray:
    """bool keep mask of a streaming tensor of `shape`."""
    n = int(np.prod(shape))
    return (stream_words(seed, site, n) >= threshold(p)).reshape(shape)


def attn_mask(seed: int, site: int, B: int, H: int, N: int, p) -> np.ndarray:
    """bool keep mask [B, H, N, N] of the attention probabilities."""
    kg = (N + 3) // 4
    bh, q, k4 = np.meshgrid(np.arange(B * H), np.arange(N), np.arange(kg), indexing="ij")
    w = philox4x32_10(k4, q, bh, site, seed & MASK32, (seed >> 32) & MASK32)
    words = np.stack(w, axis=-1).reshape(B * H, N, kg * 4)[:, :, :N]
    return (words >= threshold(p)).reshape(B, H, N, N)


class Masks:
    """Multipliers Z (keep mask x scale) of one seed as torch tensors of `dtype`."""

    def __init__(self, seed: int, p, dtype=torch.float32):
        self.seed, self.p, self.dtype = int(seed), p, dtype

    def stream(self, site: int, shape) -> torch.Tensor:
        return torch.from_numpy(stream_mask(self.seed, site, tuple(shape), self.p)).to(self.dtype) * scale(self.p)

    def attn(self, site: int, B: int, H: int, N: int) -> torch.Tensor:
        return torch.from_numpy(attn_mask(self.seed, site, B, H, N, self.p)).to(self.dtype) * scale(self.p)


class Ones:
    """All-ones masks with scale 1: the restatements then are the model without dropout."""

    def stream(self, site, shape):
        return torch.ones(())

    def attn(self, site, B, H, N):
        return torch.ones(())


def sdpa_dropout(q, k, v, Z):
    """(softmax(q k^T dh^-1/2) o Z) v in the form the kernels use: probabilities rebuilt from the row's log-sum-exp of the UNDROPPED
    scores, the mask applied to them afterwards.  q, k, v [..., N, dh]; Z broadcastable to [..., N, N]."""
    s = (q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5
    lse = torch.logsumexp(s, dim=-1, keepdim=True)
    return (torch.exp(s - lse) * Z) @ v


def block(p, prefix, h, heads, masks, base):
    """oracle.mae_oracle._block (with the LoRA adapters of tests/lora_ref.py where the state dict holds them) and the four dropout
    sites base + {ATTN, PROJ, DROP1, DROP2} (attentionblock.py:61, :65, :97-98; MONAI MLPBlock drop1 / drop2)."""
    B, N, D = h.shape
    r = O._r
    x1 = r(O._layer_norm(h, p[f"{prefix}.att_norm.weight"], p[f"{prefix}.att_norm.bias"]))
    qkv = r(F.linear(x1, r(p[f"{prefix}.attn.qkv.weight"]), p.get(f"{prefix}.attn.qkv.bias")))
    qkv = qkv.reshape(B, N, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    if f"{prefix}.attn.lora_q.lora_matrix_A" in p:
        q = r(q + lora_ref.lora_update(x1, p[f"{prefix}.attn.lora_q.lora_matrix_A"], p[f"{prefix}.attn.lora_q.lora_matrix_B"], heads))
        v = r(v + lora_ref.lora_update(x1, p[f"{prefix}.attn.lora_v.lora_matrix_A"], p[f"{prefix}.attn.lora_v.lora_matrix_B"], heads))
    att = torch.softmax((q @ k.transpose(-1, -2)) * (D // heads) ** -0.5, dim=-1)
    y = r((r(att * masks.attn(base + ATTN, B, heads, N)) @ v).transpose(1, 2).contiguous().view(B, N, D))
    # (bf16 storage emulation, O._EMU: the dropout path stores the outputs of proj and linear2 and the dropped activation in the compute
    #  dtype before the streaming pass masks them / linear2 reads it; r() is the identity otherwise)
    y = r(F.linear(y, r(p[f"{prefix}.attn.proj.weight"]), p[f"{prefix}.attn.proj.bias"]))
    h = h + y * masks.stream(base + PROJ, (B, N, D))
    x2 = r(O._layer_norm(h, p[f"{prefix}.ffn_norm.weight"], p[f"{prefix}.ffn_norm.bias"]))
    u = F.linear(x2, r(p[f"{prefix}.mlp.linear1.weight"]), p[f"{prefix}.mlp.linear1.bias"])
    gact = r(F.gelu(u))
    gact = r(gact * masks.stream(base + DROP1, tuple(gact.shape)))
    y2 = r(F.linear(gact, r(p[f"{prefix}.mlp.linear2.weight"]), p[f"{prefix}.mlp.linear2.bias"]))
    return h + y2 * masks.stream(base + DROP2, (B, N, D))


def mae_forward(cfg, p, x, noise, masks):
    """oracle.mae_oracle._forward with dropout: loss of MaskedAutoencoderViT.forward in training mode.  The embedding's dropout acts on
    the kept patches' rows of the encoder input [B, K + 1, D] (i.i.d. per element, so dropping every patch token before the masking
    picks the kept ones, as the reference does, is the same distribution)."""
    B = x.shape[0]
    D, Dd, L, P = cfg.encoder_embed_dim, cfg.decoder_embed_dim, cfg.num_patches, cfg.patch_size
    r = O._r
    tok = F.conv3d(r(x), r(p["patch_embedding.patch_embeddings.weight"]), p["patch_embedding.patch_embeddings.bias"], stride=P)
    tok = r(tok.flatten(2).transpose(-1, -2))
    if "patch_embedding.position_embeddings" in p:
        tok = tok + p["patch_embedding.position_embeddings"]
    _, ids_restore, ids_keep, mask = O.random_masking_from_noise(cfg, noise)
    xm = torch.gather(tok, 1, ids_keep.unsqueeze(-1).repeat(1, 1, D))
    z0 = masks.stream(0, (B, xm.shape[1] + 1, D))
    xm = xm * (z0[:, 1:, :] if z0.dim() else z0)
    h = torch.cat((p["cls_token"].expand(B, -1, -1), xm), dim=1)
    for i in range(cfg.encoder_depth):
        h = block(p, f"blocks.{i}", h, cfg.encoder_num_heads, masks, 1 + 4 * i)
    latent = r(O._layer_norm(h, p["norm.weight"], p["norm.bias"]))
    y = r(F.linear(latent, r(p["decoder_embed.weight"]), p.get("decoder_embed.bias")))
    mask_tokens = p["mask_token"].repeat(B, L + 1 - y.shape[1], 1)
    y_ = torch.cat([y[:, 1:, :], mask_tokens], dim=1)
    y_ = torch.gather(y_, 1, ids_restore.unsqueeze(-1).repeat(1, 1, Dd))
    y = torch.cat([y[:, :1, :], y_], dim=1)
    y = y + torch.cat((p["decoder_cls_token"].expand(B, -1, -1), p["decoder_pos_embed"].expand(B, -1, -1)), dim=1)
    for i in range(cfg.decoder_depth):
        y = block(p, f"decoder_blocks.{i}", y, cfg.decoder_num_heads, masks, 1 + 4 * (cfg.encoder_depth + i))
    y = r(O._layer_norm(y, p["decoder_norm.weight"], p["decoder_norm.bias"]))
    pred = r(F.linear(y, r(p["decoder_pred.weight"]), p.get("decoder_pred.bias")))[:, 1:, :]
    target = O.patchify(cfg, x)
    if cfg.norm_pix_loss:
        mean = target.mean(dim=-1, keepdim=True)
        var = target.var(dim=-1, keepdim=True)
        target = (target - mean) / (var + 1.0e-6) ** 0.5
    loss = ((pred - target) ** 2).mean(dim=-1)
    return (loss * mask).sum() / mask.sum(), pred


def mae_forward_backward(cfg, params, x, noise, masks):
    """(loss, gradients by name) of the restatement."""
    frozen = {n for n, _, rg in O.param_shapes(cfg) if not rg}
    p = {k: v.clone().requires_grad_(k not in frozen) for k, v in params.items()}
    loss, _ = mae_forward(cfg, p, x, noise, masks)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in p.items() if v.grad is not None}


def vit_forward(p, x, patch_size, heads, layers, masks):
    """oracle.mae_oracle.vit_forward (tokens only) with dropout; the embedding's dropout acts on the patch rows of [B, 1 + R + L, D]."""
    B = x.shape[0]
    tok = F.conv3d(x, p["patch_embedding.patch_embeddings.weight"], p["patch_embedding.patch_embeddings.bias"], stride=patch_size)
    tok = tok.flatten(2).transpose(-1, -2)
    if "patch_embedding.position_embeddings" in p:
        tok = tok + p["patch_embedding.position_embeddings"]
    R = p["register_tokens"].shape[1] if "register_tokens" in p else 0
    z0 = masks.stream(0, (B, 1 + R + tok.shape[1], tok.shape[2]))
    tok = tok * (z0[:, 1 + R:, :] if z0.dim() else z0)
    h = torch.cat((p["cls_token"].expand(B, -1, -1), tok), dim=1)
    if R:
        h = torch.cat((h[:, :1], p["register_tokens"].expand(B, -1, -1), h[:, 1:]), dim=1)
    for i in range(layers):
        h = block(p, f"blocks.{i}", h, heads, masks, 1 + 4 * i)
    return F.layer_norm(h, (h.shape[-1],), p["norm.weight"], p["norm.bias"], 1e-6)


# the cut ViT backbone of the model tests: one register token, two blocks, head dim 16
VIT_CASE = dict(in_chans=1, img_size=16, patch_size=8, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=1,
                qkv_bias=True, batch=2, seed=410, x_seed=78)


def vit_case_input(case=VIT_CASE):
    n = case["batch"] * case["in_chans"] * case["img_size"] ** 3
    return torch.from_numpy(O.hash_uniform(n, case["x_seed"]).astype("float32")).view(case["batch"], case["in_chans"], *[case["img_size"]] * 3)
