"""Yardstick of patch dropout on the ViT path: the keep count, the stable rank and the input assembly over the kept patches restated in
numpy, and the backbone's training forward restated in plain torch on tests/dropout_ref.block with injected masks (autograd supplies
the gradients).  Nothing here calls the code under test.

Definition.  K = int(L * (1 - rate)) in double.  noise [B, L] is ranked stably per sample (ties to the lower index); sample b keeps the
patches ids_shuffle[b, :K] in that order.  h0[b, 0] = cls, h0[b, 1 + r] = reg[r], h0[b, 1 + R + j] = tok[b*K + j] + pos[ids_shuffle[b, j]].
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import dropout_ref as R


def keep_count(L: int, rate: float) -> int:
    """Python's float is a double: this is the rule itself."""
    K = int(L * (1 - rate))
    if not (0 <= rate < 1) or K < 1:
        raise ValueError(f"rate {rate} keeps {K} of {L} patches")
    return K


def rank(noise: np.ndarray):
    """(ids_shuffle, ids_restore), both [B, L] int64: ids_shuffle[b] lists the positions by rising noise, equal values by rising index
    (a hand-rolled insertion by key (value, index), no library sort); ids_restore is its inverse."""
    noise = np.asarray(noise, dtype=np.float32)
    B, L = noise.shape
    ids_shuffle = np.zeros((B, L), dtype=np.int64)
    ids_restore = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        for l in range(L):
            below = int(np.sum(noise[b] < noise[b, l])) + int(np.sum(noise[b, :l] == noise[b, l]))
            ids_restore[b, l] = below
            ids_shuffle[b, below] = l
    return ids_shuffle, ids_restore


def assemble_fwd(tok, cls, reg, pos, ids_shuffle, B, K):
    """fp32 numpy.  tok [B*K, D] (already fp32 values), cls [D], reg [R, D] or None, pos [L, D] or None -> h0 [B, 1 + R + K, D].  One fp32
    add per patch element."""
    tok = np.asarray(tok, dtype=np.float32)
    D = tok.shape[1]
    Rn = 0 if reg is None else reg.shape[0]
    h0 = np.zeros((B, 1 + Rn + K, D), dtype=np.float32)
    for b in range(B):
        h0[b, 0] = cls
        for r in range(Rn):
            h0[b, 1 + r] = reg[r]
        for j in range(K):
            row = tok[b * K + j]
            h0[b, 1 + Rn + j] = row if pos is None else row + np.asarray(pos, dtype=np.float32)[ids_shuffle[b, j]]
    return h0


def assemble_bwd(dh0, ids_restore, L, K, Rn, dtype=np.float64):
    """dh0 [B, 1 + R + K, D] -> dict(dtok [B*K, D] a copy, dcls [D], dreg [R, D], dpos [L, D]) with the batch sums accumulated in `dtype` in
    batch order, and `abs` = the same sums over |terms| (what the in-order fp32 bound takes)."""
    dh0 = np.asarray(dh0)
    B, _, D = dh0.shape
    out = dict(dtok=dh0[:, 1 + Rn:, :].reshape(B * K, D).copy(), dcls=np.zeros(D, dtype), dreg=np.zeros((Rn, D), dtype), dpos=np.zeros((L, D), dtype))
    ab = dict(dcls=np.zeros(D), dreg=np.zeros((Rn, D)), dpos=np.zeros((L, D)))
    for b in range(B):
        out["dcls"] = (out["dcls"] + dh0[b, 0].astype(dtype)).astype(dtype)
        ab["dcls"] += np.abs(dh0[b, 0].astype(np.float64))
        for r in range(Rn):
            out["dreg"][r] = (out["dreg"][r] + dh0[b, 1 + r].astype(dtype)).astype(dtype)
            ab["dreg"][r] += np.abs(dh0[b, 1 + r].astype(np.float64))
        for l in range(L):
            j = int(ids_restore[b, l])
            if j < K:
                out["dpos"][l] = (out["dpos"][l] + dh0[b, 1 + Rn + j].astype(dtype)).astype(dtype)
                ab["dpos"][l] += np.abs(dh0[b, 1 + Rn + j].astype(np.float64))
    out["abs"] = ab
    return out


def vit_forward_keep(p, x, noise, rate, patch_size, heads, layers, masks):
    """Training forward of the backbone with patch dropout: tokens [B, 1 + R + K, D].  `masks` as in dropout_ref (site 0 acts on the patch
    rows of [B, 1 + R + K, D]; block sites and drop path see that tensor too).  At rate 0 every patch is kept in grid order and this is
    dropout_ref.vit_forward term for term (no noise is looked at).  Under O._EMU the values the bf16 path stores are rounded to bf16 where it
    stores them (the volume, the matrices, the embedded tokens, what dropout_ref.block rounds, the output)."""
    B = x.shape[0]
    r = O._r  # bf16 storage emulation (O._EMU): volumes, weights and the embedded tokens are stored in the compute dtype; identity otherwise
    tok = F.conv3d(r(x), r(p["patch_embedding.patch_embeddings.weight"]), p["patch_embedding.patch_embeddings.bias"], stride=patch_size)
    tok = r(tok.flatten(2).transpose(-1, -2))
    L, D = tok.shape[1], tok.shape[2]
    if "patch_embedding.position_embeddings" in p:
        tok = tok + p["patch_embedding.position_embeddings"]
    if rate > 0:
        K = keep_count(L, rate)
        ids_shuffle, _ = rank(np.asarray(noise, dtype=np.float32))
        keep = torch.from_numpy(ids_shuffle[:, :K])
        tok = torch.gather(tok, 1, keep.unsqueeze(-1).expand(B, K, D))
    Rn = p["register_tokens"].shape[1] if "register_tokens" in p else 0
    z0 = masks.stream(0, (B, 1 + Rn + tok.shape[1], D))
    tok = tok * (z0[:, 1 + Rn:, :] if z0.dim() else z0)
    h = torch.cat((p["cls_token"].expand(B, -1, -1), tok), dim=1)
    if Rn:
        h = torch.cat((h[:, :1], p["register_tokens"].expand(B, -1, -1), h[:, 1:]), dim=1)
    for i in range(layers):
        h = R.block(p, f"blocks.{i}", h, heads, masks, 1 + 4 * i)
    return r(F.layer_norm(h, (h.shape[-1],), p["norm.weight"], p["norm.bias"], 1e-6))


# the second model case: 27 patches, two register tokens, rate 0.4 keeps 16 -> 19 tokens per sample (odd)
KEEP_CASE_27 = dict(in_chans=1, img_size=24, patch_size=8, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=2,
                    qkv_bias=True, batch=3, seed=411, x_seed=79)
RATE_8, RATE_27 = 0.5, 0.4  # dropout_ref.VIT_CASE: L = 8 -> K = 4;  KEEP_CASE_27: L = 27 -> K = 16


def case_noise(case, L, seed=5):
    """Pinned noise [B, L] fp32 with a tie inside the kept set of sample 0 and one across the keep boundary of the last sample."""
    g = torch.Generator().manual_seed(seed + L)
    n = torch.rand(case["batch"], L, generator=g)
    n[0, 1] = n[0, 0] = n[0].min() / 2          # two equal lowest values: positions 0 then 1 lead sample 0's shuffle
    order = torch.argsort(n[-1], stable=True)
    K = keep_count(L, RATE_8 if L == 8 else RATE_27)
    n[-1, order[K]] = n[-1, order[K - 1]]        # rank K - 1 and rank K tie: the lower index is kept
    return n
