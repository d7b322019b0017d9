"""Plain ViT encoder for feature extraction (forward only) on the HIP kernels.

Mirror of `ViT` (src/models/vit.py:26-173) for the downstream use of a pre-trained encoder: same constructor arguments and
parameter names (`cls_token`, `register_tokens`, `patch_embedding.*`, `blocks.N.*`, `norm.*`), `forward(x) -> (x,
hidden_states_out)`: every patch embedded (+ position table, resized trilinearly when the volume is not the constructor's
size, patch_embedding.py:136-144), class token, register tokens, the blocks, final LayerNorm with eps 1e-6 (`norm_layer=RMSNorm`: the reference's RMSNorm at every normalisation, `hct_rmsnorm_fwd`).  Built from the library's primitives (`hct_patch_gather`, `hct_gemm`, `hct_vit_assemble_fwd`,
`hct_layernorm_fwd`, `hct_attention_fwd`, `hct_head_linear`); there is no autograd and no CPU path.  With
`classification=True` the class-token head of vit.py:133-137 / :170-171 (Linear, Tanh unless `post_activation` says
otherwise) is applied and `forward` returns the class scores.  `get_selfattention` / `attention_map` give the attention
probabilities of chosen query tokens (`hct_attention_row_probs`).  `lora=True` adds the reference's rank-128 adapters on q and v
(`hct_lora_qv_fwd`), for feature extraction from a LoRA-fine-tuned checkpoint.  Not built: 2-D inputs, the perceptron patch embedding.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .layers import build_vit_tree


class ViT(nn.Module):
    def __init__(self, in_chans: int, img_size, patch_size, hidden_size: int = 768, mlp_dim: int = 3072, num_layers: int = 12,
                 num_heads: int = 12, patch_embed: str = "conv", pos_embed: str = "learnable", classification: bool = False,
                 num_classes: int = 2, dropout_rate: float = 0.0, spatial_dims: int = 3, num_register_tokens: int = 0,
                 post_activation: str = "Tanh", qkv_bias: bool = False, lora: bool = False, norm_layer=nn.LayerNorm,
                 compute_dtype: str = "bf16", drop_path_rate: float = 0.0) -> None:
        super().__init__()
        self.S, self.P = build_vit_tree(self, in_chans, img_size, patch_size, hidden_size, mlp_dim, num_layers, num_heads, patch_embed,
                                        pos_embed, classification, num_classes, dropout_rate, spatial_dims, num_register_tokens,
                                        post_activation, qkv_bias, lora, norm_layer, compute_dtype, drop_path_rate)
        if pos_embed == "sincos":  # a fixed table here: this module runs forward only
            self.patch_embedding.position_embeddings.requires_grad_(False)
        self.D, self.mlp, self.heads = hidden_size, mlp_dim, num_heads
        self.L = self.grid ** 3
        self.classification = classification
        self.post_activation = post_activation
        self._wcache = {}

    # ---- low-level helpers over the C ABI -------------------------------------------------------
    def _weight(self, p: torch.Tensor, st: int) -> torch.Tensor:
        """[out, in...] weight as a 2-D matrix in the compute dtype (cached bf16 copy, refreshed when the parameter changes)."""
        w2 = p.detach().reshape(p.shape[0], -1)
        if self.compute_dtype == "fp32":
            return w2
        key = id(p)
        ver = (p._version, p.data_ptr())
        hit = self._wcache.get(key)
        if hit is None or hit[0] != ver:
            hit = (ver, _lib.cast_weight(w2, torch.bfloat16, st))
            self._wcache[key] = hit
        return hit[1]

    @staticmethod
    def _linear(a: torch.Tensor, w: torch.Tensor, bias, out_dtype, st: int, **epilogue) -> torch.Tensor:
        out = torch.empty(a.shape[0], w.shape[0], dtype=out_dtype, device=a.device)
        return _lib.gemm(a, w, out, bias=bias, stream=st, **epilogue)

    def _layernorm(self, h: torch.Tensor, ln, eps: float, out_dtype, st: int) -> torch.Tensor:
        """The model's normalisation: LayerNorm with the call site's `eps`, or RMSNorm (eps 1e-6 wherever the reference builds one)."""
        rows, D = h.shape
        y = torch.empty(rows, D, dtype=out_dtype, device=h.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=h.device)
        if self.norm_kind == _lib.NORM_RMSNORM:
            _lib.check(_lib.load().hct_rmsnorm_fwd(h.data_ptr(), ln.weight.data_ptr(), rows, D, ln.eps, y.data_ptr(), _lib.dtype_code(out_dtype),
                                                   rstd.data_ptr(), st), "hct_rmsnorm_fwd")
            return y
        mean = torch.empty(rows, dtype=torch.float32, device=h.device)
        _lib.check(_lib.load().hct_layernorm_fwd(h.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), rows, D, eps, y.data_ptr(),
                                                 _lib.dtype_code(out_dtype), mean.data_ptr(), rstd.data_ptr(), st), "hct_layernorm_fwd")
        return y

    # ---- forward ---------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        out, hidden, _ = self._run(x)
        return out, hidden

    @torch.no_grad()
    def _run(self, x: torch.Tensor, keep_qkv: Optional[int] = None) -> Tuple[torch.Tensor, List[torch.Tensor], Optional[torch.Tensor]]:
        """The whole forward: (what `forward` returns ..., the qkv buffer [B * T, 3 D] of block `keep_qkv` as its attention read it,
        LoRA update included; None when no block is asked for)."""
        if not x.is_cuda or not self.cls_token.is_cuda:
            raise _lib.HctError("ViT (HIP) runs on the GPU: move the module and the input to 'cuda' (no CPU fallback exists)")
        B = x.shape[0]
        S = x.shape[-1] if x.dim() == 5 else -1
        if x.dim() != 5 or tuple(x.shape[1:]) != (self.in_chans, S, S, S) or S <= 0 or S % self.P:
            raise _lib.HctError(f"input shape {tuple(x.shape)} != (B, {self.in_chans}, S, S, S) with S a multiple of {self.P}")
        lib = _lib.load()
        dev = x.device
        with torch.cuda.device(dev):
            st = _lib.stream_ptr()
            tdt = torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32
            dt = _lib.dtype_code(tdt)
            grid = S // self.P
            D, L, R, H = self.D, grid ** 3, self.num_register_tokens, self.heads
            T = 1 + R + L
            # fp16 volumes (the persistent cache's storage type) are read as they are; anything else goes through fp32
            x = x.contiguous() if x.dtype == torch.float16 else x.to(torch.float32).contiguous()
            rows = torch.empty(B * L, self.in_chans * self.P ** 3, dtype=tdt, device=dev)
            # (no index table: every patch in grid order -- the library then moves whole pencils of patches)
            _lib.check(lib.hct_patch_gather(x.data_ptr(), _lib.dtype_code(x), None, B, self.in_chans, S, self.P, L, L, rows.data_ptr(),
                                            dt, st), "hct_patch_gather")
            pe = self.patch_embedding
            tok = self._linear(rows, self._weight(pe.patch_embeddings.weight, st), pe.patch_embeddings.bias, tdt, st)
            h = torch.empty(B * T, D, dtype=torch.float32, device=dev)
            pos = pe.position_embeddings
            if pos is not None and grid != self.grid:
                # a volume of another size: the position table is resized trilinearly for this call, as
                # PatchEmbeddingBlock.forward does (patch_embedding.py:136-144 -> pos_embed.py:164-217)
                resized = torch.empty(1, L, D, dtype=torch.float32, device=dev)
                _lib.check(lib.hct_pos_embed_interp3d(pos.data_ptr(), self.grid, resized.data_ptr(), grid, D, 0, st),
                           "hct_pos_embed_interp3d")
                pos = resized
            _lib.check(lib.hct_vit_assemble_fwd(tok.data_ptr(), dt, self.cls_token.data_ptr(),
                                                self.register_tokens.data_ptr() if R else None,
                                                pos.data_ptr() if pos is not None else None, B, L, R, D, h.data_ptr(), st),
                       "hct_vit_assemble_fwd")
            hidden: List[torch.Tensor] = []
            kept = None
            for i, blk in enumerate(self.blocks):  # AttentionBlock.forward, attentionblock.py:96-99
                xn = self._layernorm(h, blk.att_norm, 1e-5, tdt, st)
                qkv = self._linear(xn, self._weight(blk.attn.qkv.weight, st), getattr(blk.attn.qkv, "bias", None), tdt, st)
                if self.lora:  # q += lora_q(x).reshape(B, H, N, dh), v likewise (attentionblock.py:57-59), in place in qkv
                    lq, lv = blk.attn.lora_q, blk.attn.lora_v
                    r = lq.lora_matrix_A.shape[0]
                    t_buf = torch.empty(B * T, 2 * r, dtype=tdt, device=dev)
                    _lib.check(lib.hct_lora_qv_fwd(xn.data_ptr(), self._weight(lq.lora_matrix_A, st).data_ptr(), self._weight(lv.lora_matrix_A, st).data_ptr(),
                                                   self._weight(lq.lora_matrix_B, st).data_ptr(), self._weight(lv.lora_matrix_B, st).data_ptr(), B, T, H,
                                                   D // H, r, dt, t_buf.data_ptr(), qkv.data_ptr(), st), "hct_lora_qv_fwd")
                if i == keep_qkv:
                    kept = qkv
                o = torch.empty(B * T, D, dtype=tdt, device=dev)
                lse = torch.empty(B * H * T, dtype=torch.float32, device=dev)
                _lib.check(lib.hct_attention_fwd(qkv.data_ptr(), B, T, H, D // H, dt, o.data_ptr(), lse.data_ptr(), st),
                           "hct_attention_fwd")
                h_mid = self._linear(o, self._weight(blk.attn.proj.weight, st), blk.attn.proj.bias, torch.float32, st, residual=h)
                xn = self._layernorm(h_mid, blk.ffn_norm, 1e-5, tdt, st)
                pre = torch.empty(B * T, self.mlp, dtype=tdt, device=dev)
                g = self._linear(xn, self._weight(blk.mlp.linear1.weight, st), blk.mlp.linear1.bias, tdt, st, act=_lib.HCT_ACT_GELU, aux=pre)
                h = self._linear(g, self._weight(blk.mlp.linear2.weight, st), blk.mlp.linear2.bias, torch.float32, st, residual=h_mid)
                hidden.append(h.view(B, T, D))
            out = self._layernorm(h, self.norm, 1e-6, torch.float32, st).view(B, T, D)
            if self.classification:  # classification_head(x[:, 0]), vit.py:170-171
                tanh = self.post_activation == "Tanh"
                head = self.classification_head[0] if tanh else self.classification_head
                ncls = head.weight.shape[0]
                scores = torch.empty(B, ncls, dtype=torch.float32, device=dev)
                _lib.check(lib.hct_head_linear(out.data_ptr(), T * D, 1, None, None, 0.0, head.weight.data_ptr(), head.bias.data_ptr(),
                                               _lib.HCT_ACT_TANH if tanh else _lib.HCT_ACT_NONE, scores.data_ptr(), B, D, ncls, st),
                           "hct_head_linear")
                out = scores
        return out, hidden, kept

    # ---- attention maps --------------------------------------------------------------------------
    @torch.no_grad()
    def get_selfattention(self, x: torch.Tensor, block: int = -1, rows: Sequence[int] = (0,)) -> torch.Tensor:
        """Attention probabilities [B, H, len(rows), T] (fp32) of the query tokens `rows` in block `block` (negative: from the end),
        over all T = 1 + registers + patches keys: softmax(q k^T dh^-1/2) of the qkv the block's attention read
        (`hct_attention_row_probs`; the attention kernels themselves never write probabilities)."""
        from .retrieval import attention_row_probs
        n = len(self.blocks)
        if not -n <= block < n:
            raise _lib.HctError(f"block {block} outside [-{n}, {n})")
        _, _, qkv = self._run(x, keep_qkv=block % n)
        B = x.shape[0]
        T = qkv.shape[0] // B
        return attention_row_probs(qkv, B, T, self.heads, self.D // self.heads, rows)

    @torch.no_grad()
    def attention_map(self, x: torch.Tensor, block: int = -1, upsample: Optional[str] = "trilinear") -> torch.Tensor:
        """What the class token attends to, per head, on the patch grid: the class token's row of `get_selfattention` without the
        class and register columns, as [B, H, g, g, g] in the patch order (gh, gw, gd) of the volume's last three axes.
        `upsample` = 'trilinear' or 'nearest' resizes it to the volume, [B, H, S, S, S] (F.interpolate on the device)."""
        if upsample not in ("trilinear", "nearest", None):
            raise ValueError(f"upsample {upsample!r} not supported ('trilinear', 'nearest' or None)")
        att = self.get_selfattention(x, block, rows=(0,))  # [B, H, 1, T]
        B, S = x.shape[0], x.shape[-1]
        g = S // self.P
        m = att[:, :, 0, 1 + self.num_register_tokens:].reshape(B, self.heads, g, g, g)
        if upsample is None:
            return m
        if upsample == "nearest":
            return F.interpolate(m, size=(S, S, S), mode="nearest")
        return F.interpolate(m, size=(S, S, S), mode="trilinear", align_corners=False)
