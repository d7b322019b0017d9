"""MaskedAutoencoderViT: drop-in host module over the MI355X HIP hot path.

Mirrors the reference's nn.Module contract (src/models/mae.py:20-317): identical constructor kwargs,
`forward(x) -> (loss, None, None)`, parameter names/shapes/registration order (so `state_dict()`,
`load_state_dict()`, `.parameters()` and checkpoints are interchangeable), the reference initialisation
(mae.py:125-148, patch_embedding.py:107-124), `patchify` / `unpatchify`.

All arithmetic runs in libheadct_hip.so.  PyTorch only provides device memory, the RNG draw of the
masking noise (mae.py:206) and the autograd hand-off.  There is no CPU fallback: calling forward on a
CPU tensor, or without the built library, raises.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import HCT_BF16, HCT_F32, HctError
from .flat import FlatPlanModule
from .layers import POS_CODES, _Affine, _Holder, _block, _norm, _to_3tuple, build_sincos_position_embedding, init_linear_, norm_kind


class _MAEFunction(torch.autograd.Function):
    """Autograd hand-off: forward enqueues the native forward, backward the staged native backward, which
    writes straight into the model's flat gradient buffer (`p.grad` are views of it)."""

    @staticmethod
    def forward(ctx, anchor, model, x, noise, train):
        plan = model._plan_for(x.shape[0])
        st = _lib.stream_ptr()
        model._sync_frozen(plan)  # (before the refresh: a change of flags makes it a full one)
        model._ensure_weights_fresh(plan, st)
        # a training forward needs no prediction for the kept patches (the loss drops them, mae.py:298-299): the decoder's tail
        # then runs on the masked patches' rows only, unless the caller asked for the full prediction (`full_pred`)
        # (with dropout active the plan runs every decoder block on every row: cat rows are invalid there -- the masked rows stop being
        #  identical across volumes -- and the compact tail, which would be valid, is unmeasured)
        dropping = model._arm_dropout(plan)
        plan.tail = bool(plan.lib.hct_mae_plan_set_tail(plan.handle, int(train and not dropping and not getattr(model, "full_pred", False))) == 1)
        if not getattr(model, "dec0_table", True):  # (testing: the first decoder block on every row instead of kept rows + one row per position)
            plan.lib.hct_mae_plan_set_dec0(plan.handle, 0)
        # training forward: the loss pass also leaves d(loss)/d(pred) (scaled by 1/world under data parallelism) for the backward
        _lib.check(plan.lib.hct_mae_forward(plan.handle, x.data_ptr(), _lib.dtype_code(x), noise.data_ptr(), plan.loss.data_ptr(),
                                            float(model._grad_prescale) if train else 0.0, st), "hct_mae_forward")
        plan.serial += 1  # the plan's one activation workspace now belongs to this forward
        ctx.model, ctx.plan, ctx.x, ctx.serial = model, plan, x, plan.serial
        return plan.loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        model, plan, x = ctx.model, ctx.plan, ctx.x
        if plan.serial != ctx.serial:
            raise HctError("backward of a stale forward: another forward at the same batch size has overwritten the activation "
                           "workspace (run loss.backward() before the next model(...) call, e.g. before an eval pass)")
        model._run_backward(plan, x, grad_out)
        return None, None, None, None, None


class MaskedAutoencoderViT(FlatPlanModule):
    """Masked Autoencoder with VisionTransformer backbone (HIP / gfx950 implementation)."""

    def __init__(self, input_size: int, patch_size: int, mask_ratio: float, in_chans: int = 1, dropout_rate: float = 0.,
                 spatial_dims: int = 3, patch_embed: str = 'conv', pos_embed: str = 'learnable', encoder_depth: int = 12,
                 encoder_embed_dim: int = 768, encoder_mlp_dim: int = 3072, encoder_num_heads: int = 12,
                 decoder_depth: int = 8, decoder_embed_dim: int = 768, decoder_mlp_dim: int = 3072,
                 decoder_num_heads: int = 16, norm_pix_loss: bool = False, use_bias: bool = False,
                 norm_layer=nn.LayerNorm, compute_dtype: str = "bf16"):
        super().__init__()
        input_size, patch_size = _to_3tuple(input_size), _to_3tuple(patch_size)
        if spatial_dims != 3 or len(set(input_size)) != 1 or len(set(patch_size)) != 1:
            raise HctError("the HIP MAE path supports cubic 3-D volumes and patches")
        if patch_embed != "conv":
            raise ValueError(f"patch_embed type {patch_embed} not supported.")
        if pos_embed not in POS_CODES:
            raise ValueError(f"pos_embed type {pos_embed} not supported.")
        if not (0 <= dropout_rate <= 1):
            raise ValueError("dropout_rate should be between 0 and 1.")
        if dropout_rate == 1:
            raise ValueError("dropout_rate 1 drops every value and has no finite scale 1 / (1 - p): the HIP path takes 0 <= dropout_rate < 1")
        self.norm_kind = norm_kind(norm_layer, "MaskedAutoencoderViT")  # MAE.NORM_LAYER: layernorm / rmsnorm (mae.py:41, :107-117)
        if encoder_embed_dim % encoder_num_heads or decoder_embed_dim % decoder_num_heads:
            raise ValueError("hidden_size should be divisible by num_heads.")
        for m, p in zip(input_size, patch_size):
            if m < p:
                raise ValueError("patch_size should be smaller than img_size.")
            assert m % p == 0, "input size and patch size are not proper"
        if compute_dtype not in ("bf16", "fp32"):
            raise ValueError("compute_dtype must be 'bf16' or 'fp32'")

        self.input_size, self.patch_size = input_size, patch_size
        self.mask_ratio, self.spatial_dims, self.pos_embed, self.norm_pix_loss = mask_ratio, spatial_dims, pos_embed, norm_pix_loss
        self.encoder_embed_dim, self.decoder_embed_dim = encoder_embed_dim, decoder_embed_dim
        self.in_chans = in_chans
        self.out_chans = in_chans * int(np.prod(patch_size))
        self.grid_size = [i // p for i, p in zip(input_size, patch_size)]
        self.compute_dtype = compute_dtype
        num_patches = int(np.prod(self.grid_size))
        self.num_patches = num_patches
        D, Dd, P = encoder_embed_dim, decoder_embed_dim, patch_size[0]

        # ---- parameters: the reference's names and registration order (mae.py:90-121) ----
        self.cls_token = nn.Parameter(torch.zeros(1, 1, D))
        self.decoder_cls_token = nn.Parameter(torch.zeros(1, 1, Dd))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches, Dd), requires_grad=False)
        self.patch_embedding = _Holder()
        self.patch_embedding.n_patches = num_patches  # attribute interpolate_pos_embed reads (patch_embedding.py:96)
        if pos_embed != "none":
            self.patch_embedding.position_embeddings = nn.Parameter(torch.zeros(1, num_patches, D))
        else:
            self.patch_embedding.position_embeddings = None
        self.patch_embedding.patch_embeddings = _Affine(D, in_chans, P, P, P, bias_shape=(D,))
        self.blocks = nn.ModuleList([_block(D, encoder_mlp_dim, use_bias, norm_layer=norm_layer) for _ in range(encoder_depth)])
        self.decoder_blocks = nn.ModuleList([_block(Dd, decoder_mlp_dim, use_bias, norm_layer=norm_layer) for _ in range(decoder_depth)])
        self.norm = _norm(D, norm_layer)
        self.decoder_norm = _norm(Dd, norm_layer)
        self.decoder_embed = _Affine(Dd, D, bias_shape=(Dd,) if use_bias else None)
        self.decoder_pred = _Affine(P ** 3 * in_chans, Dd, bias_shape=(P ** 3 * in_chans,) if use_bias else None)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, Dd))

        self._ccfg = _lib.MaeConfig(
            input_size=input_size[0], patch_size=P, in_chans=in_chans, mask_ratio=float(mask_ratio), pos_embed=POS_CODES[pos_embed],
            encoder_depth=encoder_depth, encoder_embed_dim=D, encoder_mlp_dim=encoder_mlp_dim, encoder_num_heads=encoder_num_heads,
            decoder_depth=decoder_depth, decoder_embed_dim=Dd, decoder_mlp_dim=decoder_mlp_dim, decoder_num_heads=decoder_num_heads,
            norm_pix_loss=int(bool(norm_pix_loss)), use_bias=int(bool(use_bias)), norm_kind=self.norm_kind, dropout_rate=float(dropout_rate))
        self._dt = HCT_BF16 if compute_dtype == "bf16" else HCT_F32
        self.len_keep = int(num_patches * (1 - mask_ratio))  # mae.py:205
        self.full_pred = False  # True: training forwards also predict the kept patches (parity tests, reconstructions)

        self.initialize_weights()
        self._init_dropout(dropout_rate)
        self._init_flat()

    # ------------------------------------------------------------------------------------------
    # initialisation (mae.py:125-148; patch_embedding.py:107-124; Conv3d keeps torch's default)
    # ------------------------------------------------------------------------------------------
    def initialize_weights(self) -> None:
        D, Dd = self.encoder_embed_dim, self.decoder_embed_dim
        pe = self.patch_embedding
        with torch.no_grad():
            conv = pe.patch_embeddings
            init_linear_(conv)  # torch Conv3d.reset_parameters
            if self.pos_embed == "learnable":
                nn.init.trunc_normal_(pe.position_embeddings, mean=0.0, std=0.02, a=-2.0, b=2.0)
            elif self.pos_embed == "sincos":
                pe.position_embeddings.copy_(build_sincos_position_embedding(self.grid_size, D, 3))
            if self.pos_embed == "sincos":
                self.decoder_pos_embed.copy_(build_sincos_position_embedding(self.grid_size, Dd, 3))
            else:
                nn.init.trunc_normal_(self.decoder_pos_embed, std=.02)
            nn.init.trunc_normal_(self.cls_token, std=.02)
            nn.init.trunc_normal_(self.decoder_cls_token, std=.02)
            nn.init.trunc_normal_(self.mask_token, std=.02)
            for name, m in self.named_modules():
                if not isinstance(m, _Affine) or m is conv:
                    continue  # (mae.py:140-148 touches nn.Linear and nn.LayerNorm only: RMSNorm weights keep their ones)
                if m.weight.dim() == 2:  # nn.Linear: xavier_uniform weight, zero bias (mae.py:143-146)
                    nn.init.xavier_uniform_(m.weight)
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
                else:  # nn.LayerNorm (mae.py:147-148)
                    nn.init.constant_(m.bias, 0)
                    nn.init.constant_(m.weight, 1.0)

    # ------------------------------------------------------------------------------------------
    # public API (reference: mae.py:150-192, 303-317)
    # ------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None):
        if not x.is_cuda:
            raise HctError("MaskedAutoencoderViT (HIP) got a CPU tensor: this path has no CPU fallback")
        B = x.shape[0]
        expect = (B, self.in_chans) + tuple(self.input_size)
        if tuple(x.shape) != expect:
            raise HctError(f"input shape {tuple(x.shape)} != {expect} (run-time pos-embed interpolation is out of scope)")
        # fp16 volumes (the persistent cache's storage type, transforms.py:171-178) are consumed as they are: the patch gather
        # and the loss read them directly, which halves the two input passes of a step; anything else is taken as fp32
        x = x.contiguous() if x.dtype == torch.float16 else x.contiguous().float()
        if noise is None:
            noise = torch.rand(B, self.num_patches, device=x.device)  # mae.py:206
        noise = noise.contiguous().float()
        # a freshly zero_grad()-ed model (all .grad None) means the next backward overwrites
        if all(p.grad is None for p in self.parameters()):
            self._grad_overwrite = True
        # grad mode is read here: inside autograd.Function.forward it is always off.  The autograd anchor is a parameter that trains
        # (cls_token may be frozen); with none the loss carries no graph
        anchor = next((p for p in self.parameters() if p.requires_grad), self.cls_token)
        loss = _MAEFunction.apply(anchor, self, x, noise, torch.is_grad_enabled())
        return loss, None, None

    def activation(self, name: str, batch: int) -> torch.Tensor:
        """Named intermediate of the last forward (parity tests): e.g. 'latent', 'dec0.out', 'pred_full', 'mask'."""
        return self._plan_for(batch).activation(name)

    def last_pred(self, batch: int) -> torch.Tensor:
        """pred [B, L, pd] of the last forward (mae.py:272-273), fp32.  A training forward predicts the masked patches only
        (the loss takes no other row, mae.py:298-299) unless `model.full_pred = True`; forwards under `torch.no_grad()` always
        predict every patch."""
        plan = self._plan_for(batch)
        if getattr(plan, "tail", False):
            raise HctError("the last forward was a training forward, which predicts only the masked patches: set model.full_pred = True "
                           "(or run the forward under torch.no_grad()) to get the prediction of every patch")
        full = self.activation("pred_full", batch).float()
        return full.view(batch, self.num_patches + 1, -1)[:, 1:, :]

    def last_pred_masked(self, batch: int):
        """(rows, pred): prediction rows of the masked patches of the last forward and their row index b * (L + 1) + 1 + patch in
        the decoder layout -- available after every forward (in a training forward these are the only rows computed)."""
        plan = self._plan_for(batch)
        n = batch * (self.num_patches - self.len_keep)
        if getattr(plan, "tail", False):
            rows = plan.activation("tail_rows").view(-1)[:n].long()
            return rows, self.activation("pred_full", batch)[:n].float()
        ids_restore = self.activation("ids_restore", batch).long()
        rows = ((ids_restore >= self.len_keep).nonzero()[:, 0] * (self.num_patches + 1) + 1 + (ids_restore >= self.len_keep).nonzero()[:, 1])
        return rows, self.activation("pred_full", batch).float()[rows]

    def last_mask(self, batch: int) -> torch.Tensor:
        return self.activation("mask", batch)

    def reconstruct(self, x: torch.Tensor, passes: Optional[int] = None, seed: int = 0, noise: Optional[torch.Tensor] = None,
                    error_volume: bool = False):
        """Reconstruction, per-patch error map and mask counts of `x` over a covering schedule of masks (reconstruct.py)."""
        from .reconstruct import reconstruct
        return reconstruct(self, x, passes=passes, seed=seed, noise=noise, error_volume=error_volume)

    def patchify(self, x: torch.Tensor) -> torch.Tensor:
        B, Cc = x.shape[:2]
        gh, gw, gd = self.grid_size
        ph, pw, pd = self.patch_size
        x = x.reshape(B, Cc, gh, ph, gw, pw, gd, pd)
        return x.permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, gh * gw * gd, ph * pw * pd * Cc)

    def unpatchify(self, x: torch.Tensor, x_ori: torch.Tensor) -> torch.Tensor:
        """[B, L, pd] -> [B, C, H, W, D] "reconstructed voxels" (mae.py:172-192) via the HIP kernel."""
        B, Cc = x_ori.shape[:2]
        lib = _lib.load()
        if not x.is_cuda:
            raise HctError("unpatchify (HIP) needs a GPU tensor")
        src = x.contiguous()
        dt = HCT_BF16 if src.dtype == torch.bfloat16 else HCT_F32
        if dt == HCT_F32:
            src = src.float()
        vol = torch.empty((B, Cc) + tuple(self.input_size), dtype=torch.float32, device=x.device)
        _lib.check(lib.hct_unpatchify(src.data_ptr(), dt, 0, B, Cc, self.input_size[0], self.patch_size[0], vol.data_ptr(),
                                      _lib.stream_ptr()), "hct_unpatchify")
        return vol
