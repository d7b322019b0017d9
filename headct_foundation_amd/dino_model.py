"""DINO pre-training models on the HIP path (BASELINE config #5): the trainable plain ViT backbone, the projection head and the
multi-crop wrapper.

Reference contracts mirrored here (constructor arguments, parameter names / shapes / registration order, outputs):
  * `ViTBackbone`      -- src/models/vit.py:25-173 (`ViT`): every patch embedded, class token, register tokens, blocks, final
                          LayerNorm eps 1e-6; returns `(x, hidden_states_out)` with `x` = the normalised tokens [B, 1+R+L, D].
                          Forward AND backward run in the native plan (csrc/mae_plan.hip, encoder-only mode).
  * `DINOHead`         -- src/models/dino_head.py:7-41 (use_bn=False, the reference yaml's setting): 3-layer GELU MLP, L2
                          normalisation, weight-normalised prototype layer; composed from hct_gemm + the head kernels of csrc/dino.hip.
  * `MultiCropWrapper` -- src/utils/misc.py:447-484: crops of one resolution are concatenated, one backbone pass per resolution,
                          head on the class-token features; returns {'dino_output': logits}.  With `patch_rows` (iBOT, ibot.py) the
                          masked patch tokens go through the same head call and come back as 'ibot_output'.
PyTorch carries tensors between the native calls and owns the autograd graph edges (two custom Functions); no arithmetic of
the path runs in torch ops.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict

import torch
import torch.nn as nn

from . import _lib
from ._lib import HCT_BF16, HCT_F32, HctError
from .dropout import check_patch_rate, patch_keep_count
from .flat import FlatModule, FlatPlanModule
from .layers import LORA_RANK, POS_CODES, _Affine, _Holder, build_vit_tree


# ================================================================================================
# backbone
# ================================================================================================
class _ViTFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, model, train, noise, masks, *xs):
        # xs: the batch as one tensor or as several equally shaped ones in batch order (crops that are not concatenated first)
        # noise: None, or [B, L] fp32 of a forward that drops patches (the plan of the kept patches runs it)
        # masks: None, or [B, L] uint8 of a forward whose masked patches enter as the mask token (the plan of every patch runs it)
        B = sum(int(t.shape[0]) for t in xs)
        plan = model._plan_for(B) if noise is None else model._plan_for(B, model._ccfg_keep, model.patch_keep)
        st = _lib.stream_ptr()
        model._sync_frozen(plan)  # (before the refresh: a change of flags makes it a full one)
        model._ensure_weights_fresh(plan, st)
        model._arm_dropout(plan)
        ptrs = (C.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
        if masks is not None:
            _lib.check(plan.lib.hct_vit_forward_parts_masked(plan.handle, ptrs, len(xs), _lib.dtype_code(xs[0]), masks.data_ptr(), st),
                       "hct_vit_forward_parts_masked")
        elif noise is None:
            _lib.check(plan.lib.hct_vit_forward_parts(plan.handle, ptrs, len(xs), _lib.dtype_code(xs[0]), st), "hct_vit_forward_parts")
        else:
            _lib.check(plan.lib.hct_vit_forward_parts_keep(plan.handle, ptrs, len(xs), _lib.dtype_code(xs[0]), noise.data_ptr(), st),
                       "hct_vit_forward_parts_keep")
        plan.serial += 1
        ctx.model, ctx.plan, ctx.serial, ctx.nx = model, plan, plan.serial, len(xs)
        lat = plan.activation("latent").view(B, 1 + model.num_register_tokens + plan.len_keep, model.hidden_size)
        return lat.clone()  # the workspace is reused by the next forward of this plan

    @staticmethod
    def backward(ctx, dlat):
        model, plan = ctx.model, ctx.plan
        if plan.serial != ctx.serial:
            raise HctError("backward of a stale ViT forward: another forward at the same batch size has overwritten the activations")
        tdt = torch.bfloat16 if model._dt == HCT_BF16 else torch.float32
        d = dlat.to(tdt).contiguous()
        if model._grad_prescale != 1.0:
            d = d * model._grad_prescale  # data-parallel mean (ddp.py)
        st = _lib.stream_ptr()
        lib = plan.lib
        model._keep_alive = d
        model._run_staged_backward(plan, lambda s: lib.hct_vit_backward_stage(plan.handle, s, d.data_ptr() if s == 0 else None, st),
                                   "hct_vit_backward_stage")
        return (None, None, None, None, None) + (None,) * ctx.nx


class ViTBackbone(FlatPlanModule):
    """Plain ViT (reference `ViT`, src/models/vit.py) with a native forward and backward.  `lora=True` adds the reference's rank-128
    adapters on q and v of every block (`blocks.i.attn.lora_{q,v}.lora_matrix_{B,A}`; csrc/lora.hip); which parameters train is
    decided by `misc.set_requires_grad_false(model, lora=True)`, as in the reference.  `drop_path_rate` (an addition of this build)
    is stochastic depth: in training mode block j drops each residual branch per sample at rate r * j / (num_layers - 1)
    (dropout.py, DESIGN.md "Dropout").  It adds no parameters.  `patch_dropout` (an addition of this build) is the share of patch
    tokens a training-mode forward drops: each sample keeps `patch_keep = int(L * (1 - rate))` patches, chosen by ranking noise as the
    MAE does, in shuffle order, and the blocks run on `1 + R + patch_keep` tokens; evaluation and rate 0 see every patch through the
    plan they always used (DESIGN.md "Patch dropout").  `mask_token=True` (an addition of this build, for the iBOT patch loss) registers
    `mask_token` [1, D], zero-initialised: a forward given `masks` feeds it, plus the position embedding, in the place of every masked
    patch's embedding (DESIGN.md "iBOT").  Without the flag the parameters and their flat layout are those of the reference's ViT."""

    def __init__(self, in_chans: int, img_size, patch_size, hidden_size: int = 768, mlp_dim: int = 3072, num_layers: int = 12,
                 num_heads: int = 12, patch_embed: str = "conv", pos_embed: str = "learnable", classification: bool = False,
                 num_classes: int = 2, dropout_rate: float = 0.0, spatial_dims: int = 3, num_register_tokens: int = 0,
                 post_activation: str = "Tanh", qkv_bias: bool = False, lora: bool = False, norm_layer=nn.LayerNorm,
                 compute_dtype: str = "bf16", drop_path_rate: float = 0.0, patch_dropout: float = 0.0, mask_token: bool = False):
        super().__init__()
        check_patch_rate(patch_dropout)
        if classification:
            raise NotImplementedError("HIP ViTBackbone: classification=False (the DINO / fine-tuning backbone has no classification head)")
        S, P = build_vit_tree(self, in_chans, img_size, patch_size, hidden_size, mlp_dim, num_layers, num_heads, patch_embed, pos_embed,
                              False, num_classes, dropout_rate, spatial_dims, num_register_tokens, post_activation, qkv_bias, lora,
                              norm_layer, compute_dtype, drop_path_rate)
        self.img_size, self.patch_size, self.hidden_size = S, P, hidden_size
        self.has_mask_token = bool(mask_token)
        if self.has_mask_token:
            self.mask_token = nn.Parameter(torch.zeros(1, hidden_size))
        self.num_patches = self.grid ** 3
        self.len_keep = self.num_patches  # every patch is embedded
        self.num_tokens = 1 + num_register_tokens + self.num_patches
        self._ccfg = _lib.MaeConfig(
            input_size=S, patch_size=P, in_chans=in_chans, mask_ratio=0.0, pos_embed=POS_CODES[pos_embed], encoder_depth=num_layers,
            encoder_embed_dim=hidden_size, encoder_mlp_dim=mlp_dim, encoder_num_heads=num_heads, decoder_depth=0,
            decoder_embed_dim=hidden_size, decoder_mlp_dim=mlp_dim, decoder_num_heads=num_heads, norm_pix_loss=0,
            use_bias=int(bool(qkv_bias)), encoder_only=1, num_register_tokens=num_register_tokens, final_norm_eps=1e-6,
            lora_rank=LORA_RANK if lora else 0, norm_kind=self.norm_kind, dropout_rate=float(dropout_rate),
            drop_path_rate=float(drop_path_rate), mask_token=int(self.has_mask_token))
        # patch dropout: a second plan per batch size over the same buffers, created with the rate; rate 0 has no such plan
        self.patch_dropout = float(patch_dropout)
        self.patch_keep = patch_keep_count(self.num_patches, self.patch_dropout)
        self._ccfg_keep = None
        if self.patch_dropout > 0.0:
            self._ccfg_keep = _lib.MaeConfig.from_buffer_copy(self._ccfg)
            self._ccfg_keep.patch_dropout = self.patch_dropout
        self._dt = HCT_BF16 if compute_dtype == "bf16" else HCT_F32
        self._init_dropout(dropout_rate, drop_path_rate, num_layers)
        self._init_flat()

    def forward(self, x, noise=None, masks=None):
        """x: `[B, C, S, S, S]`, or a list / tuple of equally shaped tensors standing for their concatenation along the batch (the
        crops of one resolution, which MultiCropWrapper would otherwise copy into one tensor first).  In training mode with
        `patch_dropout > 0` the output is `[B, 1 + R + patch_keep, D]`: sample b keeps the `patch_keep` patches of lowest `noise[b]`
        (`[B, L]`; default `torch.rand(B, L, device=x.device)`, the device generator's, as MaskedAutoencoderViT.forward draws it).
        Otherwise `noise` is not looked at and nothing is drawn.  `masks` (a backbone built with `mask_token=True`): bool or uint8
        `[B, L]` on the device, honoured whenever given, in training and evaluation alike: patch l of sample b enters the blocks as
        `mask_token + pos[l]` where `masks[b, l]` is set.  The output keeps its shape.  Masks and patch dropout in one forward are refused."""
        xs = list(x) if isinstance(x, (list, tuple)) else [x]
        for t in xs:
            if not t.is_cuda:
                raise HctError("ViTBackbone (HIP) got a CPU tensor: this path has no CPU fallback")
            expect = (t.shape[0], self.in_chans, self.img_size, self.img_size, self.img_size)
            if tuple(t.shape) != expect:
                raise HctError(f"input shape {tuple(t.shape)} != {expect}")
        if any(t.shape[0] != xs[0].shape[0] or t.dtype != xs[0].dtype for t in xs):
            xs = [torch.cat(xs)]  # unequal parts: the copy after all
        xs = [t.contiguous() if t.dtype == torch.float16 else t.contiguous().float() for t in xs]
        if all(p.grad is None for p in self.parameters()):
            self._grad_overwrite = True
        # the autograd anchor is a parameter that trains (cls_token is frozen under the LoRA rule); with none the output carries no graph
        anchor = next((p for p in self.parameters() if p.requires_grad), self.cls_token)
        if self.training and self.patch_keep < self.num_patches:  # (a rate so small that int(L * (1 - rate)) = L drops nothing)
            B = sum(int(t.shape[0]) for t in xs)
            if noise is None:
                noise = torch.rand(B, self.num_patches, device=xs[0].device)
            if tuple(noise.shape) != (B, self.num_patches) or noise.device != xs[0].device:
                raise HctError(f"noise {tuple(noise.shape)} on {noise.device}: patch dropout ranks one fp32 row of {self.num_patches} per volume, "
                               f"({B}, {self.num_patches}) on {xs[0].device}")
            noise = noise.detach().float().contiguous()
        else:
            noise = None
        if masks is not None:
            B = sum(int(t.shape[0]) for t in xs)
            if not self.has_mask_token:
                raise HctError("ViTBackbone: `masks` needs a backbone built with mask_token=True")
            if noise is not None:
                raise HctError("ViTBackbone: patch dropout and masks in one forward are refused (the plan of the kept patches takes no mask)")
            if masks.dtype not in (torch.bool, torch.uint8) or tuple(masks.shape) != (B, self.num_patches) or masks.device != xs[0].device:
                raise HctError(f"masks {tuple(masks.shape)} {masks.dtype} on {masks.device}: one bool / uint8 row of {self.num_patches} per volume, "
                               f"({B}, {self.num_patches}) on {xs[0].device}")
            masks = masks.detach().contiguous()
            masks = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        out = _ViTFunction.apply(anchor, self, torch.is_grad_enabled(), noise, masks, *xs)
        return out, []  # (normalised tokens, hidden_states_out): the per-block states are not materialised on this path


# ================================================================================================
# projection head
# ================================================================================================
class _HeadFunction(torch.autograd.Function):
    """DINOHead.forward / backward over hct_gemm (bias + GELU epilogues, dGELU dgrad, wgrad) and the L2-norm / weight-norm kernels."""

    @staticmethod
    def forward(ctx, anchor, head, x):
        lib = _lib.load()
        st = _lib.stream_ptr()
        dev = x.device
        cd = torch.bfloat16 if head.compute_dtype == "bf16" else torch.float32
        M, D = x.shape
        H, Bn, K = head.hidden_dim, head.bottleneck_dim, head.out_dim
        x = x.to(cd).contiguous()
        W = head._working_weights(cd)
        mk = lambda n, dt=cd: torch.empty(M, n, dtype=dt, device=dev)
        l0, l1, l2 = head._lin
        bn_saved = []
        if not head.use_bn:
            u1, h1, u2, h2 = mk(H), mk(H), mk(H), mk(H)
            # Linear + GELU (exact erf)
            _lib.gemm(x, W[f"mlp.{l0}.weight"], h1, bias=head.mlp[l0].bias, act=_lib.HCT_ACT_GELU, aux=u1, workspace=True)
            _lib.gemm(h1, W[f"mlp.{l1}.weight"], h2, bias=head.mlp[l1].bias, act=_lib.HCT_ACT_GELU, aux=u2, workspace=True)
        else:
            # Linear -> BatchNorm1d -> GELU (dino_head.py:15-21): the Linear's output stays fp32, the statistics are the batch's in
            # training (shared over the ranks like the reference's SyncBatchNorm, main_pretrain_dino.py:183-185) and the running
            # ones in eval; xhat and gelu'(y) are kept for the backward
            u1 = u2 = None
            h1, h2 = mk(H), mk(H)
            inp, width = x, D
            for li, bi, hout in ((l0, head._bn[0], h1), (l1, head._bn[1], h2)):
                u = mk(H, torch.float32)
                _lib.gemm(inp, W[f"mlp.{li}.weight"], u, bias=head.mlp[li].bias, workspace=True)
                bn = head.mlp[bi]
                mean, var, count = head._bn_statistics(lib, bn, u, M, H)
                xhat, dact = mk(H, torch.float32), mk(H, torch.float32)
                _lib.check(lib.hct_bn_gelu_fwd(u.data_ptr(), mean.data_ptr(), var.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                                               float(bn.eps), M, H, hout.data_ptr(), _lib.dtype_code(hout), xhat.data_ptr(), dact.data_ptr(),
                                               st), "hct_bn_gelu_fwd")
                bn_saved.append((xhat, dact, var, count))
                inp, width = hout, H
        z = mk(Bn, torch.float32)
        _lib.gemm(h2, W[f"mlp.{l2}.weight"], z, bias=head.mlp[l2].bias, workspace=True)
        zn, inv_z = mk(Bn), torch.empty(M, dtype=torch.float32, device=dev)
        _lib.check(lib.hct_l2norm_rows_fwd(z.data_ptr(), M, Bn, zn.data_ptr(), _lib.dtype_code(zn), inv_z.data_ptr(), st), "hct_l2norm_rows_fwd")
        wn = torch.empty(K, Bn, dtype=cd, device=dev)
        inv_v = torch.empty(K, dtype=torch.float32, device=dev)
        ll = head.last_layer
        _lib.check(lib.hct_weight_norm_fwd(ll.weight_v.data_ptr(), ll.weight_g.data_ptr(), K, Bn, wn.data_ptr(), _lib.dtype_code(wn),
                                           inv_v.data_ptr(), st), "hct_weight_norm_fwd")
        logits = torch.empty(M, K, dtype=cd, device=dev)
        _lib.gemm(zn, wn, logits, workspace=True)
        # the dgrad of the prototype layer runs as a split-K product over the prototypes when it can (bf16, 16-aligned); only the
        # NT fallback needs W_n^T
        wn_t = None
        if not (cd == torch.bfloat16 and M % 16 == 0 and Bn % 16 == 0):
            wn_t = torch.empty(Bn, K, dtype=cd, device=dev)
            _lib.check(lib.hct_transpose_cast(wn.data_ptr(), _lib.dtype_code(wn), wn_t.data_ptr(), _lib.dtype_code(wn_t), K, Bn, st),
                       "hct_transpose_cast")
        ctx.head, ctx.saved, ctx.wn, ctx.bn_saved = head, (x, u1, h1, u2, h2, zn, inv_z, wn_t, inv_v, W), wn, bn_saved
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        lib = _lib.load()
        st = _lib.stream_ptr()
        head = ctx.head
        x, u1, h1, u2, h2, zn, inv_z, wn_t, inv_v, W = ctx.saved
        dev, cd = x.device, x.dtype
        M, D = x.shape
        H, Bn, K = head.hidden_dim, head.bottleneck_dim, head.out_dim
        dl = dlogits.to(cd).contiguous()
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        ll = head.last_layer
        gv = head._grad_view
        # prototype layer: dzn = dlogits . Wn ;  dWn = dlogits^T . zn  -> weight-norm backward into weight_v (weight_g frozen or not)
        # (as a split-K "TN" product over the 65 536 prototypes: dl^T [K, M] and Wn [K, Bn] -- the NT form is one 80 x 256 output
        #  tile with a 65 536-deep reduction on a single CU, 1.2 ms)
        dzn = f32(M, Bn)
        if wn_t is None:
            dl_t = torch.empty(K, M, dtype=cd, device=dev)
            _lib.check(lib.hct_transpose_cast(dl.data_ptr(), _lib.dtype_code(dl), dl_t.data_ptr(), _lib.dtype_code(dl_t), M, K, st),
                       "hct_transpose_cast")
            _lib.gemm(dl_t, ctx.wn, dzn, trans_a=True, trans_b=False, workspace=True)
        else:
            _lib.gemm(dl, wn_t, dzn, workspace=True)
        dwn = f32(K, Bn)
        _lib.gemm(dl, zn, dwn, trans_a=True, trans_b=False, workspace=True)
        dg = gv("last_layer.weight_g") if ll.weight_g.requires_grad else None
        _lib.check(lib.hct_weight_norm_bwd(dwn.data_ptr(), ll.weight_v.data_ptr(), ll.weight_g.data_ptr(), inv_v.data_ptr(), K, Bn,
                                           gv("last_layer.weight_v").data_ptr(), _lib.ptr(dg), st), "hct_weight_norm_bwd")
        dz = f32(M, Bn)
        _lib.check(lib.hct_l2norm_rows_bwd(dzn.data_ptr(), zn.data_ptr(), _lib.dtype_code(zn), inv_z.data_ptr(), M, Bn, dz.data_ptr(), st),
                   "hct_l2norm_rows_bwd")
        dzc = dz.to(cd)
        ws = torch.empty(max(16, lib.hct_colsum_workspace_bytes(M, max(H, Bn))), dtype=torch.uint8, device=dev)
        colsum = lambda t, n, name: _lib.check(lib.hct_colsum(t.data_ptr(), _lib.dtype_code(t), M, n, n, gv(name).data_ptr(), ws.data_ptr(),
                                                              ws.numel(), st), "hct_colsum")
        l0, l1, l2 = head._lin
        # last Linear of the MLP
        _lib.gemm(dzc, h2, gv(f"mlp.{l2}.weight"), trans_a=True, trans_b=False, workspace=True)
        colsum(dzc, Bn, f"mlp.{l2}.bias")
        du2 = torch.empty(M, H, dtype=cd, device=dev)
        du1 = torch.empty(M, H, dtype=cd, device=dev)
        if not head.use_bn:
            _lib.gemm(dzc, W[f"mlp.{l2}.weight_t"], du2, act=_lib.HCT_ACT_DGELU, aux=u2, workspace=True)        # (dz . W) * gelu'(u2)
        else:
            dh2 = torch.empty(M, H, dtype=cd, device=dev)
            _lib.gemm(dzc, W[f"mlp.{l2}.weight_t"], dh2, workspace=True)
            head._bn_backward(lib, head.mlp[head._bn[1]], dh2, ctx.bn_saved[1], M, H, du2)
        # second Linear
        _lib.gemm(du2, h1, gv(f"mlp.{l1}.weight"), trans_a=True, trans_b=False, workspace=True)
        colsum(du2, H, f"mlp.{l1}.bias")
        if not head.use_bn:
            _lib.gemm(du2, W[f"mlp.{l1}.weight_t"], du1, act=_lib.HCT_ACT_DGELU, aux=u1, workspace=True)
        else:
            dh1 = torch.empty(M, H, dtype=cd, device=dev)
            _lib.gemm(du2, W[f"mlp.{l1}.weight_t"], dh1, workspace=True)
            head._bn_backward(lib, head.mlp[head._bn[0]], dh1, ctx.bn_saved[0], M, H, du1)
        # first Linear
        _lib.gemm(du1, x, gv(f"mlp.{l0}.weight"), trans_a=True, trans_b=False, workspace=True)
        colsum(du1, H, f"mlp.{l0}.bias")
        dx = torch.empty(M, D, dtype=torch.float32, device=dev)
        _lib.gemm(du1, W[f"mlp.{l0}.weight_t"], dx, workspace=True)
        head._attach_grads()
        return None, None, dx


class _BatchNorm(_Holder):
    """Parameters and buffers of nn.BatchNorm1d(n) / SyncBatchNorm under the reference's names (weight, bias, running_mean, running_var,
    num_batches_tracked): a holder, the arithmetic runs in the head's kernels."""

    def __init__(self, n: int, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.eps, self.momentum = eps, momentum
        self.weight = nn.Parameter(torch.ones(n))
        self.bias = nn.Parameter(torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class DINOHead(FlatModule):
    """Reference DINOHead (src/models/dino_head.py) with nlayers=3; use_bn=False (the reference yaml) or True (the default of
    config.py:86: Linear -> BatchNorm1d -> GELU, batch statistics shared over the ranks like the SyncBatchNorm the reference converts
    to, main_pretrain_dino.py:183-185)."""

    def __init__(self, in_dim, out_dim, use_bn=False, norm_last_layer=True, nlayers=3, hidden_dim=2048, bottleneck_dim=256,
                 compute_dtype: str = "bf16"):
        super().__init__()
        if nlayers != 3:
            raise NotImplementedError("HIP DINOHead: nlayers=3 (the reference's head)")
        if in_dim % 4 or hidden_dim % 4 or bottleneck_dim % 4 or out_dim % 4:
            raise HctError("HIP DINOHead: dimensions must be multiples of 4")
        self.in_dim, self.out_dim, self.hidden_dim, self.bottleneck_dim = in_dim, out_dim, hidden_dim, bottleneck_dim
        self.compute_dtype = compute_dtype
        self.use_bn = bool(use_bn)
        lin = lambda o, i: _Affine(o, i, bias_shape=(o,))
        if self.use_bn:  # Sequential indices as in the reference: Linear 0, BatchNorm1d 1, GELU 2, Linear 3, BatchNorm1d 4, GELU 5, Linear 6
            mlp = [lin(hidden_dim, in_dim), _BatchNorm(hidden_dim), _Holder(), lin(hidden_dim, hidden_dim), _BatchNorm(hidden_dim), _Holder(),
                   lin(bottleneck_dim, hidden_dim)]
            self._lin, self._bn = (0, 3, 6), (1, 4)
        else:
            mlp = [lin(hidden_dim, in_dim), _Holder(), lin(hidden_dim, hidden_dim), _Holder(), lin(bottleneck_dim, hidden_dim)]
            self._lin, self._bn = (0, 2, 4), ()
        self.mlp = nn.Sequential(*mlp)  # the Linear / BatchNorm indices carry the parameters, as in the reference's Sequential
        self.last_layer = _Holder()
        self.last_layer.weight_g = nn.Parameter(torch.ones(out_dim, 1), requires_grad=not norm_last_layer)
        self.last_layer.weight_v = nn.Parameter(torch.empty(out_dim, bottleneck_dim))
        with torch.no_grad():
            for i in self._lin:
                nn.init.trunc_normal_(self.mlp[i].weight, std=.02)
                nn.init.constant_(self.mlp[i].bias, 0)
            nn.init.kaiming_uniform_(self.last_layer.weight_v, a=math.sqrt(5))  # nn.Linear default, then weight_norm splits g / v
        self._wver, self._wcache = -1, {}
        self._init_flat()

    def _working_weights(self, cd) -> Dict[str, torch.Tensor]:
        """Linear weights W [out, in] and their transposes W^T [in, out] in the compute dtype: forward products are NT GEMMs with
        W, dgrad products NT GEMMs with W^T (the MFMA kernels take both operands K-contiguous).  Copies are refreshed when the
        masters changed; without a HipAdamW reporting updates they are rebuilt every forward."""
        if self._managed_updates and self._wver == self._weights_version and self._wcache.get("dtype") == cd:
            return self._wcache
        lib, st = _lib.load(), _lib.stream_ptr()
        out = {"dtype": cd}
        for i in self._lin:
            w = self.mlp[i].weight.detach()
            out[f"mlp.{i}.weight"] = _lib.cast_weight(w, cd, st)
            t = torch.empty(w.shape[1], w.shape[0], dtype=cd, device=w.device)
            _lib.check(lib.hct_transpose_cast(w.data_ptr(), HCT_F32, t.data_ptr(), _lib.dtype_code(cd), w.shape[0], w.shape[1], st),
                       "hct_transpose_cast")
            out[f"mlp.{i}.weight_t"] = t
        self._wcache, self._wver = out, self._weights_version
        return out

    def _bn_statistics(self, lib, bn, u: torch.Tensor, M: int, H: int):
        """(mean, var, count) the BatchNorm normalises with.  Training: the batch's (biased variance), over the rows of ALL ranks when a
        process group is up (SyncBatchNorm), and the running statistics move (momentum 0.1, unbiased variance).  Eval: the running ones."""
        import torch.distributed as dist
        if not self.training:
            return bn.running_mean, bn.running_var, float(M)
        st = _lib.stream_ptr()
        if M < 2:
            raise HctError("BatchNorm1d in training mode needs more than one row")
        mean, var = torch.empty(H, device=u.device), torch.empty(H, device=u.device)
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if world == 1:
            _lib.check(lib.hct_batchnorm_stats(u.data_ptr(), M, H, float(bn.momentum), mean.data_ptr(), var.data_ptr(), bn.running_mean.data_ptr(),
                                               bn.running_var.data_ptr(), st), "hct_batchnorm_stats")
            bn.num_batches_tracked += 1
            return mean, var, float(M)
        # equal row counts on every rank (same batch size): global mean = mean of means, E[u^2] likewise (2 x H floats of glue)
        _lib.check(lib.hct_batchnorm_stats(u.data_ptr(), M, H, 0.0, mean.data_ptr(), var.data_ptr(), None, None, st), "hct_batchnorm_stats")
        both = torch.stack([mean, var + mean * mean])
        dist.all_reduce(both)
        both /= world
        gmean, gvar = both[0], (both[1] - both[0] * both[0]).clamp_min_(0.0)
        n = float(M * world)
        with torch.no_grad():
            bn.running_mean.mul_(1 - bn.momentum).add_(gmean, alpha=bn.momentum)
            bn.running_var.mul_(1 - bn.momentum).add_(gvar * (n / (n - 1)), alpha=bn.momentum)
            bn.num_batches_tracked += 1
        return gmean.contiguous(), gvar.contiguous(), n

    def _bn_backward(self, lib, bn, dh: torch.Tensor, saved, M: int, H: int, du: torch.Tensor) -> None:
        """dh = gradient wrt the GELU's output -> du = gradient wrt the Linear's output; the BatchNorm's weight / bias gradients."""
        import torch.distributed as dist
        xhat, dact, var, count = saved
        st = _lib.stream_ptr()
        name = next(f"mlp.{i}" for i in self._bn if self.mlp[i] is bn)
        sums = torch.empty(2, H, device=dh.device)
        _lib.check(lib.hct_bn_gelu_bwd_sums(dh.data_ptr(), _lib.dtype_code(dh), dact.data_ptr(), xhat.data_ptr(), M, H, sums.data_ptr(), st),
                   "hct_bn_gelu_bwd_sums")
        self._grad_view(name + ".bias").copy_(sums[0])    # this rank's rows: the data-parallel gradient mean adds the other ranks'
        self._grad_view(name + ".weight").copy_(sums[1])
        if count > M:  # statistics shared over the ranks: so are the two sums that enter du
            dist.all_reduce(sums)
        _lib.check(lib.hct_bn_gelu_bwd_apply(dh.data_ptr(), _lib.dtype_code(dh), dact.data_ptr(), xhat.data_ptr(), bn.weight.data_ptr(),
                                             var.data_ptr(), float(bn.eps), sums.data_ptr(), float(count), M, H, du.data_ptr(),
                                             _lib.dtype_code(du), st), "hct_bn_gelu_bwd_apply")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise HctError("DINOHead (HIP) got a CPU tensor: this path has no CPU fallback")
        return _HeadFunction.apply(self.mlp[0].weight, self, x)


# ================================================================================================
# multi-crop wrapper
# ================================================================================================
class _GatherRowsFn(torch.autograd.Function):
    """out[r] = row idx[r] of the token matrix (hct_gather_rows; repeats allowed).  Backward: the gradient's rows go back through the inverse
    map `inv` (row of `out` that holds token row t, -1 for none) -- one more hct_gather_rows, which zero-fills and scatters in one pass."""

    @staticmethod
    def forward(ctx, tokens, idx, inv):
        D = tokens.shape[-1]
        src = tokens.contiguous()
        out = torch.empty(idx.numel(), D, dtype=tokens.dtype, device=tokens.device)
        _lib.check(_lib.load().hct_gather_rows(src.data_ptr(), idx.data_ptr(), idx.numel(), D * src.element_size(), out.data_ptr(), _lib.stream_ptr()),
                   "hct_gather_rows")
        ctx.inv, ctx.shape, ctx.dtype = inv, tuple(tokens.shape), tokens.dtype
        return out

    @staticmethod
    def backward(ctx, d):
        d = d.contiguous()
        dtok = torch.empty(ctx.shape, dtype=d.dtype, device=d.device)
        _lib.check(_lib.load().hct_gather_rows(d.data_ptr(), ctx.inv.data_ptr(), ctx.inv.numel(), ctx.shape[-1] * d.element_size(), dtok.data_ptr(),
                                               _lib.stream_ptr()), "hct_gather_rows")
        return dtok.to(ctx.dtype), None, None


class _SplitRowsFn(torch.autograd.Function):
    """(x[:n_a], x[n_a:n_a + n_b]) of a row matrix whose remaining rows are padding.  Backward: one buffer of x's shape, the two gradients
    copied into their rows and an exact 0 into the pad rows -- copies only, where two slice backwards would fill and add two such buffers."""

    @staticmethod
    def forward(ctx, x, n_a, n_b):
        ctx.n_a, ctx.n_b, ctx.rows = n_a, n_b, x.shape[0]
        return x[:n_a], x[n_a:n_a + n_b]

    @staticmethod
    def backward(ctx, ga, gb):
        n_a, n_b = ctx.n_a, ctx.n_b
        dx = torch.empty((ctx.rows,) + tuple(ga.shape[1:]), dtype=ga.dtype, device=ga.device)
        dx[:n_a].copy_(ga)
        dx[n_a:n_a + n_b].copy_(gb)
        dx[n_a + n_b:].zero_()
        return dx, None, None


class MultiCropWrapper(nn.Module):
    """One backbone pass per crop resolution over the concatenated crops, head on the class-token features (misc.py:447-484).
    `return_cls=True` (an addition of this build) also returns 'cls_tokens': the view of the class-token rows that feeds the head, for a
    loss on the features themselves (dino.koleo_loss); autograd adds its gradient to the head's before the backbone's backward."""

    def __init__(self, backbone, head, return_cls: bool = False):
        super().__init__()
        self.backbone, self.head = backbone, head
        self.return_cls = bool(return_cls)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=False)
        for m in (self.backbone, self.head):  # the children's fp32 masters changed underneath their bf16 working copies
            if hasattr(m, "mark_weights_updated"):
                m.mark_weights_updated()
        return out

    def head_rows(self, n_samples: int, patch_rows, device):
        """Index tensors of the head's input rows for the iBOT pass, built on the host from `patch_rows` (host int32 rows of the masked
        patch tokens inside the token matrix, `ibot.ibot_rows_and_weights`): (idx [Mh], inv [n_samples * T1]) on the device.  The
        class-token rows come first, the patch rows behind them, then repeats of the last real row up to a multiple of 16 rows."""
        import numpy as np
        from .ibot import pad_head_rows
        T1 = self.backbone.num_tokens
        rows = np.asarray(patch_rows.cpu() if isinstance(patch_rows, torch.Tensor) else patch_rows, dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= n_samples * T1 or np.any(rows % T1 == 0)):
            raise HctError(f"patch_rows must be rows of patch or register tokens inside the [{n_samples} * {T1}] token matrix")
        real = np.concatenate((np.arange(n_samples, dtype=np.int64) * T1, rows))
        idx = np.concatenate((real, np.full(pad_head_rows(real.size) - real.size, real[-1], dtype=np.int64))).astype(np.int32)
        inv = np.full(n_samples * T1, -1, dtype=np.int32)
        inv[real] = np.arange(real.size, dtype=np.int32)
        return torch.from_numpy(idx).to(device, non_blocking=True), torch.from_numpy(inv).to(device, non_blocking=True)

    def forward(self, x, masks=None, patch_rows=None):
        """`masks` (bool / uint8 `[n_g, L]` or `[B_total, L]` on the device; a backbone with `mask_token=True`): handed to the backbone, rows
        behind the first n_g padded with "nothing masked".  `patch_rows` (host int32 `[M]`): the masked patch tokens' rows are gathered
        behind the class-token rows, the shared head runs once on all of them (row count padded to a multiple of 16 with repeats of a
        real row, which no loss reads), and the output gains 'ibot_output' `[M, K]`."""
        if not isinstance(x, list):
            x = [x]
        if (masks is not None or patch_rows is not None) and (len({int(t.shape[-1]) for t in x}) != 1 or not hasattr(self.backbone, "_plan_for")):
            raise HctError("MultiCropWrapper: masks / patch_rows need the native backbone and crops of one resolution")
        if patch_rows is not None and getattr(self.head, "use_bn", False):
            raise ValueError("the iBOT patch loss runs class and patch rows through one head: with DINO.USE_BN True the batch statistics "
                             "would mix them")
        if masks is not None or patch_rows is not None:
            n = sum(int(t.shape[0]) for t in x)
            if masks is not None and masks.shape[0] < n:  # local crops are never masked
                masks = torch.cat((masks, torch.zeros(n - masks.shape[0], masks.shape[1], dtype=masks.dtype, device=masks.device)))
            tokens = self.backbone(x, masks=masks)[0]
            out = {}
            if patch_rows is None:
                cls = tokens[:, 0, :]
                out['dino_output'] = self.head(cls)
            else:
                idx, inv = self.head_rows(n, patch_rows, tokens.device)
                logits = self.head(_GatherRowsFn.apply(tokens, idx, inv))
                out['dino_output'], out['ibot_output'] = _SplitRowsFn.apply(logits, n, len(patch_rows))
                cls = tokens[:, 0, :]
            if self.return_cls:
                out['cls_tokens'] = cls
            return out
        sizes = [int(t.shape[-1]) for t in x]
        feats, start = [], 0
        while start < len(x):  # runs of consecutive crops with the same last dimension (torch.unique_consecutive in the reference)
            end = start
            while end < len(x) and sizes[end] == sizes[start]:
                end += 1
            out = self.backbone(x[start:end] if hasattr(self.backbone, "_plan_for") else torch.cat(x[start:end]))  # the native backbone reads the crops in place
            feats.append(out[0] if isinstance(out, tuple) else out)
            start = end
        tokens = torch.cat(feats)
        if not self.return_cls:
            return {'dino_output': self.head(tokens[:, 0, :])}
        cls = tokens[:, 0, :]
        return {'dino_output': self.head(cls), 'cls_tokens': cls}
