"""Classification heads over ViT features on the HIP kernels: eval mode, linear probing and fine-tuning.

Mirrors of `LinearClassifier` and `AttentionClassifier` (src/models/classifier.py:7-99): same constructor arguments,
parameter and buffer names (`bn.running_mean`, `bn.running_var`, `bn.num_batches_tracked`, `linear.*`; `bn1`, `bn2`, `wkv.*`,
`cls_token`), so a head trained with the reference loads with `load_state_dict`.  In eval mode the BatchNorm layers use their
running statistics.  In training mode they use the batch's (and move the running statistics, momentum 0.1), as
engine_downstream.py:70-117 runs them:
  * `LinearClassifier` on detached features (linear probing, TRAIN.LOCK) gives the gradients of `linear.*`; built with
    `feature_grad=True` it also returns the gradient with respect to the features (fine-tuning the backbone through the head).
    It takes `[B, dim]` features or the backbone's `[B, T, dim]` tokens, of which it classifies the class token (index 0): the
    feature gradient then lands in the class-token row of a `[B, T, dim]` gradient.
  * `AttentionClassifier` in training mode: batch statistics for `bn1` (over B*N token rows) and `bn2` (over B*Q rows), the
    gradients of `cls_token`, `wkv.*`, `linear.*` and of the tokens.
Both heads keep their parameters and gradients in flat fp32 buffers (`flat.FlatModule`, as DINOHead), so `HipAdamW` and
`clip_grad_norm_` drive them; gradients accumulate into `.grad` as autograd's do (a backward after `zero_grad` writes them).
The linear head reads an fp32 copy of its B x D features (the probing kernels, bit-identical to linear probing before
fine-tuning existed); the attentive head reads the backbone's tokens in their own dtype (fp32 or bf16).  No CPU path; no
arithmetic of the path runs in torch ops.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from .flat import FlatModule
from .layers import _Affine, _Holder, init_linear_


class _BatchNormStats(_Holder):
    """Buffers of nn.BatchNorm1d(dim, affine=False): running_mean, running_var, num_batches_tracked."""

    def __init__(self, dim: int):
        super().__init__()
        self.eps = 1e-6
        self.register_buffer("running_mean", torch.zeros(dim))
        self.register_buffer("running_var", torch.ones(dim))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


def _require_eval_cuda(mod: nn.Module, x: torch.Tensor, what: str) -> None:
    if not x.is_cuda or not mod.linear.weight.is_cuda:
        raise _lib.HctError(f"{what} (HIP) runs on the GPU in train and eval mode: move the module and the input to 'cuda' "
                            "(no CPU fallback exists)")


def _as_read(t: torch.Tensor) -> torch.Tensor:
    """The features as the kernels read them: fp32 or bf16 in place (unit stride along the channels), anything else as fp32."""
    if t.dtype not in (torch.float32, torch.bfloat16):
        t = t.to(torch.float32)
    return t if t.stride(-1) == 1 else t.contiguous()


def _grad_buffer(head: FlatModule):
    """(buffer, accumulate): where a backward writes the head's parameter gradients.  With no gradient held (after zero_grad)
    that is the flat gradient buffer itself; otherwise a zeroed scratch buffer, added to it by `_finish_grads` -- autograd's
    accumulation into `.grad`."""
    acc = any(p.grad is not None for p in head.parameters() if p.requires_grad)
    return (torch.zeros_like(head._flat_grad) if acc else head._flat_grad), acc


def _finish_grads(head: FlatModule, lib, buf: torch.Tensor, acc: bool) -> None:
    if acc:
        _lib.check(lib.hct_add_f32(head._flat_grad.data_ptr(), buf.data_ptr(), buf.numel(), _lib.stream_ptr(buf.device)), "hct_add_f32")
    head._attach_grads()


def _bn_train_stats(lib, bn, x: torch.Tensor, ldx: int, rows: int, D: int):
    """Batch mean / biased variance of `rows` rows (row stride ldx) + the running update (momentum 0.1)."""
    if rows < 2:
        raise _lib.HctError("BatchNorm1d in training mode needs more than one row (B * rows per sample > 1)")
    dev = x.device
    mean, var = torch.empty(D, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
    ws = torch.empty(max(16, lib.hct_bn_rows_workspace_bytes(rows, D)), dtype=torch.uint8, device=dev)
    _lib.check(lib.hct_bn_stats_rows(x.data_ptr(), _lib.dtype_code(x), ldx, rows, D, 0.1, mean.data_ptr(), var.data_ptr(),
                                     bn.running_mean.data_ptr(), bn.running_var.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _lib.stream_ptr(dev)), "hct_bn_stats_rows")
    bn.num_batches_tracked += 1
    return mean, var


class _LinearHeadFn(torch.autograd.Function):
    """Training-mode LinearClassifier: BatchNorm1d batch statistics (+ running update), Linear, on an fp32 copy of the B x D
    features (the arithmetic and kernels of linear probing: hct_batchnorm_stats, hct_head_linear, hct_head_linear_wgrad).
    Backward: the gradients of linear.* into the head's flat buffer and, when the features require one, the gradient with
    respect to them (hct_bn_bwd_input with the Linear's dgrad fused in), in the features' dtype."""

    @staticmethod
    def forward(ctx, anchor, head, x, tokens):
        # x: [B, D] features (tokens None), or tokens [B, T, D] (x None) whose class-token row (index 0) is classified
        lib = _lib.load()
        src = tokens if tokens is not None else x
        feat = src[:, 0, :] if tokens is not None else src
        xf = feat.detach().to(torch.float32).contiguous()
        B, D = xf.shape
        W, b = head.linear.weight, head.linear.bias
        ncls = W.shape[0]
        dev = xf.device
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            mean = torch.empty(D, dtype=torch.float32, device=dev)
            var = torch.empty(D, dtype=torch.float32, device=dev)
            _lib.check(lib.hct_batchnorm_stats(xf.data_ptr(), B, D, 0.1, mean.data_ptr(), var.data_ptr(), head.bn.running_mean.data_ptr(),
                                               head.bn.running_var.data_ptr(), st), "hct_batchnorm_stats")
            head.bn.num_batches_tracked += 1
            out = torch.empty(B, ncls, dtype=torch.float32, device=dev)
            _lib.check(lib.hct_head_linear(xf.data_ptr(), D, 1, mean.data_ptr(), var.data_ptr(), head.bn.eps, W.data_ptr(), b.data_ptr(),
                                           _lib.HCT_ACT_NONE, out.data_ptr(), B, D, ncls, st), "hct_head_linear")
        ctx.head = head
        ctx.src_meta = (tuple(src.shape), src.dtype, tokens is not None)
        ctx.save_for_backward(xf, mean, var)
        return out

    @staticmethod
    def backward(ctx, dlogits):
        head = ctx.head
        xf, mean, var = ctx.saved_tensors
        shape, dtype, is_tokens = ctx.src_meta
        lib = _lib.load()
        B, D = xf.shape
        W = head.linear.weight
        ncls = W.shape[0]
        dl = dlogits.to(torch.float32).contiguous()
        dev = xf.device
        dsrc = None
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            buf, acc = _grad_buffer(head)
            _lib.check(lib.hct_head_linear_wgrad(xf.data_ptr(), mean.data_ptr(), var.data_ptr(), head.bn.eps, dl.data_ptr(), B, D, ncls,
                                                 head._grad_view("linear.weight", buf).data_ptr(),
                                                 head._grad_view("linear.bias", buf).data_ptr(), st), "hct_head_linear_wgrad")
            if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
                gdt = dtype if dtype in (torch.float32, torch.bfloat16) else torch.float32  # autograd casts to the input's dtype
                if is_tokens:  # a fresh contiguous [B, T, D]: only the class-token rows receive a gradient
                    dsrc = torch.zeros(shape, dtype=gdt, device=dev)
                else:
                    dsrc = torch.empty(B, D, dtype=gdt, device=dev)
                ldo = dsrc.stride(0)
                assert dsrc.is_contiguous() and (B - 1) * ldo + D <= dsrc.numel()
                ws = torch.empty(lib.hct_bn_rows_workspace_bytes(B, D) + 8 * D, dtype=torch.uint8, device=dev)
                _lib.check(lib.hct_bn_bwd_input(xf.data_ptr(), _lib.HCT_F32, D, mean.data_ptr(), var.data_ptr(), head.bn.eps, None, 0,
                                                dl.data_ptr(), W.data_ptr(), 1, ncls, B, D, dsrc.data_ptr(), _lib.dtype_code(dsrc), ldo,
                                                ws.data_ptr(), ws.numel(), st), "hct_bn_bwd_input")
            _finish_grads(head, lib, buf, acc)
        if is_tokens:
            return None, None, None, dsrc
        return None, None, dsrc, None


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        lib = _lib.load()
        B, ncls = logits.shape
        with torch.cuda.device(logits.device):
            loss = torch.empty((), dtype=torch.float32, device=logits.device)
            _lib.check(lib.hct_softmax_xent(logits.data_ptr(), target.data_ptr(), B, ncls, None, loss.data_ptr(), None,
                                            _lib.stream_ptr(logits.device)), "hct_softmax_xent")
        ctx.save_for_backward(logits, target)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target = ctx.saved_tensors
        lib = _lib.load()
        B, ncls = logits.shape
        dloss = dloss.to(torch.float32).contiguous()
        with torch.cuda.device(logits.device):
            dlogits = torch.empty_like(logits)
            _lib.check(lib.hct_softmax_xent(logits.data_ptr(), target.data_ptr(), B, ncls, dloss.data_ptr(), None, dlogits.data_ptr(),
                                            _lib.stream_ptr(logits.device)), "hct_softmax_xent")
        return dlogits, None


def cross_entropy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """nn.CrossEntropyLoss() of main_downstream.py:214 (mean reduction, class-index targets, no weights) on the HIP kernel.
    A target outside [0, num_classes) makes the loss NaN (the reference's loop stops on a non-finite loss)."""
    if not logits.is_cuda or logits.dim() != 2 or target.shape != logits.shape[:1]:
        raise _lib.HctError("cross_entropy (HIP): logits [B, C] on 'cuda' and class-index targets [B] expected (no CPU fallback exists)")
    return _CrossEntropyFn.apply(logits.to(torch.float32).contiguous(), target.to(device=logits.device, dtype=torch.int64).contiguous())


class _SoftCrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, lam, smoothing):
        lib = _lib.load()
        B, ncls = logits.shape
        with torch.cuda.device(logits.device):
            loss = torch.empty((), dtype=torch.float32, device=logits.device)
            _lib.check(lib.hct_mix_xent(logits.data_ptr(), target.data_ptr(), _lib.ptr(lam), smoothing, B, ncls, None, loss.data_ptr(), None,
                                        _lib.stream_ptr(logits.device)), "hct_mix_xent")
        ctx.lam, ctx.smoothing = lam, smoothing
        ctx.save_for_backward(logits, target)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target = ctx.saved_tensors
        lib = _lib.load()
        B, ncls = logits.shape
        dloss = dloss.to(torch.float32).contiguous()
        with torch.cuda.device(logits.device):
            dlogits = torch.empty_like(logits)
            _lib.check(lib.hct_mix_xent(logits.data_ptr(), target.data_ptr(), _lib.ptr(ctx.lam), ctx.smoothing, B, ncls, dloss.data_ptr(), None,
                                        dlogits.data_ptr(), _lib.stream_ptr(logits.device)), "hct_mix_xent")
        return dlogits, None, None, None


def soft_cross_entropy(logits: torch.Tensor, target: torch.Tensor, lam: Optional[torch.Tensor] = None, smoothing: float = 0.0) -> torch.Tensor:
    """Cross-entropy against the soft target of the fine-tuning recipe (an addition of this build) on the HIP kernel hct_mix_xent:
    row b is scored against lam[b] * s(target[b]) + (1 - lam[b]) * s(target[B - 1 - b]), s the one-hot row smoothed by `smoothing`
    (timm's mixup_target; torch's label_smoothing).  The soft target is never materialised.  lam None: no mixing; with
    smoothing 0 as well this is `cross_entropy`'s value, except that a target outside [0, num_classes) matches no class instead
    of making the loss NaN."""
    if not logits.is_cuda or logits.dim() != 2 or target.shape != logits.shape[:1]:
        raise _lib.HctError("soft_cross_entropy (HIP): logits [B, C] on 'cuda' and class-index targets [B] expected (no CPU fallback exists)")
    smoothing = float(smoothing)
    if not 0.0 <= smoothing < 1.0:
        raise ValueError(f"smoothing must lie in [0, 1): got {smoothing}")
    if lam is not None:
        if lam.numel() != logits.shape[0]:
            raise _lib.HctError(f"soft_cross_entropy (HIP): lam needs one entry per row ({logits.shape[0]}), not {lam.numel()}")
        lam = lam.detach().to(device=logits.device, dtype=torch.float32).contiguous()
    return _SoftCrossEntropyFn.apply(logits.to(torch.float32).contiguous(), target.to(device=logits.device, dtype=torch.int64).contiguous(),
                                     lam, smoothing)


def _sigmoid_bce(lib, logits, target, pos_weight, dloss, loss, dlogits):
    B, T = logits.shape
    ws = torch.empty(lib.hct_sigmoid_bce_workspace_bytes(B, T), dtype=torch.uint8, device=logits.device)
    _lib.check(lib.hct_sigmoid_bce(logits.data_ptr(), target.data_ptr(), _lib.ptr(pos_weight), B, T, _lib.ptr(dloss), _lib.ptr(loss), None,
                                   _lib.ptr(dlogits), ws.data_ptr(), ws.numel(), _lib.stream_ptr(logits.device)), "hct_sigmoid_bce")


class _BceWithLogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, pos_weight):
        lib = _lib.load()
        with torch.cuda.device(logits.device):
            loss = torch.empty((), dtype=torch.float32, device=logits.device)
            _sigmoid_bce(lib, logits, target, pos_weight, None, loss, None)
        ctx.pos_weight = pos_weight
        ctx.save_for_backward(logits, target)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target = ctx.saved_tensors
        lib = _lib.load()
        dloss = dloss.to(torch.float32).contiguous()
        with torch.cuda.device(logits.device):
            dlogits = torch.empty_like(logits)
            _sigmoid_bce(lib, logits, target, ctx.pos_weight, dloss, None, dlogits)
        return dlogits, None, None


def bce_with_logits(logits: torch.Tensor, target: torch.Tensor, pos_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Multi-label loss (TRAIN.LABEL_NAMES; an addition of this build) on the HIP kernel: the mean over the valid entries of the
    binary cross-entropy of sigmoid(logits [B, T]) against target [B, T] in [0, 1], where a negative target marks a missing label
    that adds nothing to loss or gradient; `pos_weight` [T] scales the positive term of its label.  With no valid entry at all
    the loss is 0 (torch's would be NaN)."""
    if not logits.is_cuda or logits.dim() != 2:
        raise _lib.HctError("bce_with_logits (HIP): logits [B, T] on 'cuda' and targets [B, T] expected (no CPU fallback exists)")
    if target.shape != logits.shape:
        raise _lib.HctError(f"bce_with_logits (HIP): target shape {tuple(target.shape)} differs from the logits' {tuple(logits.shape)}")
    if pos_weight is not None:
        if pos_weight.numel() != logits.shape[1]:
            raise _lib.HctError(f"bce_with_logits (HIP): pos_weight needs one entry per label ({logits.shape[1]}), not {pos_weight.numel()}")
        pos_weight = pos_weight.detach().to(device=logits.device, dtype=torch.float32).contiguous()
    return _BceWithLogitsFn.apply(logits.to(torch.float32).contiguous(), target.to(device=logits.device, dtype=torch.float32).contiguous(),
                                  pos_weight)


class LinearClassifier(FlatModule):
    """classifier.py:7-33: BatchNorm1d(dim, affine=False, eps=1e-6) -> Linear(dim, num_classes) on [B, dim] features.
    `feature_grad=True` (fine-tuning): in training mode the features may require a gradient and receive it."""

    def __init__(self, dim: int, num_classes: int, feature_grad: bool = False):
        super().__init__()
        self.bn = _BatchNormStats(dim)
        self.linear = _Affine(num_classes, dim, bias_shape=(num_classes,))
        self.feature_grad = bool(feature_grad)
        with torch.no_grad():
            init_linear_(self.linear)
        self._init_flat()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _require_eval_cuda(self, x, "LinearClassifier")
        ncls, dim = self.linear.weight.shape
        tokens = None
        if x.dim() == 3 and x.shape[2] == dim:  # the backbone's tokens: classify the class token
            tokens, x = x, x[:, 0, :]
        if x.dim() != 2 or x.shape[1] != dim:
            raise _lib.HctError(f"input shape {tuple(x.shape)} != (B, {dim}) or (B, T, {dim})")
        if self.training:
            if (tokens if tokens is not None else x).requires_grad and not self.feature_grad:
                raise _lib.HctError("LinearClassifier (HIP) trains on detached features (TRAIN.LOCK) unless built with "
                                    "feature_grad=True (fine-tuning the backbone through the head)")
            if tokens is not None:
                return _LinearHeadFn.apply(self.linear.weight, self, None, tokens)
            return _LinearHeadFn.apply(self.linear.weight, self, x, None)
        lib = _lib.load()
        with torch.no_grad(), torch.cuda.device(x.device):
            st = _lib.stream_ptr()
            x = x.to(torch.float32).contiguous()
            out = torch.empty(x.shape[0], ncls, dtype=torch.float32, device=x.device)
            _lib.check(lib.hct_head_linear(x.data_ptr(), dim, 1, self.bn.running_mean.data_ptr(), self.bn.running_var.data_ptr(), self.bn.eps,
                                           self.linear.weight.data_ptr(), self.linear.bias.data_ptr(), _lib.HCT_ACT_NONE, out.data_ptr(),
                                           x.shape[0], dim, ncls, st), "hct_head_linear")
        return out


class AttentionClassifier(FlatModule):
    """classifier.py:35-99: `num_queries` learnt query tokens attend over the (batch-normalised) token features through a
    key/value projection `wkv`; the attended vectors are batch-normalised, averaged over the queries and classified."""

    def __init__(self, dim: int, num_classes: int, num_heads: int = 12, qkv_bias: bool = False, qk_scale: Optional[float] = None,
                 num_queries: int = 1, compute_dtype: str = "fp32"):
        super().__init__()
        if dim % num_heads:
            raise ValueError("dim should be divisible by num_heads.")
        if compute_dtype not in ("bf16", "fp32"):
            raise ValueError("compute_dtype must be 'bf16' or 'fp32'")
        self.num_heads, self.num_queries, self.compute_dtype = num_heads, num_queries, compute_dtype
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.bn1 = _BatchNormStats(dim)
        self.bn2 = _BatchNormStats(dim)
        self.wkv = _Affine(dim * 2, dim, bias_shape=(dim * 2,) if qkv_bias else None)
        self.linear = _Affine(num_classes, dim, bias_shape=(num_classes,))
        self.cls_token = nn.Parameter(torch.zeros(1, num_queries, dim))
        with torch.no_grad():
            init_linear_(self.wkv)
            init_linear_(self.linear)
            nn.init.trunc_normal_(self.cls_token, std=0.02)
        self._init_flat()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _require_eval_cuda(self, x, "AttentionClassifier")
        ncls, dim = self.linear.weight.shape
        if x.dim() != 3 or x.shape[2] != dim:
            raise _lib.HctError(f"input shape {tuple(x.shape)} != (B, N, {dim})")
        if self.training:
            return _AttentionHeadFn.apply(self.linear.weight, self, _as_read(x).contiguous())
        return self._forward_eval(x)

    @torch.no_grad()
    def _forward_eval(self, x: torch.Tensor) -> torch.Tensor:
        ncls, dim = self.linear.weight.shape
        B, N, _ = x.shape
        H, Q, dh = self.num_heads, self.num_queries, dim // self.num_heads
        lib = _lib.load()
        dev = x.device
        tdt = torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32
        dt = _lib.dtype_code(tdt)
        with torch.cuda.device(dev):
            st = _lib.stream_ptr()
            x = x.to(torch.float32).contiguous()
            xn = torch.empty(B * N, dim, dtype=tdt, device=dev)  # bn1, classifier.py:89
            _lib.check(lib.hct_channel_norm(x.data_ptr(), self.bn1.running_mean.data_ptr(), self.bn1.running_var.data_ptr(), self.bn1.eps,
                                            xn.data_ptr(), dt, B * N, dim, st), "hct_channel_norm")
            w = _lib.cast_weight(self.wkv.weight.detach(), tdt, st)
            kv = torch.empty(B * N, 2 * dim, dtype=tdt, device=dev)  # wkv, classifier.py:90: [B, N, 2, H, dh] as it lies
            _lib.gemm(xn, w, kv, bias=self.wkv.bias, stream=st)
            att = torch.empty(B, H, Q, dh, dtype=torch.float32, device=dev)  # classifier.py:86, :93
            _lib.check(lib.hct_query_attention(self.cls_token.data_ptr(), Q, kv.data_ptr(), dt, B, N, H, dh, self.scale * dh ** -0.5,
                                               att.data_ptr(), st), "hct_query_attention")
            out = torch.empty(B, ncls, dtype=torch.float32, device=dev)  # reshape(B, Q, C) -> bn2 -> mean -> linear, :95-99
            _lib.check(lib.hct_head_linear(att.data_ptr(), Q * dim, Q, self.bn2.running_mean.data_ptr(), self.bn2.running_var.data_ptr(),
                                           self.bn2.eps, self.linear.weight.data_ptr(), self.linear.bias.data_ptr(), _lib.HCT_ACT_NONE,
                                           out.data_ptr(), B, dim, ncls, st), "hct_head_linear")
        return out


class _AttentionHeadFn(torch.autograd.Function):
    """Training-mode AttentionClassifier (classifier.py:73-99 with batch statistics).  Forward: bn1 statistics over the B*N token
    rows, the normalised tokens in the compute dtype, the wkv GEMM, the query attention (+ log-sum-exp), bn2 statistics over the
    B*Q rows, mean over the queries + linear.  Backward: linear.* ; bn2 backward with the linear dgrad fused in ; the attention
    backward (wkv output gradient, cls_token gradient) ; wkv.* and the normalised tokens' gradient over hct_gemm / hct_colsum ;
    bn1 backward into the tokens' gradient."""

    @staticmethod
    def forward(ctx, anchor, head, x):
        lib = _lib.load()
        B, N, D = x.shape
        H, Q = head.num_heads, head.num_queries
        dh = D // H
        ncls = head.linear.weight.shape[0]
        if B * Q < 2:
            raise _lib.HctError("AttentionClassifier in training mode: bn2 needs more than one row (B * num_queries > 1)")
        dev = x.device
        tdt = torch.bfloat16 if head.compute_dtype == "bf16" else torch.float32
        dt = _lib.dtype_code(tdt)
        ls = head.scale * dh ** -0.5
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            mean1, var1 = _bn_train_stats(lib, head.bn1, x, D, B * N, D)
            xn = torch.empty(B * N, D, dtype=tdt, device=dev)
            _lib.check(lib.hct_bn_norm(x.data_ptr(), _lib.dtype_code(x), D, B * N, D, mean1.data_ptr(), var1.data_ptr(), head.bn1.eps,
                                       xn.data_ptr(), dt, st), "hct_bn_norm")
            w = _lib.cast_weight(head.wkv.weight.detach(), tdt, st)
            kv = torch.empty(B * N, 2 * D, dtype=tdt, device=dev)
            _lib.gemm(xn, w, kv, bias=head.wkv.bias, workspace=True)
            att = torch.empty(B, H, Q, dh, dtype=torch.float32, device=dev)
            lse = torch.empty(B, H, Q, dtype=torch.float32, device=dev)
            _lib.check(lib.hct_query_attention_lse(head.cls_token.data_ptr(), Q, kv.data_ptr(), dt, B, N, H, dh, ls, att.data_ptr(),
                                                   lse.data_ptr(), st), "hct_query_attention_lse")
            mean2, var2 = _bn_train_stats(lib, head.bn2, att, D, B * Q, D)
            out = torch.empty(B, ncls, dtype=torch.float32, device=dev)
            _lib.check(lib.hct_head_linear_x(att.data_ptr(), _lib.HCT_F32, Q * D, Q, mean2.data_ptr(), var2.data_ptr(), head.bn2.eps,
                                             head.linear.weight.data_ptr(), head.linear.bias.data_ptr(), out.data_ptr(), B, D, ncls, st),
                       "hct_head_linear_x")
        ctx.head = head
        ctx.save_for_backward(x, xn, kv, att, lse, mean1, var1, mean2, var2)
        return out

    @staticmethod
    def backward(ctx, dlogits):
        head = ctx.head
        x, xn, kv, att, lse, mean1, var1, mean2, var2 = ctx.saved_tensors
        lib = _lib.load()
        B, N, D = x.shape
        H, Q = head.num_heads, head.num_queries
        dh = D // H
        W = head.linear.weight
        ncls = W.shape[0]
        dev = x.device
        tdt, dt = (kv.dtype, _lib.dtype_code(kv))
        ls = head.scale * dh ** -0.5
        dl = dlogits.to(torch.float32).contiguous()
        dx = None
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            buf, acc = _grad_buffer(head)
            gv = lambda name: head._grad_view(name, buf)
            _lib.check(lib.hct_head_linear_bwd(att.data_ptr(), _lib.HCT_F32, Q * D, Q, mean2.data_ptr(), var2.data_ptr(), head.bn2.eps,
                                               dl.data_ptr(), B, D, ncls, gv("linear.weight").data_ptr(), gv("linear.bias").data_ptr(), st),
                       "hct_head_linear_bwd")
            rows_max = max(B * Q, B * N)
            ws = torch.empty(lib.hct_bn_rows_workspace_bytes(rows_max, D) + 8 * D, dtype=torch.uint8, device=dev)
            datt = torch.empty(B, H, Q, dh, dtype=torch.float32, device=dev)  # [B, Q, D] as classifier.py:95 reshapes it
            _lib.check(lib.hct_bn_bwd_input(att.data_ptr(), _lib.HCT_F32, D, mean2.data_ptr(), var2.data_ptr(), head.bn2.eps, None, 0,
                                            dl.data_ptr(), W.data_ptr(), Q, ncls, B * Q, D, datt.data_ptr(), _lib.HCT_F32, D, ws.data_ptr(),
                                            ws.numel(), st),
                       "hct_bn_bwd_input")
            dkv = torch.empty(B * N, 2 * D, dtype=tdt, device=dev)
            wsq = torch.empty(max(16, lib.hct_query_attention_bwd_workspace_bytes(B, Q, H, dh)), dtype=torch.uint8, device=dev)
            _lib.check(lib.hct_query_attention_bwd(head.cls_token.data_ptr(), Q, kv.data_ptr(), dt, B, N, H, dh, ls, att.data_ptr(),
                                                   lse.data_ptr(), datt.data_ptr(), dkv.data_ptr(), gv("cls_token").data_ptr(), wsq.data_ptr(),
                                                   wsq.numel(), st), "hct_query_attention_bwd")
            _lib.gemm(dkv, xn, gv("wkv.weight"), trans_a=True, trans_b=False, workspace=True)  # dWkv = dkv^T . xn
            if head.wkv.bias is not None:
                wsc = torch.empty(max(16, lib.hct_colsum_workspace_bytes(B * N, 2 * D)), dtype=torch.uint8, device=dev)
                _lib.check(lib.hct_colsum(dkv.data_ptr(), dt, B * N, 2 * D, 2 * D, gv("wkv.bias").data_ptr(), wsc.data_ptr(), wsc.numel(), st),
                           "hct_colsum")
            if ctx.needs_input_grad[2]:
                wt = torch.empty(D, 2 * D, dtype=tdt, device=dev)  # Wkv^T: the dgrad is an NT product like the forward
                _lib.check(lib.hct_transpose_cast(head.wkv.weight.data_ptr(), _lib.HCT_F32, wt.data_ptr(), dt, 2 * D, D, st), "hct_transpose_cast")
                dxn = torch.empty(B * N, D, dtype=torch.float32, device=dev)
                _lib.gemm(dkv, wt, dxn, workspace=True)
                dx = torch.empty(B, N, D, dtype=x.dtype, device=dev)
                _lib.check(lib.hct_bn_bwd_input(x.data_ptr(), _lib.dtype_code(x), D, mean1.data_ptr(), var1.data_ptr(), head.bn1.eps,
                                                dxn.data_ptr(), D, None, None, 1, 0, B * N, D, dx.data_ptr(), _lib.dtype_code(dx), D,
                                                ws.data_ptr(), ws.numel(), st), "hct_bn_bwd_input")
            _finish_grads(head, lib, buf, acc)
        return None, None, dx
