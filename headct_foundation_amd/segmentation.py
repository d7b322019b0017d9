"""Segmentation fine-tuning on the HIP kernels (an addition of this build): a linear voxel decoder over the backbone's patch
tokens and a Dice + cross-entropy loss over the voxels, read from the logits in token layout.

`SegmentationHead(dim, patch_size, num_classes)` is Segmenter's "linear decoder": one Linear `dim -> K * P^3` per token.  Row
`c * P^3 + v` of `linear.weight` is class c at voxel v = (pz * P + py) * P + px of the patch (the order of the patch embedding's
kernel axes); patch l = (lz * G + ly) * G + lx covers z = lz * P + pz, likewise y and x.  It takes the backbone's tokens
`[B, T, dim]` in their own dtype (fp32 or bf16) and gives logits `[B, T, K * P^3]` in that dtype.  The Linear runs over all B * T
rows -- the 1 + R leading rows (class token, registers) cost (1 + R) / T of the product and save a gather copy; the loss and the
prediction skip them (`first`).  The logits are never un-patchified.  Forward, dgrad and wgrad go through `_lib.gemm`, the bias
gradient through `hct_colsum`; parameters and gradients live in flat fp32 buffers (`flat.FlatModule`), so the fused optimizers,
the clips, layer decay and DDP drive the head as they drive the classification heads.

`seg_loss` wraps `hct_seg_loss` (stats + finalize in the forward, the gradient phase alone in the backward, out of the workspace
the forward left), `seg_predict` wraps `hct_seg_predict`, `gather_flip_labels` wraps `hct_gather_flip_labels`,
`affine_labels` wraps `hct_affine_labels` (the labels' half of a random affine, SEG.AFFINE_PROB).  No CPU path; no arithmetic of the
path runs in torch ops.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .classifier import _as_read, _finish_grads, _grad_buffer
from .flat import FlatModule
from .layers import _Affine, init_linear_

IGNORE_INDEX = 255
MAX_CLASSES = 16


def _rows(logits: torch.Tensor, what: str):
    """(B, T, ld) of token-layout logits [B, T, N]: unit stride along the columns, one row stride over the batch and the tokens."""
    if not logits.is_cuda or logits.dim() != 3 or logits.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.HctError(f"{what} (HIP): logits [B, T, K * P^3] in fp32 or bf16 on 'cuda' expected (no CPU fallback exists)")
    B, T, _ = logits.shape
    ld = logits.stride(1)
    if logits.stride(2) != 1 or (B > 1 and logits.stride(0) != T * ld):
        raise _lib.HctError(f"{what} (HIP): the logits need unit column stride and one row stride over batch and tokens")
    return B, T, ld


def _geometry(logits: torch.Tensor, patch_size: int, num_classes: int, first: int, what: str):
    B, T, ld = _rows(logits, what)
    P, K = int(patch_size), int(num_classes)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"{what}: num_classes must lie in [2, {MAX_CLASSES}], got {K}")
    if logits.shape[2] != K * P ** 3:
        raise _lib.HctError(f"{what} (HIP): {logits.shape[2]} columns, K * P^3 = {K * P ** 3} expected")
    L = T - int(first)
    G = round(L ** (1.0 / 3.0)) if L > 0 else 0
    if first < 0 or G < 1 or G ** 3 != L:
        raise _lib.HctError(f"{what} (HIP): T - first = {L} tokens are no cubic patch grid")
    return B, T, ld, G, P, K


def _check_labels(labels: torch.Tensor, B: int, S: int, device, what: str) -> torch.Tensor:
    if labels.dtype != torch.uint8 or tuple(labels.shape) != (B, S, S, S):
        raise _lib.HctError(f"{what} (HIP): labels uint8 [{B}, {S}, {S}, {S}] expected, got {labels.dtype} {tuple(labels.shape)}")
    return labels.to(device).contiguous()


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, class_weight, geom, w_ce, w_dice, inplace_grad, parts):
        lib = _lib.load()
        B, T, ld, G, P, K, first = geom
        dev = logits.device
        with torch.cuda.device(dev):
            ws = torch.empty(max(16, lib.hct_seg_loss_workspace_bytes(B, G, P, K)), dtype=torch.uint8, device=dev)
            out = torch.empty(3 + B * K, dtype=torch.float32, device=dev)  # loss, ce, dice, dice_bc
            _lib.check(lib.hct_seg_loss(logits.data_ptr(), _lib.dtype_code(logits), ld, labels.data_ptr(), _lib.ptr(class_weight), B, T, first,
                                        G, P, K, w_ce, w_dice, None, out.data_ptr(), out[1:].data_ptr(), out[2:].data_ptr(),
                                        out[3:].data_ptr(), None, 0, 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "hct_seg_loss")
        if parts is not None:
            parts.update(ce=out[1], dice=out[2], dice_bc=out[3:].view(B, K))
        ctx.geom, ctx.weights, ctx.inplace, ctx.class_weight = geom, (w_ce, w_dice), inplace_grad, class_weight
        ctx.save_for_backward(logits, labels, ws)
        return out[0].clone()

    @staticmethod
    def backward(ctx, dloss):
        logits, labels, ws = ctx.saved_tensors
        lib = _lib.load()
        B, T, ld, G, P, K, first = ctx.geom
        dev = logits.device
        dloss = dloss.to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            if ctx.inplace:  # the thread that reads a voxel's logits writes its gradients: the logits buffer becomes the gradient
                dlogits, ldd = logits, ld
            else:
                dlogits = torch.empty(logits.shape, dtype=logits.dtype, device=dev)
                ldd = dlogits.stride(1)
            _lib.check(lib.hct_seg_loss(logits.data_ptr(), _lib.dtype_code(logits), ld, labels.data_ptr(), _lib.ptr(ctx.class_weight), B, T,
                                        first, G, P, K, ctx.weights[0], ctx.weights[1], dloss.data_ptr(), None, None, None, None,
                                        dlogits.data_ptr(), ldd, 1, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "hct_seg_loss")
        return dlogits, None, None, None, None, None, None, None


def seg_loss(logits: torch.Tensor, labels: torch.Tensor, patch_size: int, num_classes: int, first: int = 0, ce_weight: float = 1.0,
             dice_weight: float = 1.0, class_weight: Optional[torch.Tensor] = None, inplace_grad: bool = False,
             parts: Optional[dict] = None) -> torch.Tensor:
    """ce_weight * CE + dice_weight * Dice over the voxels of `labels` (uint8 [B, S, S, S], 0 .. K-1, 255 = ignore) of token-layout
    `logits` [B, T, K * P^3] whose first `first` rows per sample are no patches.  CE is the class-weighted mean over the valid
    voxels (torch's `cross_entropy(weight=, ignore_index=255)`), Dice MONAI's `DiceLoss(softmax=True, include_background=True,
    batch=False)` over the valid voxels; a batch with no valid voxel has loss 0 and a zero gradient.  `parts` (a dict) receives
    `ce`, `dice`, `dice_bc [B, K]`.  The gradient is zero in the leading rows and at ignored voxels.  `inplace_grad=True` writes it
    over the logits themselves (the caller no longer needs them, and runs one backward): the decoder's logits are the largest
    tensor of the step."""
    first = int(first)
    B, T, ld, G, P, K = _geometry(logits, patch_size, num_classes, first, "seg_loss")
    labels = _check_labels(labels, B, G * P, logits.device, "seg_loss")
    if class_weight is not None:
        class_weight = torch.as_tensor(class_weight).detach().to(device=logits.device, dtype=torch.float32).contiguous()
        if class_weight.numel() != K:
            raise _lib.HctError(f"seg_loss (HIP): class_weight needs one entry per class ({K}), not {class_weight.numel()}")
    return _SegLossFn.apply(logits, labels, class_weight, (B, T, ld, G, P, K, first), float(ce_weight), float(dice_weight), bool(inplace_grad),
                            parts)


@torch.no_grad()
def seg_predict(logits: torch.Tensor, patch_size: int, num_classes: int, first: int = 0, labels: Optional[torch.Tensor] = None,
                prob_class: Optional[int] = None, want_pred: bool = True) -> dict:
    """One pass over token-layout logits: `pred` uint8 [B, S, S, S] (arg-max class, ties to the lowest), `prob` fp16 [B, S, S, S]
    (softmax probability of `prob_class`, when given), `counts` int64 [B, K, 3] = TP, FP, FN over the valid voxels (when `labels`
    are given)."""
    first = int(first)
    B, T, ld, G, P, K = _geometry(logits, patch_size, num_classes, first, "seg_predict")
    S, dev = G * P, logits.device
    lib = _lib.load()
    out = {}
    with torch.cuda.device(dev):
        pred = torch.empty(B, S, S, S, dtype=torch.uint8, device=dev) if want_pred else None
        prob = torch.empty(B, S, S, S, dtype=torch.float16, device=dev) if prob_class is not None else None
        counts = ws = None
        if labels is not None:
            labels = _check_labels(labels, B, S, dev, "seg_predict")
            counts = torch.empty(B, K, 3, dtype=torch.int64, device=dev)
            ws = torch.empty(max(16, lib.hct_seg_predict_workspace_bytes(B, G, P, K)), dtype=torch.uint8, device=dev)
        _lib.check(lib.hct_seg_predict(logits.data_ptr(), _lib.dtype_code(logits), ld, _lib.ptr(labels), B, T, first, G, P, K,
                                       int(prob_class) if prob_class is not None else 0, _lib.ptr(pred), _lib.ptr(prob), _lib.ptr(counts),
                                       _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr(dev)), "hct_seg_predict")
    if pred is not None:
        out["pred"] = pred
    if prob is not None:
        out["prob"] = prob
    if counts is not None:
        out["counts"] = counts
    return out


@torch.no_grad()
def gather_flip_labels(pool: torch.Tensor, slots: torch.Tensor, flip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] = flips(pool[slots[b]]) for label volumes: pool uint8 [n, S, S, S], slots int32 [B] (-1: an all-ignore volume), flip
    uint8 [B] the 3-bit code `DeviceAugment.draw` gives the volume launch (bit a = spatial axis a)."""
    if not pool.is_cuda or pool.dtype != torch.uint8 or pool.dim() != 4:
        raise _lib.HctError("gather_flip_labels (HIP): pool uint8 [n, S, S, S] on 'cuda' expected (no CPU fallback exists)")
    dev = pool.device
    pool = pool.contiguous()
    n, S = pool.shape[0], pool.shape[1]
    slots = slots.to(device=dev, dtype=torch.int32).contiguous()
    B = slots.numel()
    if flip is not None:
        flip = flip.to(device=dev, dtype=torch.uint8).contiguous()
        if flip.numel() != B:
            raise _lib.HctError(f"gather_flip_labels (HIP): flip needs one code per sample ({B}), not {flip.numel()}")
    out = torch.empty(B, S, S, S, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().hct_gather_flip_labels(pool.data_ptr(), slots.data_ptr(), out.data_ptr(), B, S, n, _lib.ptr(flip),
                                                      _lib.stream_ptr(dev)), "hct_gather_flip_labels")
    return out


@torch.no_grad()
def affine_labels(pool: torch.Tensor, slots: torch.Tensor, mat: Optional[torch.Tensor], fire: Optional[torch.Tensor] = None,
                  flip: Optional[torch.Tensor] = None, outside: int = 0) -> torch.Tensor:
    """Label volumes through the table the scans take in `data.affine_augment` (hct_affine_labels): out[b] is pool[slots[b]] read at
    the nearest voxel of mat[b]'s coordinates where fire[b] (None: everywhere; a tie at half a voxel goes to the higher index, a
    coordinate outside [-0.5, S - 0.5) on any axis gives the byte `outside`), and flips(pool[slots[b]]) with flip[b]'s bits where
    not.  pool uint8 [n, S, S, S], slots int32 [B] (-1: an all-ignore volume), mat [B, 12] fp32 with the flips folded in
    (`data.affine_matrices`) or None for the plain `gather_flip_labels`.  A matrix given on the CPU with a non-finite entry raises."""
    from .data import _checked_mat
    if not pool.is_cuda or pool.dtype != torch.uint8 or pool.dim() != 4:
        raise _lib.HctError("affine_labels (HIP): pool uint8 [n, S, S, S] on 'cuda' expected (no CPU fallback exists)")
    if isinstance(outside, bool) or int(outside) != outside or not 0 <= int(outside) <= 255:
        raise ValueError(f"affine_labels: outside must be a byte 0 .. 255, got {outside!r}")
    dev = pool.device
    pool = pool.contiguous()
    n, S = pool.shape[0], pool.shape[1]
    slots = slots.to(device=dev, dtype=torch.int32).contiguous()
    B = slots.numel()
    mat, fire = _checked_mat(mat, fire, B)
    on = lambda t, dt: None if t is None else t.to(device=dev, dtype=dt).contiguous()
    mat, fire, flip = on(mat, torch.float32), on(fire, torch.uint8), on(flip, torch.uint8)
    if flip is not None and flip.numel() != B:
        raise _lib.HctError(f"affine_labels (HIP): flip needs one code per sample ({B}), not {flip.numel()}")
    out = torch.empty(B, S, S, S, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().hct_affine_labels(pool.data_ptr(), slots.data_ptr(), n, out.data_ptr(), B, S, _lib.ptr(mat), _lib.ptr(fire),
                                                 _lib.ptr(flip), int(outside), _lib.stream_ptr(dev)), "hct_affine_labels")
    return out


class _SegHeadFn(torch.autograd.Function):
    """Training-mode SegmentationHead.  Forward: logits = tokens . W^T + b over all B * T rows (NT product).  Backward: dW = dL^T .
    tokens (TN product) and db = column sums of dL into the head's flat gradient buffer; when the tokens require one, their
    gradient dL . W as an NT product against W^T."""

    @staticmethod
    def forward(ctx, anchor, head, x):
        B, T, D = x.shape
        W = head.linear.weight
        N = W.shape[0]
        dev = x.device
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            w = _lib.cast_weight(W.detach(), x.dtype, st)
            out = torch.empty(B * T, N, dtype=x.dtype, device=dev)
            _lib.gemm(x.view(B * T, D), w, out, bias=head.linear.bias, workspace=True, stream=st)
        ctx.head = head
        ctx.save_for_backward(x)
        return out.view(B, T, N)

    @staticmethod
    def backward(ctx, dlogits):
        head = ctx.head
        (x,) = ctx.saved_tensors
        lib = _lib.load()
        B, T, D = x.shape
        W = head.linear.weight
        N = W.shape[0]
        dev = x.device
        dl = dlogits if dlogits.dtype == x.dtype else dlogits.to(x.dtype)
        dl = dl.contiguous().view(B * T, N)
        dt = _lib.dtype_code(x)
        dx = None
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            buf, acc = _grad_buffer(head)
            gv = lambda name: head._grad_view(name, buf)
            _lib.gemm(dl, x.view(B * T, D), gv("linear.weight"), trans_a=True, trans_b=False, workspace=True, stream=st)
            wsc = torch.empty(max(16, lib.hct_colsum_workspace_bytes(B * T, N)), dtype=torch.uint8, device=dev)
            _lib.check(lib.hct_colsum(dl.data_ptr(), dt, B * T, N, N, gv("linear.bias").data_ptr(), wsc.data_ptr(), wsc.numel(), st), "hct_colsum")
            if ctx.needs_input_grad[2]:
                wt = torch.empty(D, N, dtype=x.dtype, device=dev)  # W^T: the dgrad is an NT product like the forward
                _lib.check(lib.hct_transpose_cast(W.data_ptr(), _lib.HCT_F32, wt.data_ptr(), dt, N, D, st), "hct_transpose_cast")
                dx = torch.empty(B, T, D, dtype=x.dtype, device=dev)
                _lib.gemm(dl, wt, dx.view(B * T, D), workspace=True, stream=st)
            _finish_grads(head, lib, buf, acc)
        return None, None, dx


class SegmentationHead(FlatModule):
    """Linear voxel decoder: Linear(dim, num_classes * patch_size^3) on every token of [B, T, dim]; logits stay in token layout."""

    def __init__(self, dim: int, patch_size: int, num_classes: int):
        super().__init__()
        if not 2 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"num_classes must lie in [2, {MAX_CLASSES}], got {num_classes}")
        if int(patch_size) < 1 or int(dim) < 1:
            raise ValueError("dim and patch_size must be positive")
        self.dim, self.patch_size, self.num_classes = int(dim), int(patch_size), int(num_classes)
        n = self.num_classes * self.patch_size ** 3
        self.linear = _Affine(n, self.dim, bias_shape=(n,))
        with torch.no_grad():
            init_linear_(self.linear)
        self._init_flat()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda or not self.linear.weight.is_cuda:
            raise _lib.HctError("SegmentationHead (HIP) runs on the GPU in train and eval mode: move the module and the input to 'cuda' "
                                "(no CPU fallback exists)")
        if x.dim() != 3 or x.shape[2] != self.dim:
            raise _lib.HctError(f"input shape {tuple(x.shape)} != (B, T, {self.dim})")
        x = _as_read(x).contiguous()
        if torch.is_grad_enabled() and (self.training or x.requires_grad):
            return _SegHeadFn.apply(self.linear.weight, self, x)
        B, T, D = x.shape
        N = self.linear.weight.shape[0]
        with torch.no_grad(), torch.cuda.device(x.device):
            st = _lib.stream_ptr(x.device)
            w = _lib.cast_weight(self.linear.weight.detach(), x.dtype, st)
            out = torch.empty(B * T, N, dtype=x.dtype, device=x.device)
            _lib.gemm(x.view(B * T, D), w, out, bias=self.linear.bias, workspace=True, stream=st)
        return out.view(B, T, N)
