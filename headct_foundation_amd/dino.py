"""DINO self-distillation pieces on the HIP path (BASELINE config #5; reference engine_pretrain_dino.py:14-130).

Built: `DINOLoss` (src/losses/losses.py:46-102: same constructor, `forward(student_output, teacher_output, epoch)`, `center`
buffer and `update_center`, fused loss + gradient kernel over the K prototypes), `update_momentum_encoder`
(src/utils/misc.py:386-397) on the models' flat fp32 parameter buffers, and the cosine weight-decay / momentum schedules
(src/utils/wd_sched.py:3-23).  No CPU fallback: tensors must live on the GPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib
from ._lib import HctError


def wd_cosine_scheduler(base_value, final_value, epochs, niter_per_ep, warmup_epochs=0, start_warmup_value=0):
    """Per-iteration schedule: optional linear warm-up, then half a cosine from base_value to final_value."""
    n_warm = warmup_epochs * niter_per_ep
    warm = np.linspace(start_warmup_value, base_value, n_warm) if warmup_epochs > 0 else np.array([])
    t = np.arange(epochs * niter_per_ep - n_warm)
    body = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * t / len(t)))
    out = np.concatenate((warm, body))
    if len(out) != epochs * niter_per_ep:
        raise AssertionError("schedule length does not match epochs * iterations per epoch")
    return out


def get_wd_scheduler(config, niter_per_ep, warmup_epochs=0, start_warmup_value=0):
    return wd_cosine_scheduler(config.TRAIN.WEIGHT_DECAY, config.TRAIN.WEIGHT_DECAY_END, config.TRAIN.MAX_EPOCHS, niter_per_ep,
                               warmup_epochs, start_warmup_value)


class _DinoLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, center, ncrops, student_temp, teacher_temp, center_sum):
        lib = _lib.load()
        if not (student.is_cuda and teacher.is_cuda):
            raise HctError("DINOLoss (HIP) needs GPU tensors; there is no CPU fallback")
        if student.dtype not in (torch.float32, torch.bfloat16) or teacher.dtype != student.dtype:
            raise HctError("DINOLoss (HIP): student / teacher logits must both be fp32 or both bf16")
        student, teacher = student.contiguous(), teacher.contiguous()
        K = student.shape[1]
        B = teacher.shape[0] // 2
        if student.shape[0] != ncrops * B or teacher.shape[0] != 2 * B or teacher.shape[1] != K:
            raise HctError(f"DINOLoss: shapes student {tuple(student.shape)} / teacher {tuple(teacher.shape)} do not match {ncrops} crops")
        ws = torch.empty(lib.hct_dino_loss_workspace_bytes(ncrops, B, K), dtype=torch.uint8, device=student.device)
        loss = torch.empty(1, dtype=torch.float32, device=student.device)
        dstudent = torch.empty_like(student) if ctx.needs_input_grad[0] else None
        _lib.check(lib.hct_dino_loss(student.data_ptr(), teacher.data_ptr(), _lib.dtype_code(student), ncrops, B, K, center.data_ptr(),
                                     float(student_temp), float(teacher_temp), loss.data_ptr(), _lib.ptr(dstudent), None,
                                     _lib.ptr(center_sum), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "hct_dino_loss")
        ctx.dstudent = dstudent
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        if ctx.dstudent is None:
            raise HctError("DINOLoss: the forward ran without gradient storage")
        return ctx.dstudent * g.to(ctx.dstudent.dtype), None, None, None, None, None, None


CENTERING_MODES = ("centering", "sinkhorn_knopp")


def combine_lse(local_lse, group=None):
    """Log-sum-exp over the ranks of a per-rank log-sum-exp vector: all-reduce MAX, all-reduce SUM of exp(lse - max), log.  A list or
    tuple of vectors stands for the ranks themselves (no collective: what the ranks would agree on).  The identity without a process
    group.  Plain torch on a [K] vector, CPU tensors included."""
    if isinstance(local_lse, (list, tuple)):
        stack = torch.stack(list(local_lse))
        m = stack.max(dim=0).values
        return m + torch.log(torch.exp(stack - m).sum(dim=0))
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local_lse
    m = local_lse.clone()
    dist.all_reduce(m, op=dist.ReduceOp.MAX, group=group)
    s = torch.exp(local_lse - m)
    dist.all_reduce(s, op=dist.ReduceOp.SUM, group=group)
    return m + torch.log(s)


def _check_teacher(t):
    if not t.is_cuda:
        raise HctError("Sinkhorn-Knopp (HIP) needs GPU tensors; there is no CPU fallback")
    if t.dtype not in (torch.float32, torch.bfloat16) or t.dim() != 2 or t.shape[1] % 4:
        raise HctError(f"Sinkhorn-Knopp (HIP): teacher logits [R, K] must be fp32 or bf16 with K % 4 == 0, got {tuple(t.shape)} {t.dtype}")


def sk_col_lse(teacher, inv_temp: float, lr=None):
    """[K] fp32: logsumexp over this rank's rows of teacher[b, k] * inv_temp + lr[b] (hct_dino_sk_col_lse; lr None = zeros)."""
    _check_teacher(teacher)
    lib = _lib.load()
    teacher = teacher.contiguous()
    R, K = teacher.shape
    out = torch.empty(K, dtype=torch.float32, device=teacher.device)
    ws = torch.empty(max(16, lib.hct_dino_sk_workspace_bytes(R, K)), dtype=torch.uint8, device=teacher.device)
    _lib.check(lib.hct_dino_sk_col_lse(teacher.data_ptr(), _lib.dtype_code(teacher), R, K, float(inv_temp), _lib.ptr(lr), out.data_ptr(),
                                       ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "hct_dino_sk_col_lse")
    return out


def sk_row_lse(teacher, inv_temp: float, lc):
    """[R] fp32: logsumexp over k of teacher[b, k] * inv_temp + lc[k] (hct_dino_sk_row_lse)."""
    _check_teacher(teacher)
    teacher = teacher.contiguous()
    R, K = teacher.shape
    out = torch.empty(R, dtype=torch.float32, device=teacher.device)
    _lib.check(_lib.load().hct_dino_sk_row_lse(teacher.data_ptr(), _lib.dtype_code(teacher), R, K, float(inv_temp), lc.data_ptr(), out.data_ptr(),
                                               _lib.stream_ptr()), "hct_dino_sk_row_lse")
    return out


@torch.no_grad()
def sinkhorn_knopp_logs(teacher, teacher_temp: float, n_iters: int = 3, world: int = 1, n_total=None):
    """(lc [K], lr [R], log N) of the Sinkhorn-Knopp teacher q = exp(t / T + lr + lc + log N) (csrc/dino.hip): `n_iters` rounds of the
    column pass, `combine_lse` over the ranks, the row pass.  N = R * world rows, or `n_total` where the ranks hold unequal row counts
    (the masked patch rows of the iBOT loss)."""
    if n_iters < 1:
        raise ValueError(f"Sinkhorn-Knopp needs at least one iteration, got {n_iters}")
    R, K = teacher.shape
    inv_t = float(np.float32(1.0) / np.float32(teacher_temp))  # what hct_dino_loss_sk forms from teacher_temp
    log_n, log_k = math.log(R * world if n_total is None else int(n_total)), math.log(K)
    lr = None
    for _ in range(n_iters):
        lc = (-log_k) - combine_lse(sk_col_lse(teacher, inv_t, lr))
        lr = (-log_n) - sk_row_lse(teacher, inv_t, lc)
    return lc, lr, log_n


class _DinoLossSkFn(torch.autograd.Function):
    """_DinoLossFn with the teacher distribution given by the Sinkhorn-Knopp (lc, lr, log N): hct_dino_loss_sk, no centre sums."""

    @staticmethod
    def forward(ctx, student, teacher, lc, lr, log_n, ncrops, student_temp, teacher_temp):
        lib = _lib.load()
        if not (student.is_cuda and teacher.is_cuda):
            raise HctError("DINOLoss (HIP) needs GPU tensors; there is no CPU fallback")
        if student.dtype not in (torch.float32, torch.bfloat16) or teacher.dtype != student.dtype:
            raise HctError("DINOLoss (HIP): student / teacher logits must both be fp32 or both bf16")
        student, teacher = student.contiguous(), teacher.contiguous()
        K = student.shape[1]
        B = teacher.shape[0] // 2
        if student.shape[0] != ncrops * B or teacher.shape[0] != 2 * B or teacher.shape[1] != K:
            raise HctError(f"DINOLoss: shapes student {tuple(student.shape)} / teacher {tuple(teacher.shape)} do not match {ncrops} crops")
        ws = torch.empty(lib.hct_dino_loss_sk_workspace_bytes(ncrops, B, K), dtype=torch.uint8, device=student.device)
        loss = torch.empty(1, dtype=torch.float32, device=student.device)
        dstudent = torch.empty_like(student) if ctx.needs_input_grad[0] else None
        _lib.check(lib.hct_dino_loss_sk(student.data_ptr(), teacher.data_ptr(), _lib.dtype_code(student), ncrops, B, K, lc.data_ptr(), lr.data_ptr(),
                                        float(log_n), float(student_temp), float(teacher_temp), loss.data_ptr(), _lib.ptr(dstudent), None,
                                        ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "hct_dino_loss_sk")
        ctx.dstudent = dstudent
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        if ctx.dstudent is None:
            raise HctError("DINOLoss: the forward ran without gradient storage")
        return ctx.dstudent * g.to(ctx.dstudent.dtype), None, None, None, None, None, None, None


class DINOLoss(nn.Module):
    """Same interface as the reference's DINOLoss (losses.py:46-102).  `centering` (an addition of this build): 'centering' is the
    reference's EMA centre; 'sinkhorn_knopp' makes the teacher distribution by `sk_iters` Sinkhorn-Knopp iterations over the batch of
    all ranks (DINOv2; csrc/dino.hip) and leaves `center` alone -- the buffer stays for the checkpoint layout.  Pairing of the crops and
    the 1 / (2 (V - 1)) normalisation are the same in both modes."""

    def __init__(self, out_dim, ncrops, warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs, nepochs, student_temp=0.1,
                 center_momentum=0.9, centering="centering", sk_iters=3):
        super().__init__()
        if centering not in CENTERING_MODES:
            raise ValueError(f"DINOLoss: centering must be one of {CENTERING_MODES}, got {centering!r}")
        if centering == "sinkhorn_knopp" and int(sk_iters) < 1:
            raise ValueError(f"DINOLoss: sk_iters must be at least 1, got {sk_iters}")
        self.centering, self.sk_iters = centering, int(sk_iters)
        self.student_temp, self.center_momentum, self.ncrops = student_temp, center_momentum, ncrops
        self.register_buffer("center", torch.zeros(1, out_dim))
        self.teacher_temp_schedule = np.concatenate((np.linspace(warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs),
                                                     np.ones(nepochs - warmup_teacher_temp_epochs) * teacher_temp))

    def forward(self, student_output, teacher_output, epoch):
        temp = float(self.teacher_temp_schedule[epoch])
        if self.centering == "sinkhorn_knopp":
            teacher = teacher_output.detach().contiguous()
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
            lc, lr, log_n = sinkhorn_knopp_logs(teacher, temp, self.sk_iters, world=world)
            return _DinoLossSkFn.apply(student_output, teacher, lc, lr, log_n, self.ncrops, self.student_temp, temp)
        csum = torch.empty(self.center.shape[1], dtype=torch.float32, device=self.center.device)
        # grad mode is read by the Function's caller side: inside Function.forward it is always off
        loss = _DinoLossFn.apply(student_output, teacher_output.detach(), self.center, self.ncrops, self.student_temp, temp, csum)
        self._apply_center(csum, teacher_output.shape[0])
        return loss

    @torch.no_grad()
    def _apply_center(self, csum, n_rows):
        world = 1
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(csum)
            world = dist.get_world_size()
        _lib.check(_lib.load().hct_dino_center_update(self.center.data_ptr(), csum.data_ptr(), csum.numel(), float(self.center_momentum),
                                                      float(n_rows * world), _lib.stream_ptr()), "hct_dino_center_update")

    @torch.no_grad()
    def update_center(self, teacher_output):
        """losses.py:93-102 as a stand-alone call (forward() already does it from the loss kernel's column sums)."""
        csum = teacher_output.float().sum(dim=0).contiguous()
        self._apply_center(csum, teacher_output.shape[0])


class _KoLeoFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        n, D = x.shape
        dev = x.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nn_index = torch.empty(n, dtype=torch.int32, device=dev)
        d, inv = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(lib.hct_koleo_fwd(x.data_ptr(), _lib.dtype_code(x), n, D, x.stride(0), loss.data_ptr(), nn_index.data_ptr(), d.data_ptr(),
                                     inv.data_ptr(), _lib.stream_ptr()), "hct_koleo_fwd")
        ctx.saved = (x, nn_index, d, inv)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        x, nn_index, d, inv = ctx.saved
        n, D = x.shape
        dx = torch.empty(n, D, dtype=x.dtype, device=x.device)
        gl = g.detach().float().reshape(1).contiguous()
        _lib.check(_lib.load().hct_koleo_bwd(x.data_ptr(), _lib.dtype_code(x), n, D, x.stride(0), nn_index.data_ptr(), d.data_ptr(), inv.data_ptr(),
                                             gl.data_ptr(), dx.data_ptr(), D, _lib.stream_ptr()), "hct_koleo_bwd")
        return dx


def koleo_loss(x: torch.Tensor) -> torch.Tensor:
    """KoLeo regulariser of DINOv2 on feature rows x [n, D] (fp32 or bf16; n >= 2, D % 4 == 0): -mean_i log(||xh_i - xh_nn(i) + 1e-8|| + 1e-8)
    over the L2-normalised rows, nn(i) the row of largest cosine to row i (a constant in the backward).  Rows may be a strided view
    with contiguous columns -- the class tokens `tokens[:, 0, :]` of a token tensor are read where they lie (csrc/koleo.hip)."""
    if not x.is_cuda:
        raise HctError("koleo_loss (HIP) needs a GPU tensor; there is no CPU fallback")
    if x.dim() != 2 or x.shape[0] < 2 or x.shape[1] % 4 or x.shape[1] > 4096:
        raise HctError(f"koleo_loss: needs [n, D] with n >= 2 rows, D % 4 == 0 and D <= 4096, got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise HctError(f"koleo_loss: rows must be fp32 or bf16, got {x.dtype}")
    if x.stride(1) != 1 or x.stride(0) % 4 or x.stride(0) < x.shape[1] or x.data_ptr() % (4 * x.element_size()):
        x = x.contiguous()
    return _KoLeoFn.apply(x)


@torch.no_grad()
def update_momentum_encoder(model, momentum_model, m: float) -> None:
    """misc.py:386-397 for flat-buffer HIP models: one fused launch over the whole parameter buffer (k = k*m + (1-m)*q)."""
    q, k = getattr(model, "_flat", None), getattr(momentum_model, "_flat", None)
    if q is None or k is None or q.numel() != k.numel() or not q.is_cuda:
        raise HctError("update_momentum_encoder (HIP) needs two flat-buffer HIP models of the same architecture on the GPU")
    _lib.check(_lib.load().hct_ema_update(k.data_ptr(), q.data_ptr(), k.numel(), float(m), _lib.stream_ptr()), "hct_ema_update")
    if hasattr(momentum_model, "mark_weights_updated"):
        momentum_model.mark_weights_updated()


@torch.no_grad()
def ema_update_(k: torch.Tensor, q: torch.Tensor, m: float) -> None:
    """The same update on two arbitrary contiguous fp32 GPU tensors (numel % 4 == 0)."""
    _lib.check(_lib.load().hct_ema_update(k.data_ptr(), q.data_ptr(), k.numel(), float(m), _lib.stream_ptr()), "hct_ema_update")


class DinoOptimizer:
    """One optimizer over the student's two flat parameter buffers (backbone plan + projection head): two fused launches of the
    same kind (`kind` = TRAIN.OPTIMIZER: 'AdamW' | 'Lion' | 'Lamb' | 'SGD') that share the hyper-parameters of `param_groups[0]`
    (what the LR scheduler and the weight-decay schedule write to; SGD ignores the weight decay, as the reference's does).
    The reference builds one optimizer over MultiCropWrapper.parameters() (main_pretrain_dino.py:219); the arithmetic per
    parameter is the same, and `state_dict()` has the reference's flat layout (one state dict over backbone + head parameters)."""

    def __init__(self, model, lr, betas=(0.9, 0.999), weight_decay=0.0, eps=None, kind="AdamW", momentum=0.0):
        from .optim import make_optimizer
        m = model.module if hasattr(model, "module") else model
        self.primary, self.secondary = (make_optimizer(kind, part, lr, betas=betas, weight_decay=weight_decay, momentum=momentum, eps=eps)
                                        for part in (m.backbone, m.head))
        self.kind = kind
        self._parts = (("backbone.", self.primary), ("head.", self.secondary))
        self._names = [n for n, _ in m.named_parameters()]

    def set_scales(self, lr_scale=None, wd_scale=None):
        """`_FlatOptimizer.set_scales` over names as `MultiCropWrapper.named_parameters()` gives them (`backbone.*`, `head.*`):
        each part gets its own share."""
        split = {prefix: [None, None] for prefix, _ in self._parts}
        for slot, spec in enumerate((lr_scale, wd_scale)):
            if spec is None:
                continue
            if callable(spec):
                for prefix, _ in self._parts:
                    split[prefix][slot] = (lambda n, p, f=spec, pre=prefix: f(pre + n, p))
                continue
            if not isinstance(spec, dict):
                raise TypeError("DinoOptimizer.set_scales: expected None, a dict of parameter name -> float or a callable")
            for prefix, _ in self._parts:
                split[prefix][slot] = {}
            for n, v in spec.items():
                prefix = next((pre for pre, _ in self._parts if n.startswith(pre)), None)
                if prefix is None or n not in self._names:
                    raise ValueError(f"DinoOptimizer.set_scales: the student has no parameter named {n!r}")
                split[prefix][slot][n[len(prefix):]] = v
        for prefix, opt in self._parts:
            opt.set_scales(*split[prefix])
        return self

    def scales(self):
        return {prefix + n: v for prefix, opt in self._parts for n, v in opt.scales().items()}

    @property
    def param_groups(self):
        return self.primary.param_groups

    def zero_grad(self, set_to_none: bool = True):
        self.primary.zero_grad(set_to_none=set_to_none)
        self.secondary.zero_grad(set_to_none=set_to_none)

    def step(self):
        src, dst = self.primary.param_groups[0], self.secondary.param_groups[0]
        for k in ("lr", "weight_decay", "betas", "eps", "momentum"):
            if k in src:
                dst[k] = src[k]
        self.primary.step()
        self.secondary.step()

    # The checkpoint's "optimizer" entry has the reference's layout: ONE optimizer state dict (torch AdamW's by default) over MultiCropWrapper.parameters()
    # (main_pretrain_dino.py:219; misc.py:55-69 loads it back), i.e. state indices 0 .. nb-1 = backbone parameters, nb .. = head
    # parameters, one param group.  The two fused optimizers' dicts are merged / split at nb.
    def _nb(self) -> int:
        return len(self.primary.param_groups[0]["params"])

    def state_dict(self):
        a, b = self.primary.state_dict(), self.secondary.state_dict()
        nb = len(a["param_groups"][0]["params"])
        state = dict(a["state"])
        state.update({nb + i: v for i, v in b["state"].items()})
        group = dict(a["param_groups"][0])
        group["params"] = list(range(nb + len(b["param_groups"][0]["params"])))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        if "backbone" in sd and "head" in sd:  # checkpoints written before the flat layout
            self.primary.load_state_dict(sd["backbone"])
            self.secondary.load_state_dict(sd["head"])
            return
        nb, nh = self._nb(), len(self.secondary.param_groups[0]["params"])
        group = sd["param_groups"][0]
        if len(sd["param_groups"]) != 1 or len(group["params"]) != nb + nh:
            raise ValueError(f"optimizer state of {sum(len(g['params']) for g in sd['param_groups'])} parameters in {len(sd['param_groups'])} "
                             f"group(s) does not match backbone ({nb}) + head ({nh}) in one group")
        ga, gb = dict(group), dict(group)
        ga["params"], gb["params"] = list(range(nb)), list(range(nh))
        self.primary.load_state_dict({"state": {i: v for i, v in sd["state"].items() if i < nb}, "param_groups": [ga]})
        self.secondary.load_state_dict({"state": {i - nb: v for i, v in sd["state"].items() if i >= nb}, "param_groups": [gb]})


class DinoDataParallel(nn.Module):
    """Data-parallel wrapper of a MultiCropWrapper: the backbone's flat gradient is all-reduced in buckets while its staged backward
    is still running (ddp.DistributedDataParallel), the head's (8 % of the parameters) in one all-reduce that the engine issues
    right after `loss.backward()` (`reduce_head_gradients`).  Rank 0's parameters are broadcast at construction."""

    def __init__(self, module, device_ids=None, broadcast_buffers: bool = False, find_unused_parameters: bool = False, bucket_cap_mb: float = 64.0):
        super().__init__()
        from .ddp import DistributedDataParallel
        self.module = module
        self.world_size = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self._backbone_ddp = DistributedDataParallel(module.backbone, bucket_cap_mb=bucket_cap_mb)
        if self.world_size > 1:
            dist.broadcast(module.head._flat, src=0)
            module.head.mark_weights_updated()

    def forward(self, x, masks=None, patch_rows=None):
        if masks is None and patch_rows is None:
            return self.module(x)
        return self.module(x, masks=masks, patch_rows=patch_rows)

    def reduce_head_gradients(self) -> None:
        if self.world_size > 1:
            g = self.module.head._flat_grad
            dist.all_reduce(g)
            g.div_(self.world_size)


class SyntheticCrops:
    """`n_batches` pre-generated multi-crop batches on the device: each a list of `n_crops` tensors [B, C, S, S, S] in [0, 1) (the
    reference resizes global and local crops to one size, transforms.py:75-97, so one backbone pass serves all crops)."""

    def __init__(self, n_batches, batch_size, n_crops, in_chans, size, device, seed=0):
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        self.batches = [[torch.rand(batch_size, in_chans, size, size, size, device=device, generator=gen) for _ in range(n_crops)]
                        for _ in range(n_batches)]

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)
