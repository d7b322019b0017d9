"""Flat parameter / gradient buffers: every Parameter of a model is a view into ONE fp32 buffer, its gradient a view into a
second one.  This is the contract that `HipAdamW`, `clip_gradients` / `clip_grad_norm_`, `ddp.DistributedDataParallel`,
`misc.set_requires_grad_false` and `dino.update_momentum_encoder` rely on (`_flat`, `_flat_grad`, `_layout`,
`flat_segments()`, `mark_weights_updated()`, `_managed_updates`, `_grad_prescale`).

Two layout sources: `FlatModule` packs the parameters in registration order, each starting at a multiple of 1024 elements
(the DINO head, the classification heads); `FlatPlanModule` takes the layout of the native plan (MAE, ViT backbone), whose
staged backward fills the gradient buffer from its end to its start.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._lib import HCT_BF16, HctError
from .dropout import drop_path_rates


class FlatModule(nn.Module):
    """Flat fp32 parameter / gradient buffers in the packed layout.  Subclasses register their parameters, then call
    `_init_flat()`; the buffers are rebuilt on every device move / cast."""

    def _init_flat(self) -> None:
        self._weights_version = 0      # bumped whenever fp32 master weights may have changed
        self._managed_updates = False  # True once a HipAdamW owns the weight updates
        self._grad_prescale = 1.0      # data parallelism: 1 / world
        self._build_flat(torch.device("cpu"))

    def _flat_layout(self) -> Tuple[List[Tuple[str, int, int, Tuple[int, ...], bool, int]], int]:
        """(layout, total): [(name, offset, numel, shape, requires_grad, bf16_t_offset)] and the buffer length."""
        layout, off = [], 0
        for n, p in self.named_parameters():
            layout.append((n, off, p.numel(), tuple(p.shape), bool(p.requires_grad), -1))
            off += (p.numel() + 1023) // 1024 * 1024
        return layout, off

    def _build_flat(self, device: torch.device) -> None:
        layout, total = self._flat_layout()
        named = dict(self.named_parameters())
        flat = torch.zeros(total, dtype=torch.float32, device=device)
        for name, off, numel, shape, _, _ in layout:
            p = named[name]
            flat[off:off + numel].copy_(p.data.reshape(-1).to(device=device, dtype=torch.float32))
            p.data = flat[off:off + numel].view(shape)
            p.grad = None
        self._layout, self._named_cache, self._off = layout, named, {n: o for n, o, *_ in layout}
        self._flat = flat
        self._flat_grad = torch.zeros(total, dtype=torch.float32, device=device)
        self._flat_bf16 = None
        ordered = sorted(layout, key=lambda t: t[1])
        self._seg_names = [n for n, *_ in ordered]
        self._seg_off_host = [o for _, o, *_ in ordered] + [total]
        self._weights_version += 1

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        # parameters were moved/cast one by one; rebuild the flat buffer on their new device
        self._build_flat(next(self.parameters()).device)
        return out

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=False)
        self.mark_weights_updated()
        return out

    def mark_weights_updated(self, plain_bf16_fresh: bool = False) -> None:
        """Tell the model the fp32 master weights changed (optimizer step / manual edit)."""
        self._weights_version += 1

    def flat_segments(self):
        """(names, element offsets[nseg+1]) of the flat parameter/gradient buffers."""
        return self._seg_names, self._seg_off_host

    def _grad_view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Parameter `name`'s slice of the flat gradient (or of a buffer laid out like it), in the parameter's shape."""
        p, o = self._named_cache[name], self._off[name]
        return (self._flat_grad if buf is None else buf)[o:o + p.numel()].view(p.shape)

    def _attach_grads(self) -> None:
        for n, o, numel, shape, rg, _ in self._layout:
            if rg:
                self._named_cache[n].grad = self._flat_grad[o:o + numel].view(shape)


class _Plan:
    """One bound native plan (per batch size and keep count).  `ccfg` / `len_keep`: the config and the kept patches per volume of
    this plan where they are not the model's own (the ViT backbone's patch-dropout plan); every plan of a model has the model's
    parameter layout and is bound to its flat buffers."""

    def __init__(self, model: "FlatPlanModule", batch: int, ccfg=None, len_keep: Optional[int] = None):
        lib = _lib.load()
        self.lib = lib
        self.batch = batch
        self.len_keep = model.len_keep if len_keep is None else int(len_keep)
        self.serial = 0
        self.handle = lib.hct_mae_plan_create(C.byref(model._ccfg if ccfg is None else ccfg), batch, model._dt)
        if not self.handle:
            raise HctError("hct_mae_plan_create: " + lib.hct_last_error_string().decode())
        if lib.hct_mae_plan_len_keep(self.handle) != self.len_keep:
            raise HctError(f"native plan keeps {lib.hct_mae_plan_len_keep(self.handle)} patches, the module {self.len_keep}")
        nbytes = lib.hct_mae_plan_workspace_bytes(self.handle)
        dev = model._flat.device
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.nstages = lib.hct_mae_num_backward_stages(self.handle)
        self.stage_ranges = []
        for s in range(self.nstages):
            b, e = C.c_int64(), C.c_int64()
            _lib.check(lib.hct_mae_backward_stage_range(self.handle, s, C.byref(b), C.byref(e)), "stage_range")
            self.stage_ranges.append((b.value, e.value))
        self.rg_key = None  # requires_grad flags the native plan was last told (FlatPlanModule._sync_frozen)
        self.rebind(model)

    def rebind(self, model):
        _lib.check(self.lib.hct_mae_plan_bind(
            self.handle, model._flat.data_ptr(), model._flat_grad.data_ptr(),
            _lib.ptr(model._flat_bf16), _lib.ptr(model._flat_bf16_t), self.workspace.data_ptr(), self.workspace.numel()),
            "hct_mae_plan_bind")

    def activation(self, name: str) -> torch.Tensor:
        rows, cols, dt = C.c_int64(), C.c_int64(), C.c_int()
        p = self.lib.hct_mae_plan_activation(self.handle, name.encode(), C.byref(rows), C.byref(cols), C.byref(dt))
        if not p:
            raise KeyError(name)
        tdt = {0: torch.float32, 1: torch.bfloat16, 2: torch.int32}[dt.value]
        off = p - self.workspace.data_ptr()
        n = rows.value * cols.value
        esz = torch.empty(0, dtype=tdt).element_size()
        return self.workspace[off:off + n * esz].view(tdt).view(rows.value, cols.value)

    def __del__(self):
        try:
            if self.handle:
                self.lib.hct_mae_plan_destroy(self.handle)
        except Exception:
            pass


class FlatPlanModule(FlatModule):
    """Host side shared by the plan-driven models (MAE, ViT backbone): the flat buffers are laid out by the native plan, the
    staged native backward fills the gradient buffer from its end to its start (= gradient-bucket order for the data-parallel
    all-reduce), bf16 working copies are refreshed when the masters change.  Subclasses register their parameters under the
    reference's names, fill `self._ccfg` / `self._dt`, then call `_init_flat()`."""

    def _init_flat(self) -> None:
        self._plans: Dict[Tuple[int, int], _Plan] = {}  # by (batch, kept patches per volume)
        self._shadow_version = -1      # version the bf16 working copies correspond to
        self._bucket_hook: Optional[Callable[[int, int, int], None]] = None  # (stage, begin, end): gradient range that became final
        self.wgrad_group_blocks: Optional[int] = None  # data parallelism: flush the queued weight gradients every n block stages
        self._post_backward_hook: Optional[Callable[[], None]] = None
        self._grad_overwrite = True    # next backward overwrites the flat gradient (set by zero_grad paths)
        self._plain_fresh = False
        self._frozen_written: List[Tuple[int, int]] = []  # (offset, numel) of frozen parameters whose gradient the backward still writes
        super()._init_flat()

    def _flat_layout(self):
        lib = _lib.load()
        h = lib.hct_mae_plan_create(C.byref(self._ccfg), 1, self._dt)
        if not h:
            raise HctError("hct_mae_plan_create: " + lib.hct_last_error_string().decode())
        try:
            layout = []
            info = _lib.ParamInfo()
            for i in range(lib.hct_mae_plan_num_params(h)):
                _lib.check(lib.hct_mae_plan_param_info(h, i, C.byref(info)), "param_info")
                shape = tuple(int(info.shape[k]) for k in range(info.ndim))
                layout.append((info.name.decode(), int(info.offset), int(info.numel), shape, bool(info.requires_grad), int(info.bf16_t_offset)))
            total = int(lib.hct_mae_plan_param_elems(h))
            self._bf16_t_elems = int(lib.hct_mae_plan_bf16_t_elems(h))
        finally:
            lib.hct_mae_plan_destroy(h)
        named = dict(self.named_parameters())
        if set(named) != {n for n, *_ in layout}:
            raise HctError(f"parameter name mismatch between host module and native plan: {set(named) ^ {n for n, *_ in layout}}")
        for name, _, _, shape, _, _ in layout:
            if tuple(named[name].shape) != shape:
                raise HctError(f"shape mismatch for {name}: {tuple(named[name].shape)} vs {shape}")
        return layout, total

    def _build_flat(self, device: torch.device) -> None:
        old_grads = {n: p.grad for n, p in self.named_parameters()}
        super()._build_flat(device)
        total = self._flat.numel()
        for name, off, numel, shape, rg, _ in self._layout:
            p = self._named_cache[name]
            p.requires_grad_(rg and p.requires_grad)
            g = old_grads[name]
            if g is not None:  # a gradient held from before the move stays
                self._flat_grad[off:off + numel].copy_(g.reshape(-1))
                p.grad = self._flat_grad[off:off + numel].view(shape)
        if self._dt == HCT_BF16:
            self._flat_bf16 = torch.zeros(total, dtype=torch.bfloat16, device=device)
            self._flat_bf16_t = torch.zeros(max(self._bf16_t_elems, 1), dtype=torch.bfloat16, device=device)
        else:
            self._flat_bf16 = self._flat_bf16_t = None
        self._plans = {}
        self._plain_fresh = False

    def mark_weights_updated(self, plain_bf16_fresh: bool = False) -> None:
        super().mark_weights_updated()
        self._plain_fresh = plain_bf16_fresh  # False: the bf16 copies written by the last optimizer step no longer match

    # ------------------------------------------------------------------------------------------
    # dropout and drop path (dropout.py): a forward is "dropping" in training mode when elements drop (dropout_rate > 0) or some block
    # drops paths (a q_j > 0); one 64-bit seed per dropping forward serves both
    def _init_dropout(self, dropout_rate: float, drop_path_rate: float = 0.0, depth: int = 1) -> None:
        self.dropout_rate = float(dropout_rate)
        self.drop_path_rate = float(drop_path_rate)
        self._drops_paths = any(q > 0.0 for q in drop_path_rates(drop_path_rate, depth))
        self.last_dropout_seed: Optional[int] = None  # seed of the last forward that dropped
        self._next_dropout_seed: Optional[int] = None

    def set_dropout_seed(self, seed: int) -> None:
        """Pin the seed of the next forward that drops (tests, reproductions); later forwards draw their own again."""
        self._next_dropout_seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def _arm_dropout(self, plan: _Plan) -> bool:
        """Tell the plan whether the coming forward drops, and with which seed.  The seed comes from torch's CPU default generator (no
        device sync, reproducible under torch.manual_seed, different per rank through SEED + rank); nothing is drawn at rates 0 or in
        eval mode, so the random streams of such runs stay where they were."""
        can = getattr(self, "dropout_rate", 0.0) > 0.0 or getattr(self, "_drops_paths", False)
        active = bool(self.training and can)
        seed = 0
        if active:
            if self._next_dropout_seed is not None:
                seed, self._next_dropout_seed = self._next_dropout_seed, None
            else:
                lo, hi = (int(v) for v in torch.randint(0, 1 << 32, (2,), dtype=torch.int64))
                seed = lo | (hi << 32)
            self.last_dropout_seed = seed
        if can:
            plan.lib.hct_mae_plan_set_dropout(plan.handle, int(active), seed)
        return active

    def _plan_for(self, batch: int, ccfg=None, len_keep: Optional[int] = None) -> _Plan:
        """The plan of `batch` volumes: the model's own, or with `ccfg` / `len_keep` the one that keeps `len_keep` patches per volume.
        Both kinds of one batch size live side by side over the same flat buffers, each with its own workspace and serial."""
        if not self._flat.is_cuda:
            raise HctError(f"{type(self).__name__} (HIP) needs its parameters on a GPU: call .to('cuda') first; "
                           "there is no CPU fallback for this path")
        key = (batch, self.len_keep if len_keep is None else int(len_keep))
        plan = self._plans.get(key)
        if plan is None:
            plan = _Plan(self, batch, ccfg, len_keep)
            self._plans[key] = plan
        return plan

    def _ensure_weights_fresh(self, plan: _Plan, st: int) -> None:
        if self._dt != HCT_BF16:
            return
        # unless a fused optimizer reports every update (mark_weights_updated), assume the fp32 masters may
        # have been modified behind our back (e.g. torch.optim.AdamW) and refresh on every forward.
        if self._managed_updates and self._shadow_version == self._weights_version:
            return
        with_plain = 0 if getattr(self, "_plain_fresh", False) else 1
        _lib.check(plan.lib.hct_mae_refresh_weights(plan.handle, with_plain, st), "hct_mae_refresh_weights")
        self._plain_fresh = False
        self._shadow_version = self._weights_version

    # gradients that ride in another kernel's epilogue are written whatever the flag says (include/headct_hip.h,
    # hct_mae_plan_set_requires_grad), and so are the MAE's two decoder tokens when the first decoder block runs on cat rows; every
    # other frozen parameter is skipped by the native backward
    _EPILOGUE_GRADS = ("norm.weight", "norm.bias", "proj.bias", "linear1.bias", "linear2.bias", "mask_token", "decoder_cls_token")

    def _sync_frozen(self, plan: "_Plan") -> None:
        """Tell the native plan which parameters are frozen (`requires_grad False`): it skips their weight-gradient products.  A frozen
        parameter's slice of the flat gradient stays zero, so norms over the flat buffer are norms of the trainable gradients."""
        named = self._named_cache
        key = tuple(named[n].requires_grad for n, *_ in self._layout)
        if plan.rg_key == key:
            return
        self._frozen_written = []
        for i, ((name, off, numel, *_), rg) in enumerate(zip(self._layout, key)):
            _lib.check(plan.lib.hct_mae_plan_set_requires_grad(plan.handle, i, int(rg)), "hct_mae_plan_set_requires_grad")
            if not rg:
                named[name].grad = None
                self._flat_grad[off:off + numel].zero_()
                if name.endswith(self._EPILOGUE_GRADS):
                    self._frozen_written.append((off, numel))
        plan.rg_key = key

    def _attach_grads(self) -> bool:
        """Point every trainable parameter's .grad at its slice of the flat gradient buffer.
        Returns True when some parameter already held a gradient (accumulation requested)."""
        accumulate = False
        named = self._named_cache
        for name, off, numel, shape, rg, _ in self._layout:
            p = named[name]
            if not p.requires_grad:
                continue
            view = self._flat_grad[off:off + numel].view(shape)
            if p.grad is None:
                p.grad = view
            elif p.grad.data_ptr() == view.data_ptr():
                accumulate = accumulate or not self._grad_overwrite
            else:  # foreign gradient tensor: fold it in
                view.copy_(p.grad)
                p.grad = view
                accumulate = True
        return accumulate

    def _run_backward(self, plan: _Plan, x: torch.Tensor, grad_out: torch.Tensor) -> None:
        """MAE: the staged native backward seeded by the (device) scalar dLoss."""
        lib = plan.lib
        g = grad_out.detach().to(dtype=torch.float32).reshape(1).contiguous()
        _lib.check(lib.hct_mae_set_loss_grad(plan.handle, g.data_ptr()), "hct_mae_set_loss_grad")
        self._keep_alive = g
        st = _lib.stream_ptr()
        self._run_staged_backward(plan, lambda s: lib.hct_mae_backward_stage(plan.handle, s, st), "hct_mae_backward_stage")

    def _run_staged_backward(self, plan: _Plan, stage_call, what: str) -> None:
        lib = plan.lib
        # a second backward without zero_grad() adds to what is there (torch semantics).  The native stages overwrite the
        # flat buffer, so the earlier gradient is parked and added back at the end -- AFTER the data-parallel reduction of
        # the fresh gradient (every backward is reduced, as torch's DDP does; the parked part is already the mean).
        parked = None
        if not self._grad_overwrite and any(p.grad is not None for p in self.parameters()):
            self._attach_grads()  # a foreign / preset .grad tensor is folded into the flat buffer first
            parked = self._flat_grad.clone()
        # weight gradients are queued across stages and run in grouped launches (csrc/mae_plan.hip: flush_wgrads), so a stage's
        # range is final only when the plan's watermark has passed it: the bucket hook gets [watermark, previous watermark)
        if self._bucket_hook is not None and getattr(self, "wgrad_group_blocks", None) is not None and getattr(plan, "_wg_blocks", None) != self.wgrad_group_blocks:
            lib.hct_mae_plan_set_wgrad_defer(plan.handle, 1, int(self.wgrad_group_blocks))
            plan._wg_blocks = self.wgrad_group_blocks
        final = self._flat_grad.numel()
        for s in range(plan.nstages):
            _lib.check(stage_call(s), f"{what}({s})")
            if self._bucket_hook is not None:
                now = int(lib.hct_mae_backward_final_offset(plan.handle))
                if now < final:
                    self._bucket_hook(s, now, final)
                    final = now
        if self._post_backward_hook is not None:
            self._post_backward_hook()  # data parallel: the compute stream now waits for the collectives
        for off, numel in self._frozen_written:
            self._flat_grad[off:off + numel].zero_()
        if parked is not None:
            self._flat_grad.add_(parked)
        self._attach_grads()
        self._grad_overwrite = False

    def zero_grad(self, set_to_none: bool = True) -> None:
        super().zero_grad(set_to_none=set_to_none)
        self._grad_overwrite = True
